"""RGB pictures (BT.709) on the GPU and PNG files on the host (test_video.py:55-64, 87-122, 366-370; src/utils/transforms.py:17-27,
53-66; metrics.py:10-24 calc_psnr; video_reader.py:10-45 PNGReader; video_writer.py:9-30 PNGWriter).

Thin wrappers over the C-ABI entry points ``dcvc_rgb_to_x``, ``dcvc_x_to_rgb``, ``dcvc_sse`` (include/dcvc_amd_ops.h) and
``dcvc_png_*`` (include/dcvc_amd_image.h). Device operands are CUDA tensors; the kernels run on ``torch.cuda.current_stream()``.
The arithmetic is that of the reference's torch ops on a GPU, where a tensor divided by a scalar is a * fp32(1 / b).
``rgb_to_x`` / ``x_to_rgb`` with another colour matrix or range go through ``dcvc_rgb_to_x_cs`` / ``dcvc_x_to_rgb_cs``.
``rgb16_to_x`` / ``x_to_rgb16`` are the 9..16-bit pair (``dcvc_rgb16_to_x_cs`` / ``dcvc_x_to_rgb16_cs``) on 16-bit
samples in the storage ``yuv16`` uses (``torch.uint16`` or ``torch.int16`` read as unsigned); ``read_png16`` / ``write_png16``
are the 16-bit PNG files.
"""
import ctypes
import os
import re

import numpy as np

from . import _lib

DCVC_SAMPLE_U8 = 0
DCVC_SAMPLE_F16 = 1
MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}      # DCVC_MATRIX_*
RANGES = {"full": 0, "limited": 1}                    # DCVC_RANGE_*

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_fns = {}
_SIGS = {
    "dcvc_rgb_to_x": [_vp, _ll, _ll, _ll, _ci, _ci, _vp, _ci, _vp, _vp],
    "dcvc_x_to_rgb": [_vp, _ci, _ci, _ci, _vp, _vp, _vp],
    "dcvc_rgb_to_x_cs": [_vp, _ll, _ll, _ll, _ci, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _vp],
    "dcvc_x_to_rgb_cs": [_vp, _ci, _ci, _ci, _vp, _vp, _ci, _ci, _ci, _vp],
    "dcvc_sse": [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ll, _vp, _vp],
    "dcvc_png_info": [ctypes.c_char_p, ctypes.POINTER(_ci), ctypes.POINTER(_ci)],
    "dcvc_png_read_rgb": [ctypes.c_char_p, _vp, ctypes.c_size_t, ctypes.POINTER(_ci), ctypes.POINTER(_ci)],
    "dcvc_png_write_rgb": [ctypes.c_char_p, _vp, _ci, _ci],
    "dcvc_rgb16_to_x_cs": [_vp, _ll, _ll, _ll, _ci, _ci, _ci, _vp, _ci, _vp, _ci, _ci, _ci, _vp],
    "dcvc_x_to_rgb16_cs": [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _ci, _ci, _ci, _vp],
    "dcvc_msssim_range_ws": [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ll, ctypes.c_double, _vp, _vp, _ll, _vp],
    "dcvc_png_info2": [ctypes.c_char_p, ctypes.POINTER(_ci), ctypes.POINTER(_ci), ctypes.POINTER(_ci)],
    "dcvc_png_read_rgb16": [ctypes.c_char_p, _vp, ctypes.c_size_t, ctypes.POINTER(_ci), ctypes.POINTER(_ci)],
    "dcvc_png_write_rgb16": [ctypes.c_char_p, _vp, _ci, _ci],
}


def _fn(name):
    if name not in _fns:
        _fns[name] = _lib.fn(name, _ci, _SIGS[name])
    return _fns[name]


def _stream(t):
    import torch
    return _vp(torch.cuda.current_stream(t.device).cuda_stream)


def _u8_picture(rgb):
    """(tensor, row, pixel, channel strides) of a [3, H, W] or [H, W, 3] uint8 CUDA tensor"""
    import torch
    if rgb.dtype != torch.uint8 or not rgb.is_cuda or rgb.dim() != 3:
        raise ValueError("rgb: a uint8 CUDA tensor [3, H, W] or [H, W, 3] expected, got %s %s"
                         % (rgb.dtype, tuple(rgb.shape)))
    if rgb.shape[0] == 3 and rgb.shape[2] != 3:
        _, H, W = rgb.shape
        return H, W, rgb.stride(1), rgb.stride(2), rgb.stride(0)
    if rgb.shape[2] == 3:
        H, W, _ = rgb.shape
        return H, W, rgb.stride(0), rgb.stride(1), rgb.stride(2)
    raise ValueError("rgb: a uint8 CUDA tensor [3, H, W] or [H, W, 3] expected, got %s" % (tuple(rgb.shape),))


def _colour(matrix, range, yuv_depth):
    """None for the reference's conversion (bt709, full, 8: the entry points without _cs), else the three codes"""
    if matrix not in MATRICES:
        raise ValueError("unknown matrix %r (bt601, bt709 or bt2020)" % (matrix,))
    if range not in RANGES:
        raise ValueError("unknown range %r (full or limited)" % (range,))
    if (matrix, range, yuv_depth) == ("bt709", "full", 8):
        return None
    return MATRICES[matrix], RANGES[range], int(yuv_depth)


def rgb_to_x(rgb, ldx=3, x=None, planar=False, matrix="bt709", range="full", yuv_depth=8):
    """get_src_frame's model input of one RGB picture: [H, W, 3] fp16 (NHWC, x = rgb2ycbcr(rgb / 255).half() - 0.5).
    rgb: uint8 CUDA tensor [3, H, W] or [H, W, 3] (any strides). With ``x`` given, writes into it at pixel stride ``ldx``
    (a flat fp16 tensor view starting at the picture's first channel, e.g. a chunk slot) instead. planar=True also returns a
    [3, H, W] uint8 copy of the source: (x, planar). matrix ("bt601", "bt709", "bt2020"), range ("full", "limited") and
    yuv_depth (8..16, the depth of the YUV samples x stands for, which places the limited-range levels) choose the
    conversion (dcvc_rgb_to_x_cs); the defaults are the reference's and call dcvc_rgb_to_x."""
    import torch
    colour = _colour(matrix, range, yuv_depth)
    H, W, rs, ps, cs = _u8_picture(rgb)
    if x is None:
        if ldx != 3:
            raise ValueError("rgb_to_x: ldx != 3 needs an output tensor")
        x = torch.empty((H, W, 3), dtype=torch.float16, device=rgb.device)
    elif x.dtype != torch.float16 or not x.is_cuda or x.numel() < (H * W - 1) * ldx + 3:
        raise ValueError("rgb_to_x: x must be a CUDA float16 tensor of at least (H W - 1) ldx + 3 elements")
    pl = torch.empty((3, H, W), dtype=torch.uint8, device=rgb.device) if planar else None
    args = (_vp(rgb.data_ptr()), rs, ps, cs, H, W, _vp(x.data_ptr()), ldx, _vp(pl.data_ptr()) if pl is not None else None)
    if colour is None:
        _lib.check(_fn("dcvc_rgb_to_x")(*args, _stream(rgb)))
    else:
        _lib.check(_fn("dcvc_rgb_to_x_cs")(*args, *colour, _stream(rgb)))
    return (x, pl) if planar else x


def x_to_rgb(x_hat, H, W, matrix="bt709", range="full", yuv_depth=8):
    """get_distortion's RGB planes and the writer's pixels of a decoded picture. x_hat: fp16 CUDA tensor [1, 3, Hp, Wp]
    (channels_last) or [Hp, Wp, 3], Hp >= H, Wp >= W. Returns (rgb16 [3, H, W] fp16 in 0..255, rgb8 [H, W, 3] uint8).
    matrix, range and yuv_depth as for rgb_to_x (dcvc_x_to_rgb_cs; the defaults call dcvc_x_to_rgb)."""
    import torch
    colour = _colour(matrix, range, yuv_depth)
    if x_hat.dim() == 4:
        x_hat = x_hat[0].permute(1, 2, 0)
    if x_hat.dtype != torch.float16 or not x_hat.is_cuda or x_hat.dim() != 3 or x_hat.shape[2] != 3:
        raise ValueError("x_to_rgb: a float16 CUDA tensor [1, 3, Hp, Wp] or [Hp, Wp, 3] expected")
    x_hat = x_hat.contiguous()
    if x_hat.shape[0] < H or x_hat.shape[1] < W:
        raise ValueError("x_to_rgb: x_hat (%d x %d) is smaller than the picture (%d x %d)" % (x_hat.shape[1], x_hat.shape[0], W, H))
    rgb16 = torch.empty((3, H, W), dtype=torch.float16, device=x_hat.device)
    rgb8 = torch.empty((H, W, 3), dtype=torch.uint8, device=x_hat.device)
    args = (_vp(x_hat.data_ptr()), x_hat.shape[1], H, W, _vp(rgb16.data_ptr()), _vp(rgb8.data_ptr()))
    if colour is None:
        _lib.check(_fn("dcvc_x_to_rgb")(*args, _stream(x_hat)))
    else:
        _lib.check(_fn("dcvc_x_to_rgb_cs")(*args, *colour, _stream(x_hat)))
    return rgb16, rgb8


def _code(t):
    import torch
    if t.dtype == torch.uint8:
        return DCVC_SAMPLE_U8
    if t.dtype == torch.float16:
        return DCVC_SAMPLE_F16
    raise TypeError("sse: planes must be uint8 or float16, got %s" % t.dtype)


def sse(src, rec):
    """fp64 sum of squared differences of every plane pair: src / rec CUDA tensors [P, H, W] or [H, W] (uint8 or float16;
    the two dtypes may differ). Returns a float64 numpy array of P values."""
    import torch
    if src.shape != rec.shape or src.dim() not in (2, 3):
        raise ValueError("sse: src and rec must share a [P, H, W] or [H, W] shape, got %s and %s"
                         % (tuple(src.shape), tuple(rec.shape)))
    if not (src.is_cuda and rec.is_cuda) or src.device != rec.device:
        raise ValueError("sse: src and rec must be CUDA tensors on one device")
    codes = _code(src), _code(rec)
    if src.dim() == 2:
        src, rec = src[None], rec[None]
    if src.stride(2) != 1 or src.stride() != rec.stride():
        src, rec = src.contiguous(), rec.contiguous()
    P, H, W = src.shape
    out = torch.empty(P, dtype=torch.float64, device=src.device)
    _lib.check(_fn("dcvc_sse")(_vp(src.data_ptr()), codes[0], _vp(rec.data_ptr()), codes[1], P, H, W, src.stride(1),
                               src.stride(0), _vp(out.data_ptr()), _stream(src)))
    return out.cpu().numpy()


def psnr_from_sse(total, n):
    """metrics.py:10-24 calc_psnr from the fp64 sum of squares over n samples"""
    mse = total / n
    if np.isnan(mse) or np.isinf(mse):
        return -999.9
    p = 10 * np.log10(255.0 * 255.0 / mse) if mse > 1e-10 else 999.9
    return float(min(p, 99.9))


def psnr_rgb(src, rec16):
    """calc_psnr(rgb, rgb_rec) over all 3 H W samples: src [3, H, W] uint8, rec16 [3, H, W] fp16 (x_to_rgb's planes)"""
    return psnr_from_sse(float(sse(src, rec16).sum()), src.numel())


# ------------------------------------------------------------------------------------------------------------ 9..16 bits
def _u16_picture(rgb):
    """(H, W, row, pixel, channel strides in samples) of a [3, H, W] or [H, W, 3] 16-bit CUDA tensor"""
    from . import yuv16
    if rgb.dtype not in yuv16._u16_dtypes() or not rgb.is_cuda or rgb.dim() != 3:
        raise ValueError("rgb: a uint16 / int16 (unsigned samples) CUDA tensor [3, H, W] or [H, W, 3] expected, got %s %s"
                         % (rgb.dtype, tuple(rgb.shape)))
    if rgb.shape[0] == 3 and rgb.shape[2] != 3:
        _, H, W = rgb.shape
        return H, W, rgb.stride(1), rgb.stride(2), rgb.stride(0)
    if rgb.shape[2] == 3:
        H, W, _ = rgb.shape
        return H, W, rgb.stride(0), rgb.stride(1), rgb.stride(2)
    raise ValueError("rgb: a 16-bit CUDA tensor [3, H, W] or [H, W, 3] expected, got %s" % (tuple(rgb.shape),))


def _colour16(matrix, range, yuv_depth):
    if matrix not in MATRICES:
        raise ValueError("unknown matrix %r (bt601, bt709 or bt2020)" % (matrix,))
    if range not in RANGES:
        raise ValueError("unknown range %r (full or limited)" % (range,))
    return MATRICES[matrix], RANGES[range], int(yuv_depth)


def rgb16_to_x(rgb, bit_depth, ldx=3, x=None, planar=False, matrix="bt709", range="full", yuv_depth=8):
    """The model input of one 9..16-bit RGB picture: [H, W, 3] fp16, rgb_to_x's conversion of fp32(v) / fp32(2^bit_depth - 1)
    (a true division; dcvc_rgb16_to_x_cs). rgb: uint16 / int16 (read as unsigned) CUDA tensor [3, H, W] or
    [H, W, 3], any strides. x, ldx, matrix, range and yuv_depth as for rgb_to_x; planar=True also returns a [3, H, W] copy
    of the source in yuv16.u16_dtype(): (x, planar)."""
    import torch
    from . import yuv16
    colour = _colour16(matrix, range, yuv_depth)
    H, W, rs, ps, cs = _u16_picture(rgb)
    if x is None:
        if ldx != 3:
            raise ValueError("rgb16_to_x: ldx != 3 needs an output tensor")
        x = torch.empty((H, W, 3), dtype=torch.float16, device=rgb.device)
    elif x.dtype != torch.float16 or not x.is_cuda or x.numel() < (H * W - 1) * ldx + 3:
        raise ValueError("rgb16_to_x: x must be a CUDA float16 tensor of at least (H W - 1) ldx + 3 elements")
    pl = torch.empty((3, H, W), dtype=torch.int16, device=rgb.device) if planar else None
    _lib.check(_fn("dcvc_rgb16_to_x_cs")(_vp(rgb.data_ptr()), rs, ps, cs, int(bit_depth), H, W, _vp(x.data_ptr()), ldx,
                                         _vp(pl.data_ptr()) if pl is not None else None, *colour, _stream(rgb)))
    return (x, pl.view(yuv16.u16_dtype())) if planar else x


def x_to_rgb16(x_hat, H, W, bit_depth, matrix="bt709", range="full", yuv_depth=8):
    """The distortion planes and the writer's pixels of a decoded picture at 9..16 bits. x_hat as for x_to_rgb. Returns
    (dist32 [3, H, W] fp32 in 0..2^bit_depth - 1, rgb16 [H, W, 3] in yuv16.u16_dtype() = rint(dist32))."""
    import torch
    from . import yuv16
    colour = _colour16(matrix, range, yuv_depth)
    if x_hat.dim() == 4:
        x_hat = x_hat[0].permute(1, 2, 0)
    if x_hat.dtype != torch.float16 or not x_hat.is_cuda or x_hat.dim() != 3 or x_hat.shape[2] != 3:
        raise ValueError("x_to_rgb16: a float16 CUDA tensor [1, 3, Hp, Wp] or [Hp, Wp, 3] expected")
    x_hat = x_hat.contiguous()
    if x_hat.shape[0] < H or x_hat.shape[1] < W:
        raise ValueError("x_to_rgb16: x_hat (%d x %d) is smaller than the picture (%d x %d)" % (x_hat.shape[1], x_hat.shape[0], W, H))
    dist = torch.empty((3, H, W), dtype=torch.float32, device=x_hat.device)
    out = torch.empty((H, W, 3), dtype=torch.int16, device=x_hat.device)
    _lib.check(_fn("dcvc_x_to_rgb16_cs")(_vp(x_hat.data_ptr()), x_hat.shape[1], H, W, int(bit_depth), _vp(dist.data_ptr()),
                                         _vp(out.data_ptr()), *colour, _stream(x_hat)))
    return dist, out.view(yuv16.u16_dtype())


def psnr_rgb16(src, dist32, bit_depth):
    """calc_psnr at the data range 2^bit_depth - 1 over all 3 H W samples, as the dcvc tool logs it (dcvc_sse over the three
    planes, the sums added in the order (R + G) + B, the C library's log10): src [3, H, W] 16-bit samples (rgb16_to_x's
    planar copy), dist32 [3, H, W] fp32 (x_to_rgb16's planes)"""
    import math
    from . import yuv16
    s = yuv16.sse(src, dist32)
    peak = float(yuv16.max_val(bit_depth))
    mse = float((s[0] + s[1]) + s[2]) / float(src.numel())
    if math.isnan(mse) or math.isinf(mse):
        return -999.9
    p = 10.0 * math.log10(peak * peak / mse) if mse > 1e-10 else 999.9
    return p if p < 99.9 else 99.9


def msssim_rgb16(src, dist32, bit_depth):
    """the mean of the three planes' MS-SSIM at data_range = 2^bit_depth - 1 (calc_msssim_rgb's rule): three
    dcvc_msssim_range_ws calls, R, G, B one after the other on one workspace of the caller, as the dcvc tool makes them.
    src [3, H, W] 16-bit samples, dist32 [3, H, W] fp32, both contiguous."""
    import torch
    from . import yuv16
    if src.shape != dist32.shape or src.dim() != 3 or src.shape[0] != 3 or not (src.is_contiguous() and dist32.is_contiguous()):
        raise ValueError("msssim_rgb16: contiguous [3, H, W] planes expected, got %s and %s" % (tuple(src.shape), tuple(dist32.shape)))
    if src.dtype not in yuv16._u16_dtypes() or dist32.dtype != torch.float32 or not (src.is_cuda and dist32.is_cuda):
        raise ValueError("msssim_rgb16: 16-bit samples and float32 planes on the device expected, got %s and %s" % (src.dtype, dist32.dtype))
    _, H, W = src.shape
    nbytes = int(_lib.fn("dcvc_msssim_workspace_bytes", _ll, [_ci, _ci, _ci])(1, H, W))
    if nbytes <= 0:
        raise ValueError("msssim_rgb16: both sides must be >= 88, got %dx%d" % (W, H))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    out = torch.empty(3, dtype=torch.float64, device=src.device)
    f = _fn("dcvc_msssim_range_ws")
    for q in (0, 1, 2):
        _lib.check(f(_vp(src[q].data_ptr()), yuv16.DCVC_SAMPLE_U16, _vp(dist32[q].data_ptr()), yuv16.DCVC_SAMPLE_F32, 1, H, W, W, H * W,
                     float(yuv16.max_val(bit_depth)), _vp(out[q:].data_ptr()), _vp(ws.data_ptr()), nbytes, _stream(src)))
    v = out.cpu().numpy()
    return float(((0.0 + v[0]) + v[1] + v[2]) / 3)


# ------------------------------------------------------------------------------------------------------------------ PNG
def png_info2(path):
    """(width, height, bit_depth) of a PNG file; bit_depth is 8 or 16"""
    w, h, d = _ci(), _ci(), _ci()
    _lib.check(_fn("dcvc_png_info2")(os.fsencode(path), ctypes.byref(w), ctypes.byref(h), ctypes.byref(d)))
    return w.value, h.value, d.value


def read_png16(path):
    """the pixels of a 16-bit PNG file as a [H, W, 3] uint16 numpy array (grey replicated, alpha dropped)"""
    w, h, d = png_info2(path)
    out = np.empty((h, w, 3), dtype=np.uint16)
    gw, gh = _ci(), _ci()
    _lib.check(_fn("dcvc_png_read_rgb16")(os.fsencode(path), _vp(out.ctypes.data), out.nbytes, ctypes.byref(gw), ctypes.byref(gh)))
    if (gw.value, gh.value) != (w, h):
        raise _lib.DcvcError("%s changed while it was read" % path)
    return out


def write_png16(path, rgb):
    """writes [H, W, 3] 16-bit pixels (a uint16 numpy array, or a uint16 / int16-storage tensor, which is copied to the host)
    as a 16-bit RGB PNG"""
    if hasattr(rgb, "detach"):
        import torch
        rgb = rgb.detach().cpu().view(torch.int16).numpy().view(np.uint16)
    rgb = np.ascontiguousarray(rgb)
    if rgb.dtype != np.uint16 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("write_png16: [H, W, 3] uint16 pixels expected, got %s %s" % (rgb.dtype, rgb.shape))
    _lib.check(_fn("dcvc_png_write_rgb16")(os.fsencode(path), _vp(rgb.ctypes.data), rgb.shape[1], rgb.shape[0]))


def png_info(path):
    """(width, height) of a PNG file"""
    w, h = _ci(), _ci()
    _lib.check(_fn("dcvc_png_info")(os.fsencode(path), ctypes.byref(w), ctypes.byref(h)))
    return w.value, h.value


def read_png(path):
    """PNGReader's pixels (convert('RGB')) as a [H, W, 3] uint8 numpy array"""
    w, h = png_info(path)
    out = np.empty((h, w, 3), dtype=np.uint8)
    gw, gh = _ci(), _ci()
    _lib.check(_fn("dcvc_png_read_rgb")(os.fsencode(path), _vp(out.ctypes.data), out.nbytes, ctypes.byref(gw), ctypes.byref(gh)))
    if (gw.value, gh.value) != (w, h):
        raise _lib.DcvcError("%s changed while it was read" % path)
    return out


def write_png(path, rgb):
    """writes [H, W, 3] uint8 pixels (numpy, or a tensor, which is copied to the host) as an 8-bit RGB PNG"""
    if hasattr(rgb, "detach"):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("write_png: [H, W, 3] pixels expected, got %s" % (rgb.shape,))
    _lib.check(_fn("dcvc_png_write_rgb")(os.fsencode(path), _vp(rgb.ctypes.data), rgb.shape[1], rgb.shape[0]))


def png_naming(directory):
    """PNGReader's naming rule: 'im1.png' -> 1 digit, 'im00001.png' -> 5 digits (zero padded); anything else is an error"""
    names = set(os.listdir(directory))
    if "im1.png" in names:
        return 1
    if "im00001.png" in names:
        return 5
    raise ValueError("%s: unknown image naming convention (im1.png or im00001.png expected)" % directory)


def png_sequence(directory, start=1):
    """yields the [H, W, 3] uint8 pictures im<n>.png of a directory from n = start until the first missing number"""
    pad = png_naming(directory)
    n = start
    while True:
        path = os.path.join(directory, "im%s.png" % str(n).zfill(pad))
        if not os.path.exists(path):
            return
        yield read_png(path)
        n += 1


__all__ = ["rgb_to_x", "x_to_rgb", "sse", "psnr_rgb", "psnr_from_sse", "png_info", "read_png", "write_png", "png_naming",
           "png_sequence", "rgb16_to_x", "x_to_rgb16", "psnr_rgb16", "msssim_rgb16", "png_info2", "read_png16", "write_png16",
           "DCVC_SAMPLE_U8", "DCVC_SAMPLE_F16", "MATRICES", "RANGES"]
