"""4:2:0, 4:2:2, 4:4:4 planar and NV12 / P010 pictures of 8..16 bits on the GPU, and Y4M headers.

Thin wrappers over the C-ABI entry points ``dcvc_pix_picture_samples``, ``dcvc_pix_to_x`` and ``dcvc_x_to_pix``
(include/dcvc_amd_ops.h) and ``dcvc_y4m_*`` (include/dcvc_amd_image.h). Device operands are CUDA tensors; the kernels run on
``torch.cuda.current_stream()``. A picture is one flat tensor in file layout: Y [H][W], then Cb and Cr as planes [2][Hc][Wc]
or, for NV12, interleaved [Hc][Wc][2]. 8 bits: ``torch.uint8``; 9..16 bits: 16-bit samples as yuv16.py takes and returns them
(``torch.uint16`` or ``torch.int16`` storage read as unsigned in, ``yuv16.u16_dtype()`` out), LSB-aligned in the planar
formats and in the high bits for NV12 (P010 / P012 / P016).
"""
import ctypes

from . import _lib
from .yuv16 import _u16_dtypes, msssim, psnr_from_sse, sse, u16_dtype

DCVC_PIX_YUV420P = 0
DCVC_PIX_YUV422P = 1
DCVC_PIX_YUV444P = 2
DCVC_PIX_NV12 = 3
FORMATS = {"yuv420": DCVC_PIX_YUV420P, "yuv422": DCVC_PIX_YUV422P, "yuv444": DCVC_PIX_YUV444P, "nv12": DCVC_PIX_NV12}

_vp, _ci, _ll, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t
_fns = {}


class Y4mInfo(ctypes.Structure):
    """dcvc_y4m_info"""
    _fields_ = [("width", _ci), ("height", _ci), ("fps_num", _ci), ("fps_den", _ci), ("pix_fmt", _ci), ("bit_depth", _ci),
                ("header_bytes", _ll)]


_SIGS = {
    "dcvc_pix_picture_samples": (_ll, [_ci, _ci, _ci]),
    "dcvc_pix_to_x": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _ci, _vp, _vp]),
    "dcvc_x_to_pix": (_ci, [_vp, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _vp]),
    "dcvc_y4m_parse_header": (_ci, [ctypes.c_char_p, _sz, ctypes.POINTER(Y4mInfo)]),
    "dcvc_y4m_parse_header_i": (_ci, [ctypes.c_char_p, _sz, ctypes.POINTER(Y4mInfo), ctypes.POINTER(_ci)]),
    "dcvc_y4m_frame_header_bytes": (_ci, [ctypes.c_char_p, _sz]),
    "dcvc_y4m_write_header": (_ci, [ctypes.c_char_p, _sz, ctypes.POINTER(Y4mInfo)]),
}


def _fn(name):
    if name not in _fns:
        _fns[name] = _lib.fn(name, *_SIGS[name])
    return _fns[name]


def _stream(t):
    import torch
    return _vp(torch.cuda.current_stream(t.device).cuda_stream)


def max_val(bit_depth):
    """the sample value that stands for 1.0: 255, or 2^b - 1"""
    if not 8 <= bit_depth <= 16:
        raise ValueError("bit depth must be 8..16, got %r" % (bit_depth,))
    return (1 << bit_depth) - 1


def picture_samples(fmt, H, W):
    """samples of one picture: H W + 2 Hc Wc"""
    return _lib.check(_fn("dcvc_pix_picture_samples")(fmt, H, W))


def plane_shapes(fmt, H, W):
    """((H, W), (Hc, Wc)): the luma plane's and each chroma plane's shape"""
    if fmt not in FORMATS.values():
        raise ValueError("unknown pixel format %r" % (fmt,))
    return (H, W), (H // 2 if fmt in (DCVC_PIX_YUV420P, DCVC_PIX_NV12) else H, W if fmt == DCVC_PIX_YUV444P else W // 2)


def _sample_dtypes(bit_depth):
    import torch
    return (torch.uint8,) if bit_depth == 8 else _u16_dtypes()


def to_x(src, fmt, bit_depth, H, W, ldx=3, x=None, planar=False):
    """One picture (flat CUDA tensor of picture_samples(fmt, H, W) samples, file layout) as the model input [H, W, 3] fp16:
    x = fp16(fp16(v / max_val) - 0.5), nearest chroma. With ``x`` given, writes into it at pixel stride ``ldx`` (a flat fp16
    tensor view starting at the picture's first channel, e.g. a chunk slot). ``planar=True`` also returns the picture as
    LSB-aligned planar samples (Y, Cb, Cr back to back): (x, planar)."""
    import torch
    n = picture_samples(fmt, H, W)
    max_val(bit_depth)
    if src.dtype not in _sample_dtypes(bit_depth) or not src.is_cuda or not src.is_contiguous() or src.numel() != n:
        raise ValueError("to_x: a contiguous CUDA tensor of %d %s samples expected, got %d of %s"
                         % (n, "uint8" if bit_depth == 8 else "uint16 / int16", src.numel(), src.dtype))
    if x is None:
        if ldx != 3:
            raise ValueError("to_x: ldx != 3 needs an output tensor")
        x = torch.empty((H, W, 3), dtype=torch.float16, device=src.device)
    elif x.dtype != torch.float16 or not x.is_cuda or x.numel() < (H * W - 1) * ldx + 3:
        raise ValueError("to_x: x must be a CUDA float16 tensor of at least (H W - 1) ldx + 3 elements")
    pl = torch.empty(n, dtype=torch.uint8 if bit_depth == 8 else torch.int16, device=src.device) if planar else None
    _lib.check(_fn("dcvc_pix_to_x")(_vp(src.data_ptr()), fmt, bit_depth, H, W, _vp(x.data_ptr()), ldx,
                                    _vp(pl.data_ptr()) if planar else None, _stream(src)))
    if not planar:
        return x
    return x, pl if bit_depth == 8 else pl.view(u16_dtype())


def from_x(x_hat, H, W, fmt, bit_depth):
    """The distortion planes and the output samples of a decoded picture. x_hat: fp16 CUDA tensor [1, 3, Hp, Wp]
    (channels_last) or [Hp, Wp, 3], Hp >= H, Wp >= W. Returns (dist32, samples): flat tensors of picture_samples values, dist32
    fp32 and planar (Y, Cb, Cr), samples in file layout (uint8, or u16_dtype() above 8 bits)."""
    import torch
    if x_hat.dim() == 4:
        x_hat = x_hat[0].permute(1, 2, 0)
    if x_hat.dtype != torch.float16 or not x_hat.is_cuda or x_hat.dim() != 3 or x_hat.shape[2] != 3:
        raise ValueError("from_x: a float16 CUDA tensor [1, 3, Hp, Wp] or [Hp, Wp, 3] expected")
    x_hat = x_hat.contiguous()
    if x_hat.shape[0] < H or x_hat.shape[1] < W:
        raise ValueError("from_x: x_hat (%d x %d) is smaller than the picture (%d x %d)" % (x_hat.shape[1], x_hat.shape[0], W, H))
    n = picture_samples(fmt, H, W)
    max_val(bit_depth)
    dist = torch.empty(n, dtype=torch.float32, device=x_hat.device)
    samples = torch.empty(n, dtype=torch.uint8 if bit_depth == 8 else torch.int16, device=x_hat.device)
    _lib.check(_fn("dcvc_x_to_pix")(_vp(x_hat.data_ptr()), x_hat.shape[1], H, W, fmt, bit_depth, _vp(dist.data_ptr()),
                                    _vp(samples.data_ptr()), _stream(x_hat)))
    return dist, samples if bit_depth == 8 else samples.view(u16_dtype())


def split_planes(t, fmt, H, W):
    """a flat PLANAR picture (to_x's planar samples, from_x's dist32) -> (y [H, W], cbcr [2, Hc, Wc]) views"""
    (_, _), (hc, wc) = plane_shapes(fmt, H, W)
    return t[:H * W].view(H, W), t[H * W:].view(2, hc, wc)


def psnr(src_planar, dist32, fmt, bit_depth, H, W):
    """PSNR of one picture at peak = max_val: [(6 y + u + v) / 8, y, u, v]. src_planar: to_x's planar samples, dist32:
    from_x's planes. The weights are this project's convention for every format (the reference defines them for 4:2:0)."""
    peak = max_val(bit_depth)
    (sy, sc), (dy, dc) = split_planes(src_planar, fmt, H, W), split_planes(dist32, fmt, H, W)
    py = psnr_from_sse(sse(sy, dy)[0], sy.numel(), peak)
    pu, pv = (psnr_from_sse(s, sc.numel() // 2, peak) for s in sse(sc, dc))
    return [(6 * py + pu + pv) / 8, py, pu, pv]


def msssim_picture(src_planar, dist32, fmt, bit_depth, H, W):
    """MS-SSIM of one picture with data_range = max_val: [(6 y + u + v) / 8, y, u, v]; every plane's sides >= 88"""
    peak = max_val(bit_depth)
    (sy, sc), (dy, dc) = split_planes(src_planar, fmt, H, W), split_planes(dist32, fmt, H, W)
    my = float(msssim(sy, dy, peak)[0])
    mu, mv = (float(v) for v in msssim(sc, dc, peak))
    return [(6 * my + mu + mv) / 8, my, mu, mv]


def y4m_header(data):
    """the stream header at the start of a Y4M file's bytes -> dict(width, height, fps_num, fps_den, pix_fmt, bit_depth,
    header_bytes); raises DcvcError for what dcvc_y4m_parse_header refuses"""
    info = Y4mInfo()
    data = bytes(data[:1024])
    _lib.check(_fn("dcvc_y4m_parse_header")(data, len(data), ctypes.byref(info)))
    return {k: getattr(info, k) for k, _ in Y4mInfo._fields_}


def y4m_header_i(data):
    """y4m_header for material that may be field-interlaced (dcvc_y4m_parse_header_i): the same dict plus ``interlacing``,
    0 for Ip / I? / no I field, 1 for It (top field first), 2 for Ib (bottom field first); Im is refused"""
    info, fields = Y4mInfo(), _ci(0)
    data = bytes(data[:1024])
    _lib.check(_fn("dcvc_y4m_parse_header_i")(data, len(data), ctypes.byref(info), ctypes.byref(fields)))
    d = {k: getattr(info, k) for k, _ in Y4mInfo._fields_}
    d["interlacing"] = fields.value
    return d


def y4m_frame_header_bytes(data):
    """length of the "FRAME...\\n" line at the start of ``data``; raises DcvcError if there is none"""
    data = bytes(data[:1024])
    return _lib.check(_fn("dcvc_y4m_frame_header_bytes")(data, len(data)))


def y4m_write_header(width, height, pix_fmt, bit_depth, fps_num=25, fps_den=1):
    """the stream header line of a Y4M file as bytes"""
    info = Y4mInfo(width, height, fps_num, fps_den, pix_fmt, bit_depth, 0)
    buf = ctypes.create_string_buffer(256)
    n = _lib.check(_fn("dcvc_y4m_write_header")(buf, len(buf), ctypes.byref(info)))
    return buf.raw[:n]


__all__ = ["DCVC_PIX_YUV420P", "DCVC_PIX_YUV422P", "DCVC_PIX_YUV444P", "DCVC_PIX_NV12", "FORMATS", "picture_samples", "plane_shapes",
           "to_x", "from_x", "split_planes", "psnr", "msssim_picture", "max_val", "y4m_header", "y4m_header_i", "y4m_frame_header_bytes",
           "y4m_write_header"]
