"""High-bit-depth YUV420 pictures (bit depth 9..16, e.g. yuv420p10le) on the GPU: DCVC-FM's YUVReader / YUVWriter
(video_reader.py:130-183, video_writer.py:86-130) and its PSNR / MS-SSIM at the data range of that scale (test_helper.py:100-126).

Thin wrappers over the C-ABI entry points ``dcvc_yuv420p16_to_x``, ``dcvc_x_to_yuv420p16``, ``dcvc_sse`` and
``dcvc_msssim_range`` (include/dcvc_amd_ops.h). Device operands are CUDA tensors; the kernels run on
``torch.cuda.current_stream()``.

Sample tensors: torch's ``uint16`` dtype has few ops. Inputs may be ``torch.uint16`` or ``torch.int16`` storage, which is
read as unsigned (the same 16 bits: a sample 40000 is the int16 -25536). Outputs are ``torch.uint16`` where torch has
the dtype and ``torch.int16`` storage of the unsigned samples where it does not (``.view(torch.int16)`` /
``.numpy().view(numpy.uint16)`` move between the two).
"""
import ctypes

import numpy as np

from . import _lib

DCVC_SAMPLE_U8 = 0
DCVC_SAMPLE_F16 = 1
DCVC_SAMPLE_U16 = 3
DCVC_SAMPLE_F32 = 4

_vp, _ci, _ll, _dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
_fns = {}
_SIGS = {
    "dcvc_yuv420p16_to_x": [_vp, _vp, _ci, _ci, _ci, _vp, _ci, _vp],
    "dcvc_x_to_yuv420p16": [_vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp],
    "dcvc_sse": [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ll, _vp, _vp],
    "dcvc_msssim_range": [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ll, _dbl, _vp, _vp],
}


def _fn(name):
    if name not in _fns:
        _fns[name] = _lib.fn(name, _ci, _SIGS[name])
    return _fns[name]


def _stream(t):
    import torch
    return _vp(torch.cuda.current_stream(t.device).cuda_stream)


def u16_dtype():
    """the dtype of the sample tensors this module returns: torch.uint16, or torch.int16 where torch lacks it"""
    import torch
    return getattr(torch, "uint16", torch.int16)


def _u16_dtypes():
    import torch
    return tuple(d for d in (getattr(torch, "uint16", None), torch.int16) if d is not None)


def max_val(bit_depth):
    """2^b - 1, the sample value that stands for 1.0"""
    if not 9 <= bit_depth <= 16:
        raise ValueError("bit depth must be 9..16, got %r" % (bit_depth,))
    return (1 << bit_depth) - 1


def yuv420p16_to_x(y, uv, bit_depth, ldx=3, x=None):
    """YUVReader's picture as the model input [H, W, 3] fp16 (x = fp16(fp16(v / max_val) - 0.5), nearest chroma).
    y: [H, W], uv: [2, H/2, W/2] contiguous CUDA uint16 / int16 tensors. With ``x`` given, writes into it at pixel stride
    ``ldx`` (a flat fp16 tensor view starting at the picture's first channel, e.g. a chunk slot) instead."""
    import torch
    for t in (y, uv):
        if t.dtype not in _u16_dtypes() or not t.is_cuda or not t.is_contiguous():
            raise ValueError("yuv420p16_to_x: contiguous uint16 / int16 CUDA planes expected, got %s" % t.dtype)
    if y.dim() != 2 or tuple(uv.shape) != (2, y.shape[0] // 2, y.shape[1] // 2):
        raise ValueError("yuv420p16_to_x: y [H, W] and uv [2, H/2, W/2] expected, got %s and %s"
                         % (tuple(y.shape), tuple(uv.shape)))
    H, W = y.shape
    if x is None:
        if ldx != 3:
            raise ValueError("yuv420p16_to_x: ldx != 3 needs an output tensor")
        x = torch.empty((H, W, 3), dtype=torch.float16, device=y.device)
    elif x.dtype != torch.float16 or not x.is_cuda or x.numel() < (H * W - 1) * ldx + 3:
        raise ValueError("yuv420p16_to_x: x must be a CUDA float16 tensor of at least (H W - 1) ldx + 3 elements")
    _lib.check(_fn("dcvc_yuv420p16_to_x")(_vp(y.data_ptr()), _vp(uv.data_ptr()), H, W, bit_depth, _vp(x.data_ptr()), ldx,
                                          _stream(y)))
    return x


def x_to_yuv420p16(x_hat, H, W, bit_depth):
    """The distortion planes and the writer's samples of a decoded picture. x_hat: fp16 CUDA tensor [1, 3, Hp, Wp]
    (channels_last) or [Hp, Wp, 3], Hp >= H, Wp >= W. Returns (dist_y [H, W] fp32, dist_uv [2, H/2, W/2] fp32,
    y16 [H, W], uv16 [2, H/2, W/2]) with the samples in u16_dtype()."""
    import torch
    if x_hat.dim() == 4:
        x_hat = x_hat[0].permute(1, 2, 0)
    if x_hat.dtype != torch.float16 or not x_hat.is_cuda or x_hat.dim() != 3 or x_hat.shape[2] != 3:
        raise ValueError("x_to_yuv420p16: a float16 CUDA tensor [1, 3, Hp, Wp] or [Hp, Wp, 3] expected")
    x_hat = x_hat.contiguous()
    if x_hat.shape[0] < H or x_hat.shape[1] < W:
        raise ValueError("x_to_yuv420p16: x_hat (%d x %d) is smaller than the picture (%d x %d)"
                         % (x_hat.shape[1], x_hat.shape[0], W, H))
    n = H * W + 2 * (H // 2) * (W // 2)
    dist = torch.empty(n, dtype=torch.float32, device=x_hat.device)
    samples = torch.empty(n, dtype=torch.int16, device=x_hat.device)
    _lib.check(_fn("dcvc_x_to_yuv420p16")(_vp(x_hat.data_ptr()), x_hat.shape[1], H, W, bit_depth, _vp(dist.data_ptr()),
                                          _vp(samples.data_ptr()), _stream(x_hat)))
    samples = samples.view(u16_dtype())

    def split(t):
        return t[:H * W].view(H, W), t[H * W:].view(2, H // 2, W // 2)

    return split(dist) + split(samples)


def _code(t):
    import torch
    if t.dtype == torch.uint8:
        return DCVC_SAMPLE_U8
    if t.dtype == torch.float16:
        return DCVC_SAMPLE_F16
    if t.dtype in _u16_dtypes():
        return DCVC_SAMPLE_U16
    if t.dtype == torch.float32:
        return DCVC_SAMPLE_F32
    raise TypeError("planes must be uint8, float16, uint16 / int16 (unsigned samples) or float32, got %s" % t.dtype)


def _planes(src, rec, what):
    if src.shape != rec.shape or src.dim() not in (2, 3):
        raise ValueError("%s: src and rec must share a [P, H, W] or [H, W] shape, got %s and %s"
                         % (what, tuple(src.shape), tuple(rec.shape)))
    if not (src.is_cuda and rec.is_cuda) or src.device != rec.device:
        raise ValueError("%s: src and rec must be CUDA tensors on one device" % what)
    codes = _code(src), _code(rec)
    if src.dim() == 2:
        src, rec = src[None], rec[None]
    if src.stride(2) != 1 or src.stride() != rec.stride():
        src, rec = src.contiguous(), rec.contiguous()
    return src, rec, codes


def sse(src, rec):
    """fp64 sum of squared differences of every plane pair: src / rec CUDA tensors [P, H, W] or [H, W] of any sample type
    (uint8, float16, uint16 / int16 read as unsigned, float32; the two may differ). Returns a float64 numpy array of P values."""
    import torch
    src, rec, codes = _planes(src, rec, "sse")
    P, H, W = src.shape
    out = torch.empty(P, dtype=torch.float64, device=src.device)
    _lib.check(_fn("dcvc_sse")(_vp(src.data_ptr()), codes[0], _vp(rec.data_ptr()), codes[1], P, H, W, src.stride(1),
                               src.stride(0), _vp(out.data_ptr()), _stream(src)))
    return out.cpu().numpy()


def msssim(src, rec, data_range):
    """calc_msssim(src, rec, data_range) of every plane pair (shapes and sample types as sse). Returns float64 numpy values."""
    import torch
    src, rec, codes = _planes(src, rec, "msssim")
    P, H, W = src.shape
    out = torch.empty(P, dtype=torch.float64, device=src.device)
    _lib.check(_fn("dcvc_msssim_range")(_vp(src.data_ptr()), codes[0], _vp(rec.data_ptr()), codes[1], P, H, W, src.stride(1),
                                        src.stride(0), float(data_range), _vp(out.data_ptr()), _stream(src)))
    return out.cpu().numpy()


def psnr_from_sse(total, n, peak):
    """metrics.py:10-24 calc_psnr at the data range `peak` from the fp64 sum of squares over n samples"""
    mse = total / n
    if np.isnan(mse) or np.isinf(mse):
        return -999.9
    p = 10 * np.log10(float(peak) * float(peak) / mse) if mse > 1e-10 else 999.9
    return float(min(p, 99.9))


def psnr_yuv420p16(y, uv, dist_y, dist_uv, bit_depth):
    """get_distortion's PSNR of one picture in sample units: [(6 y + u + v) / 8, y, u, v]. y / uv: the source samples,
    dist_y / dist_uv: x_to_yuv420p16's fp32 planes."""
    peak = max_val(bit_depth)
    sy = sse(y, dist_y)[0]
    su, sv = sse(uv, dist_uv)
    py = psnr_from_sse(sy, y.numel(), peak)
    pu, pv = (psnr_from_sse(s, uv.numel() // 2, peak) for s in (su, sv))
    return [(6 * py + pu + pv) / 8, py, pu, pv]


def msssim_yuv420p16(y, uv, dist_y, dist_uv, bit_depth):
    """get_distortion's MS-SSIM of one picture with data_range = max_val: [(6 y + u + v) / 8, y, u, v]"""
    peak = max_val(bit_depth)
    sy = float(msssim(y, dist_y, peak)[0])
    su, sv = (float(v) for v in msssim(uv, dist_uv, peak))
    return [(6 * sy + su + sv) / 8, sy, su, sv]


__all__ = ["yuv420p16_to_x", "x_to_yuv420p16", "sse", "msssim", "psnr_from_sse", "psnr_yuv420p16", "msssim_yuv420p16",
           "max_val", "u16_dtype", "DCVC_SAMPLE_U8", "DCVC_SAMPLE_F16", "DCVC_SAMPLE_U16", "DCVC_SAMPLE_F32"]
