"""MS-SSIM on the GPU (src/utils/metrics.py:27-91 calc_msssim, :86-91 calc_msssim_rgb; test_video.py:45-51 get_distortion).

Thin wrappers over the C-ABI entry point ``dcvc_msssim`` (include/dcvc_amd_ops.h): planes are CUDA tensors of uint8 or
float16 samples in 0..255, the metric runs in fp64 on ``torch.cuda.current_stream()`` and the values come back as float64.
"""
import ctypes

from . import _lib

DCVC_SAMPLE_U8 = 0
DCVC_SAMPLE_F16 = 1

_vp, _ci = ctypes.c_void_p, ctypes.c_int
_fn = None


def _entry():
    global _fn
    if _fn is None:
        _fn = _lib.fn("dcvc_msssim", _ci, [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, ctypes.c_longlong, _vp, _vp])
    return _fn


def _dtype_code(t):
    import torch
    if t.dtype == torch.uint8:
        return DCVC_SAMPLE_U8
    if t.dtype == torch.float16:
        return DCVC_SAMPLE_F16
    raise TypeError("msssim: planes must be uint8 or float16, got %s" % t.dtype)


def msssim(src, rec):
    """calc_msssim of every plane pair: src / rec CUDA tensors [P, H, W] or [H, W] (uint8 or float16, values 0..255, the two
    dtypes may differ). Returns a float64 numpy array of P values (NaN where a cs mean is negative, as in the reference)."""
    import torch
    if src.shape != rec.shape or src.dim() not in (2, 3):
        raise ValueError("msssim: src and rec must share a [P, H, W] or [H, W] shape, got %s and %s"
                         % (tuple(src.shape), tuple(rec.shape)))
    if not (src.is_cuda and rec.is_cuda) or src.device != rec.device:
        raise ValueError("msssim: src and rec must be CUDA tensors on one device")
    codes = _dtype_code(src), _dtype_code(rec)
    if src.dim() == 2:
        src, rec = src[None], rec[None]
    # one geometry for both planes: unit sample stride, shared row and plane strides
    if src.stride(2) != 1 or src.stride() != rec.stride():
        src, rec = src.contiguous(), rec.contiguous()
    P, H, W = src.shape
    out = torch.empty(P, dtype=torch.float64, device=src.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
    _lib.check(_entry()(_vp(src.data_ptr()), codes[0], _vp(rec.data_ptr()), codes[1], P, H, W, src.stride(1), src.stride(0),
                        _vp(out.data_ptr()), stream))
    return out.cpu().numpy()


def msssim_yuv420(y, uv, y_rec, uv_rec):
    """get_distortion's MS-SSIM of one YUV420 picture (y [H, W], uv [2, H/2, W/2]): [(6 y + u + v) / 8, y, u, v]"""
    sy = float(msssim(y, y_rec)[0])
    su, sv = (float(v) for v in msssim(uv, uv_rec))
    return [(6 * sy + su + sv) / 8, sy, su, sv]


def msssim_rgb(rgb, rgb_rec):
    """calc_msssim_rgb: the mean of the three planes' MS-SSIM of 3 x H x W tensors"""
    if rgb.dim() != 3 or rgb.shape[0] != 3:
        raise ValueError("msssim_rgb: 3 x H x W planes expected, got %s" % (tuple(rgb.shape),))
    v = msssim(rgb, rgb_rec)
    return float(((0.0 + v[0]) + v[1] + v[2]) / 3)


__all__ = ["msssim", "msssim_yuv420", "msssim_rgb", "DCVC_SAMPLE_U8", "DCVC_SAMPLE_F16"]
