"""A motion-adaptive, edge-directed deinterlacer over planes of integer samples on the GPU (no reference
counterpart): the rows of one parity of a woven frame are kept, the others made from a three-direction spatial interpolation
blended with the woven sample by a motion measure against the previous input frame, every output sample defined exactly
(tests/deinterlace_np.py restates it in numpy).

``deinterlace_planes`` is a thin wrapper over ``dcvc_deinterlace_planes`` (include/dcvc_amd_ops.h,
csrc/kernels/deinterlace.hip): one launch on ``torch.cuda.current_stream()``.

Sample tensors are ``torch.uint8`` (bit depth 8), or 16-bit as yuv16.py takes and returns them (bit depth 9..16):
``torch.uint16`` or ``torch.int16`` storage read as unsigned in, ``yuv16.u16_dtype()`` out.
"""
import ctypes

from . import _lib
from .yuv16 import DCVC_SAMPLE_U8, DCVC_SAMPLE_U16, _u16_dtypes, u16_dtype

MAX_THRESHOLD = 64

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_SIG = [_vp, _ci, _ll, _vp, _ci, _ll, _vp, _ci, _ll, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp]
_fns = {}


def _fn():
    if "f" not in _fns:
        _fns["f"] = _lib.fn("dcvc_deinterlace_planes", _ci, _SIG)
    return _fns["f"]


def deinterlace_planes(cur, prev, keep, weave_from_prev, threshold, bit_depth, out=None):
    """cur: [P, H, W] or [H, W] CUDA samples of a woven frame, unit stride along a row (row and plane strides may be larger);
    prev: the same planes of the previous input frame, or None (spatial only). keep: the parity (0, 1) of the rows that are
    copied; weave_from_prev: 1 takes the woven sample of a missing row from prev, 0 from cur; threshold: 0..64 in 8-bit code
    values. out: a tensor of cur's shape to write into (strided likewise), else a new contiguous one. Returns out."""
    import torch
    squeeze = cur.dim() == 2
    t = cur[None] if squeeze else cur
    if t.dim() != 3 or not t.is_cuda:
        raise ValueError("deinterlace: CUDA planes [P, H, W] or [H, W] expected, got %s" % (tuple(cur.shape),))
    if t.dtype == torch.uint8:
        code, out_dtype = DCVC_SAMPLE_U8, torch.uint8
    elif t.dtype in _u16_dtypes():
        code, out_dtype = DCVC_SAMPLE_U16, u16_dtype()
    else:
        raise TypeError("deinterlace: planes must be uint8 or uint16 / int16 (unsigned samples), got %s" % t.dtype)
    if t.stride(2) != 1:
        t = t.contiguous()
    P, H, W = t.shape
    p = None
    if prev is not None:
        p = prev[None] if prev.dim() == 2 else prev
        if tuple(p.shape) != (P, H, W) or p.device != t.device or p.element_size() != t.element_size() or p.dtype.is_floating_point:
            raise ValueError("deinterlace: prev must hold cur's planes: [%d, %d, %d] samples of cur's width on cur's device" % (P, H, W))
        if p.stride(2) != 1:
            p = p.contiguous()
    if out is None:
        o = torch.empty((P, H, W), dtype=out_dtype, device=t.device)
    else:
        o = out[None] if out.dim() == 2 else out
        if (tuple(o.shape) != (P, H, W) or o.device != t.device or o.stride(2) != 1 or o.element_size() != t.element_size()
                or o.dtype.is_floating_point):
            raise ValueError("deinterlace: out must hold [%d, %d, %d] samples of cur's width on cur's device, rows at unit stride" % (P, H, W))
    _lib.check(_fn()(
        _vp(t.data_ptr()), t.stride(1), t.stride(0),
        _vp(p.data_ptr()) if p is not None else None, p.stride(1) if p is not None else 0, p.stride(0) if p is not None else 0,
        _vp(o.data_ptr()), o.stride(1), o.stride(0), code, int(bit_depth), H, W, P, int(keep), int(weave_from_prev), int(threshold),
        _vp(torch.cuda.current_stream(t.device).cuda_stream)))
    if out is not None:
        return out
    return o[0] if squeeze else o


__all__ = ["deinterlace_planes", "MAX_THRESHOLD"]
