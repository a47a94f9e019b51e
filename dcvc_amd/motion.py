"""Block motion search between two luma planes and motion compensation of planes through its vectors on the GPU (DESIGN.md 31;
no reference counterpart): a two-level search, one integer vector per 16 x 16 block, every value defined exactly
(tests/motion_np.py restates both in numpy).

``motion_search`` and ``motion_compensate_planes`` are thin wrappers over ``dcvc_motion_search`` and
``dcvc_motion_compensate_planes`` (include/dcvc_amd_ops.h, csrc/kernels/motion.hip): two launches and one launch on
``torch.cuda.current_stream()``.

Sample tensors are ``torch.uint8`` (bit depth 8), or 16-bit as yuv16.py takes and returns them (bit depth 9..16):
``torch.uint16`` or ``torch.int16`` storage read as unsigned in, ``yuv16.u16_dtype()`` out.
"""
import ctypes

from . import _lib
from .yuv16 import DCVC_SAMPLE_U8, DCVC_SAMPLE_U16, _u16_dtypes, u16_dtype

BLOCK = 16
MAX_RANGE = 15
MAX_LAMBDA = 255

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_fns = {}


def _fn(name):
    if not _fns:
        _fns["dcvc_motion_search_workspace_bytes"] = _lib.fn("dcvc_motion_search_workspace_bytes", _ll, [_ci, _ci])
        _fns["dcvc_motion_search"] = _lib.fn("dcvc_motion_search", _ci,
                                             [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _vp, _vp, _vp, _ll, _vp])
        _fns["dcvc_motion_compensate_planes"] = _lib.fn("dcvc_motion_compensate_planes", _ci,
                                                        [_vp, _ci, _ll, _vp, _ci, _ll, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _vp])
    return _fns[name]


def _code(t, who):
    import torch
    if t.dtype == torch.uint8:
        return DCVC_SAMPLE_U8, torch.uint8
    if t.dtype in _u16_dtypes():
        return DCVC_SAMPLE_U16, u16_dtype()
    raise TypeError("%s: planes must be uint8 or uint16 / int16 (unsigned samples), got %s" % (who, t.dtype))


def grid(H, W):
    """the block grid (Bh, Bw) of a luma plane [H, W]"""
    return (H + BLOCK - 1) // BLOCK, (W + BLOCK - 1) // BLOCK


def motion_search(cur, ref, bit_depth, search_range=7, lam=4, out=None):
    """cur, ref: [H, W] CUDA luma samples, unit stride along a row (row strides may be larger). search_range: 0..15 in
    half-resolution samples; lam: 0..255, the penalty a sample of vector length in 8-bit code values. out: a contiguous int16
    [Bh, Bw, 2] tensor to take the vectors, else a new one. Returns (mv int16 [Bh, Bw, 2] holding (dx, dy), sad int32 [Bh, Bw]:
    the winners' SADs without the penalty, below 2^31)."""
    import torch
    if cur.dim() != 2 or not cur.is_cuda or tuple(ref.shape) != tuple(cur.shape) or ref.device != cur.device:
        raise ValueError("motion_search: two CUDA planes [H, W] of one size on one device expected")
    code, _ = _code(cur, "motion_search")
    if ref.element_size() != cur.element_size() or ref.dtype.is_floating_point:
        raise ValueError("motion_search: ref must hold samples of cur's width")
    c = cur if cur.stride(1) == 1 else cur.contiguous()
    r = ref if ref.stride(1) == 1 else ref.contiguous()
    H, W = c.shape
    Bh, Bw = grid(H, W)
    if out is None:
        mv = torch.empty((Bh, Bw, 2), dtype=torch.int16, device=c.device)
    else:
        mv = out
        if tuple(mv.shape) != (Bh, Bw, 2) or mv.dtype != torch.int16 or mv.device != c.device or not mv.is_contiguous():
            raise ValueError("motion_search: out must be a contiguous int16 [%d, %d, 2] tensor on cur's device" % (Bh, Bw))
    sad = torch.empty((Bh, Bw), dtype=torch.int32, device=c.device)
    need = _fn("dcvc_motion_search_workspace_bytes")(H, W)
    ws = torch.empty((max(int(need), 2),), dtype=torch.uint8, device=c.device)
    _lib.check(_fn("dcvc_motion_search")(
        _vp(c.data_ptr()), c.stride(0), _vp(r.data_ptr()), r.stride(0), code, int(bit_depth), H, W, int(search_range), int(lam),
        _vp(mv.data_ptr()), Bh, Bw, _vp(sad.data_ptr()), None, _vp(ws.data_ptr()), ws.numel(),
        _vp(torch.cuda.current_stream(c.device).cuda_stream)))
    return mv, sad      # ws was allocated on the stream that uses it: the allocator reuses it in stream order


def motion_compensate_planes(prev, mv, sx, sy, out=None):
    """prev: [P, H, W] or [H, W] CUDA samples, unit stride along a row (row and plane strides may be larger), subsampled by
    (sx, sy) in {0, 1} against the luma plane mv was searched on; mv: a contiguous int16 [Bh, Bw, 2] tensor holding (dx, dy).
    out: a tensor of prev's shape to write into (strided likewise), else a new contiguous one. Returns out."""
    import torch
    squeeze = prev.dim() == 2
    t = prev[None] if squeeze else prev
    if t.dim() != 3 or not t.is_cuda:
        raise ValueError("motion_compensate: CUDA planes [P, H, W] or [H, W] expected, got %s" % (tuple(prev.shape),))
    code, out_dtype = _code(t, "motion_compensate")
    if t.stride(2) != 1:
        t = t.contiguous()
    if mv.dim() != 3 or mv.shape[2] != 2 or mv.dtype != torch.int16 or mv.device != t.device or not mv.is_contiguous():
        raise ValueError("motion_compensate: mv must be a contiguous int16 [Bh, Bw, 2] tensor on prev's device")
    P, H, W = t.shape
    if out is None:
        o = torch.empty((P, H, W), dtype=out_dtype, device=t.device)
    else:
        o = out[None] if out.dim() == 2 else out
        if (tuple(o.shape) != (P, H, W) or o.device != t.device or o.stride(2) != 1 or o.element_size() != t.element_size()
                or o.dtype.is_floating_point):
            raise ValueError("motion_compensate: out must hold [%d, %d, %d] samples of prev's width on prev's device, rows at unit stride"
                             % (P, H, W))
    _lib.check(_fn("dcvc_motion_compensate_planes")(
        _vp(t.data_ptr()), t.stride(1), t.stride(0), _vp(o.data_ptr()), o.stride(1), o.stride(0), code, H, W, P, int(sx), int(sy),
        _vp(mv.data_ptr()), mv.shape[0], mv.shape[1], _vp(torch.cuda.current_stream(t.device).cuda_stream)))
    if out is not None:
        return out
    return o[0] if squeeze else o


__all__ = ["motion_search", "motion_compensate_planes", "grid", "BLOCK", "MAX_RANGE", "MAX_LAMBDA"]
