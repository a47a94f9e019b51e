"""Frame-rate conversion on the GPU (no reference counterpart): the picture at k / n of the way from picture a to
picture b through the vectors of ``motion.motion_search(b, a)``, every value defined exactly (tests/interp_np.py restates it in
numpy).

``interp_select`` and ``interp_planes`` are thin wrappers over ``dcvc_interp_select`` and ``dcvc_interp_planes``
(include/dcvc_amd_ops.h, csrc/kernels/interp.hip): one launch each on ``torch.cuda.current_stream()``. ``interpolate`` runs the
search once and the two kernels per phase.

Sample tensors are ``torch.uint8`` (bit depth 8), or 16-bit as yuv16.py takes and returns them (bit depth 9..16).
"""
import ctypes

from . import _lib
from .motion import BLOCK, _code, grid, motion_search

MIN_N, MAX_N = 2, 8
MAX_LIMIT = 255

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_fns = {}


def _fn(name):
    if not _fns:
        _fns["dcvc_interp_select"] = _lib.fn("dcvc_interp_select", _ci, [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci,
                                                                         _vp, _vp, _ci, _ci, _vp, _vp, _vp])
        _fns["dcvc_interp_planes"] = _lib.fn("dcvc_interp_planes", _ci, [_vp, _ci, _ll, _vp, _ci, _ll, _vp, _ci, _ll, _ci, _ci, _ci, _ci, _ci,
                                                                         _ci, _vp, _vp, _ci, _ci, _ci, _ci, _vp, _ci, _vp])
    return _fns[name]


def _rows(t):
    return t if t.stride(-1) == 1 else t.contiguous()


def interp_select(a, b, mv, bit_depth, k, n, limit=8, fallen=None, with_sad=True):
    """a, b: [H, W] CUDA luma samples of the earlier and the later picture, unit stride along a row; mv: a contiguous int16
    [>= Bh, >= Bw, 2] tensor, the vectors of motion_search(b, a). limit: 0..255 in 8-bit code values a sample. fallen: an int32
    tensor of one element that the call adds the number of fallen blocks to (the caller zeroes it), else none is counted.
    Returns (plan int16 [Bh, Bw, 4], wb uint8 [Bh, Bw], sad int32 [Bh, Bw] or None)."""
    import torch
    if a.dim() != 2 or not a.is_cuda or tuple(b.shape) != tuple(a.shape) or b.device != a.device:
        raise ValueError("interp_select: two CUDA planes [H, W] of one size on one device expected")
    code, _ = _code(a, "interp_select")
    if b.element_size() != a.element_size() or b.dtype.is_floating_point:
        raise ValueError("interp_select: b must hold samples of a's width")
    if mv.dim() != 3 or mv.shape[2] != 2 or mv.dtype != torch.int16 or mv.device != a.device or not mv.is_contiguous():
        raise ValueError("interp_select: mv must be a contiguous int16 [Bh, Bw, 2] tensor on a's device")
    if fallen is not None and (fallen.numel() != 1 or fallen.dtype != torch.int32 or fallen.device != a.device):
        raise ValueError("interp_select: fallen must be an int32 tensor of one element on a's device")
    ta, tb = _rows(a), _rows(b)
    H, W = ta.shape
    Bh, Bw = grid(H, W)
    plan = torch.empty((Bh, Bw, 4), dtype=torch.int16, device=a.device)
    wb = torch.empty((Bh, Bw), dtype=torch.uint8, device=a.device)
    sad = torch.empty((Bh, Bw), dtype=torch.int32, device=a.device) if with_sad else None
    _lib.check(_fn("dcvc_interp_select")(
        _vp(ta.data_ptr()), ta.stride(0), _vp(tb.data_ptr()), tb.stride(0), code, int(bit_depth), H, W, _vp(mv.data_ptr()), mv.shape[0],
        mv.shape[1], int(k), int(n), int(limit), _vp(plan.data_ptr()), _vp(wb.data_ptr()), Bh, Bw,
        _vp(sad.data_ptr()) if with_sad else None, _vp(fallen.data_ptr()) if fallen is not None else None,
        _vp(torch.cuda.current_stream(a.device).cuda_stream)))
    return plan, wb, sad


def interp_planes(a, b, plan, wb, k, n, sx, sy, fallen=None, out=None, n_blocks=None):
    """a, b: [P, H, W] or [H, W] CUDA samples, unit stride along a row (row and plane strides may be larger), subsampled by
    (sx, sy) in {0, 1} against the luma plane of the selection; plan: a contiguous int16 [bh, bw, 4] tensor, wb: a contiguous
    uint8 [bh, bw] tensor. fallen: the int32 counter of the selection: with it the picture rule holds, 2 * fallen > n_blocks
    repeats the whole picture (n_blocks: the blocks of the selection, plan's bh * bw by default). out: a tensor of a's shape to
    write into (strided likewise), else a new contiguous one. Returns out."""
    import torch
    squeeze = a.dim() == 2
    ta, tb = (a[None], b[None]) if squeeze else (a, b)
    if ta.dim() != 3 or not ta.is_cuda or tuple(tb.shape) != tuple(ta.shape) or tb.device != ta.device:
        raise ValueError("interp_planes: CUDA planes [P, H, W] or [H, W] of one shape on one device expected")
    code, out_dtype = _code(ta, "interp_planes")
    if tb.element_size() != ta.element_size() or tb.dtype.is_floating_point:
        raise ValueError("interp_planes: b must hold samples of a's width")
    ta, tb = _rows(ta), _rows(tb)
    if plan.dim() != 3 or plan.shape[2] != 4 or plan.dtype != torch.int16 or plan.device != ta.device or not plan.is_contiguous():
        raise ValueError("interp_planes: plan must be a contiguous int16 [bh, bw, 4] tensor on a's device")
    if tuple(wb.shape) != tuple(plan.shape[:2]) or wb.dtype != torch.uint8 or wb.device != ta.device or not wb.is_contiguous():
        raise ValueError("interp_planes: wb must be a contiguous uint8 tensor of plan's grid on a's device")
    if fallen is not None and (fallen.numel() != 1 or fallen.dtype != torch.int32 or fallen.device != ta.device):
        raise ValueError("interp_planes: fallen must be an int32 tensor of one element on a's device")
    P, H, W = ta.shape
    if out is None:
        o = torch.empty((P, H, W), dtype=out_dtype, device=ta.device)
    else:
        o = out[None] if out.dim() == 2 else out
        if (tuple(o.shape) != (P, H, W) or o.device != ta.device or o.stride(2) != 1 or o.element_size() != ta.element_size()
                or o.dtype.is_floating_point):
            raise ValueError("interp_planes: out must hold [%d, %d, %d] samples of a's width on a's device, rows at unit stride" % (P, H, W))
    if n_blocks is None:
        n_blocks = plan.shape[0] * plan.shape[1]
    _lib.check(_fn("dcvc_interp_planes")(
        _vp(ta.data_ptr()), ta.stride(1), ta.stride(0), _vp(tb.data_ptr()), tb.stride(1), tb.stride(0), _vp(o.data_ptr()), o.stride(1),
        o.stride(0), code, H, W, P, int(sx), int(sy), _vp(plan.data_ptr()), _vp(wb.data_ptr()), plan.shape[0], plan.shape[1], int(k), int(n),
        _vp(fallen.data_ptr()) if fallen is not None else None, int(n_blocks) if fallen is not None else 0,
        _vp(torch.cuda.current_stream(ta.device).cuda_stream)))
    if out is not None:
        return out
    return o[0] if squeeze else o


def interpolate(a_planes, b_planes, bit_depth, n, search_range=7, lam=4, limit=8):
    """a_planes, b_planes: the pictures (y, u, v) as CUDA tensors [H, W]; u and v share one size, subsampled by 0 or 1 on either
    axis against y. Returns the n - 1 in-between pictures (y, u, v), k = 1..n-1: one search of b's luma against a's, then per
    phase the selection, luma in one interpolation call and both chroma planes in another, with the picture rule."""
    import torch
    ya, ua, va = a_planes
    yb, ub, vb = b_planes
    H, W = ya.shape
    ch, cw = ua.shape
    subs = [(sx, sy) for sx in (0, 1) for sy in (0, 1) if (W + sx) >> sx == cw and (H + sy) >> sy == ch]
    if not subs or tuple(va.shape) != (ch, cw):
        raise ValueError("interpolate: chroma planes of %dx%d do not belong to a luma plane of %dx%d" % (cw, ch, W, H))
    sx, sy = subs[0]
    mv, _ = motion_search(yb, ya, bit_depth, search_range, lam)
    ca, cb = torch.stack([ua, va]), torch.stack([ub, vb])
    out = []
    for k in range(1, n):
        fallen = torch.zeros(1, dtype=torch.int32, device=ya.device)
        plan, wb, _ = interp_select(ya, yb, mv, bit_depth, k, n, limit, fallen=fallen, with_sad=False)
        y = interp_planes(ya, yb, plan, wb, k, n, 0, 0, fallen=fallen)
        c = interp_planes(ca, cb, plan, wb, k, n, sx, sy, fallen=fallen)
        out.append((y, c[0], c[1]))
    return out


__all__ = ["interp_select", "interp_planes", "interpolate", "grid", "BLOCK", "MIN_N", "MAX_N", "MAX_LIMIT"]
