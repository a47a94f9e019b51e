"""Inverse telecine (no reference counterpart): film at 23.976 Hz carried as 29.97 Hz interlaced video by 3:2
pulldown is put back together. ``field_match`` measures, on the GPU and in exact integers, how well the second field of a woven
luma plane fits the first field of the same frame (match c) or the previous frame's second field fits it (match p), and how
much the first field differs from the previous frame's (dup); ``weave_fields`` builds a frame from the rows of two plane sets;
``Ivtc`` restates the host decisions ``dcvc_ivtc_*`` (include/dcvc_amd_rc.h) operation for operation. tests/ivtc_np.py
restates the measurement in numpy.

``field_match`` and ``weave_fields`` are thin wrappers over ``dcvc_field_match`` and ``dcvc_weave_fields``
(include/dcvc_amd_ops.h, csrc/kernels/ivtc.hip) on ``torch.cuda.current_stream()``.

Sample tensors are ``torch.uint8`` (bit depth 8), or 16-bit as yuv16.py takes and returns them (bit depth 9..16).
"""
import ctypes

from . import _lib
from .yuv16 import DCVC_SAMPLE_U8, DCVC_SAMPLE_U16, _u16_dtypes, u16_dtype

MAX_CTHRESH = 255
MAX_MI = 512
MAX_SAMPLES = 16384 * 16384

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_fns = {}


def _fn(name, argtypes):
    if name not in _fns:
        _fns[name] = _lib.fn(name, _ci, argtypes)
    return _fns[name]


def _code(t, who):
    import torch
    if t.dtype == torch.uint8:
        return DCVC_SAMPLE_U8, torch.uint8
    if t.dtype in _u16_dtypes():
        return DCVC_SAMPLE_U16, u16_dtype()
    raise TypeError("%s: planes must be uint8 or uint16 / int16 (unsigned samples), got %s" % (who, t.dtype))


def field_match(cur, prev, first, cthresh, bit_depth, out=None):
    """cur: [H, W] CUDA luma samples of a woven frame, unit stride along a row (the row stride may be larger); prev: the luma
    plane of the previous frame, or None. first: the parity (0, 1) of the rows of the field shown first; cthresh: 0..255 in
    8-bit code values. Returns a CUDA int64 tensor [8]: match_c, match_p, comb_c, comb_p, blkmax_c, blkmax_p, dup, 0 - out, a
    contiguous one on cur's device, when given (what it holds does not matter)."""
    import torch
    if cur.dim() != 2 or not cur.is_cuda:
        raise ValueError("field_match: a CUDA plane [H, W] expected, got %s" % (tuple(cur.shape),))
    code, _ = _code(cur, "field_match")
    t = cur if cur.stride(1) == 1 else cur.contiguous()
    H, W = t.shape
    p = None
    if prev is not None:
        if tuple(prev.shape) != (H, W) or prev.device != t.device or prev.element_size() != t.element_size() or prev.dtype.is_floating_point:
            raise ValueError("field_match: prev must hold cur's plane: [%d, %d] samples of cur's width on cur's device" % (H, W))
        p = prev if prev.stride(1) == 1 else prev.contiguous()
    if out is None:
        out = torch.empty(8, dtype=torch.int64, device=t.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (8,) or out.device != t.device or not out.is_contiguous():
        raise ValueError("field_match: out must be a contiguous int64 tensor [8] on cur's device")
    _lib.check(_fn("dcvc_field_match", [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp])(
        _vp(t.data_ptr()), t.stride(0), _vp(p.data_ptr()) if p is not None else None, p.stride(0) if p is not None else 0, code,
        int(bit_depth), H, W, int(first), int(cthresh), _vp(out.data_ptr()), _vp(torch.cuda.current_stream(t.device).cuda_stream)))
    return out


def weave_fields(a, b, first, out=None):
    """a, b: [P, H, W] or [H, W] CUDA samples, unit stride along a row (row and plane strides may be larger). The rows of parity
    ``first`` (0, 1) of the result are a's, the others b's. out: a tensor of a's shape to write into (strided likewise), else a
    new contiguous one. Returns out."""
    import torch
    squeeze = a.dim() == 2
    ta = a[None] if squeeze else a
    if ta.dim() != 3 or not ta.is_cuda:
        raise ValueError("weave_fields: CUDA planes [P, H, W] or [H, W] expected, got %s" % (tuple(a.shape),))
    code, out_dtype = _code(ta, "weave_fields")
    if ta.stride(2) != 1:
        ta = ta.contiguous()
    P, H, W = ta.shape
    tb = b[None] if b.dim() == 2 else b
    if tuple(tb.shape) != (P, H, W) or tb.device != ta.device or tb.element_size() != ta.element_size() or tb.dtype.is_floating_point:
        raise ValueError("weave_fields: b must hold a's planes: [%d, %d, %d] samples of a's width on a's device" % (P, H, W))
    if tb.stride(2) != 1:
        tb = tb.contiguous()
    if out is None:
        o = torch.empty((P, H, W), dtype=out_dtype, device=ta.device)
    else:
        o = out[None] if out.dim() == 2 else out
        if (tuple(o.shape) != (P, H, W) or o.device != ta.device or o.stride(2) != 1 or o.element_size() != ta.element_size()
                or o.dtype.is_floating_point):
            raise ValueError("weave_fields: out must hold [%d, %d, %d] samples of a's width on a's device, rows at unit stride" % (P, H, W))
    _lib.check(_fn("dcvc_weave_fields", [_vp, _ci, _ll, _vp, _ci, _ll, _vp, _ci, _ll, _ci, _ci, _ci, _ci, _ci, _vp])(
        _vp(ta.data_ptr()), ta.stride(1), ta.stride(0), _vp(tb.data_ptr()), tb.stride(1), tb.stride(0), _vp(o.data_ptr()), o.stride(1),
        o.stride(0), code, H, W, P, int(first), _vp(torch.cuda.current_stream(ta.device).cuda_stream)))
    if out is not None:
        return out
    return o[0] if squeeze else o


class Ivtc:
    """dcvc_ivtc_* in Python. Source frames are pushed in order with the eight words of ``field_match`` against their
    predecessor. The match is p (1) when has_prev and match_p < match_c, strictly, else c (0); the frame is combed when the chosen
    match's blkmax > mi. The cycle grid is fixed from frame 0; once the ``cycle`` frames of a cycle are pushed ``drop()`` names
    the position with the smallest dup - ties to the lowest position, a frame without prev is never dropped."""

    def __init__(self, cycle, mi):
        cycle, mi = int(cycle), int(mi)
        if cycle != 0 and not 2 <= cycle <= 32:
            raise ValueError("the cycle must be 0 (no decimation) or in 2..32")
        if not 0 <= mi <= MAX_MI:
            raise ValueError("mi must be in 0..512")
        self.cycle, self.mi = cycle, mi
        self._next, self._drop, self._best, self._best_pos = 0, -1, 0, -1

    def push(self, idx, has_prev, m):
        """match | 2 * combed. A refused push (ValueError) changes nothing."""
        idx, has_prev = int(idx), bool(has_prev)
        m = [int(v) for v in m]
        if len(m) != 8:
            raise ValueError("eight words expected")
        if idx != self._next:
            raise ValueError("frame %d pushed, %d is next" % (idx, self._next))
        if idx == 0 and has_prev:
            raise ValueError("frame 0 has no previous frame")
        if m[2] > MAX_SAMPLES or m[3] > MAX_SAMPLES or min(m) < 0:
            raise ValueError("a comb count is above the samples of the largest plane")
        self._next = idx + 1
        match = 1 if has_prev and m[1] < m[0] else 0
        is_combed = 1 if m[4 + match] > self.mi else 0
        if self.cycle > 0:
            pos = idx % self.cycle
            if pos == 0:
                self._best_pos = -1
            if has_prev and (self._best_pos < 0 or m[6] < self._best):
                self._best, self._best_pos = m[6], pos
            self._drop = self._best_pos if pos == self.cycle - 1 else -1
        return match | 2 * is_combed

    def drop(self):
        """the position in the cycle just completed; -1 while the cycle is incomplete or when cycle == 0"""
        return self._drop


__all__ = ["field_match", "weave_fields", "Ivtc", "MAX_CTHRESH", "MAX_MI"]
