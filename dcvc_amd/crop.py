"""Black-bar cropping (no reference counterpart): letterboxed and pillarboxed sources are coded without their
bars. ``crop_stats`` counts, on the GPU and in exact integers, the samples above a limit in every row and every column of a luma
plane; ``window_planes`` copies a window of a plane set into planes of another size - a crop, a pad or any mixture - filling
what the window shows beyond the source; ``CropDetect`` restates the host decision ``dcvc_cropdet_*`` (include/dcvc_amd_rc.h)
operation for operation. tests/crop_np.py restates all three in numpy.

``crop_stats`` and ``window_planes`` are thin wrappers over ``dcvc_crop_stats`` and ``dcvc_window_planes``
(include/dcvc_amd_ops.h, csrc/kernels/crop.hip) on ``torch.cuda.current_stream()``.

Sample tensors are ``torch.uint8`` (bit depth 8), or 16-bit as yuv16.py takes and returns them (bit depth 9..16).
"""
import ctypes

from . import _lib
from .yuv16 import DCVC_SAMPLE_U8, DCVC_SAMPLE_U16, _u16_dtypes, u16_dtype

MAX_LIMIT = 255
MAX_FRAC = 255
MAX_MIN_BAR = 4096
MAX_SIDE = 16384

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


def crop_stats(luma, limit, bit_depth, out=None):
    """luma: [H, W] CUDA luma samples, unit stride along a row (the row stride may be larger). limit: 0..255 in 8-bit code
    values. Returns a CUDA int32 tensor [H + W]: per row, then per column, the number of samples above
    limit << (bit_depth - 8) - out, a contiguous int32 or int64 one on luma's device, when given (what it holds does not
    matter; an int64 out is filled from an int32 result)."""
    import torch
    if luma.dim() != 2 or not luma.is_cuda:
        raise ValueError("crop_stats: a CUDA plane [H, W] expected, got %s" % (tuple(luma.shape),))
    code, _ = _code(luma, "crop_stats")
    t = luma if luma.stride(1) == 1 else luma.contiguous()
    H, W = t.shape
    if out is not None and (out.dtype not in (torch.int32, torch.int64) or tuple(out.shape) != (H + W,) or out.device != t.device
                            or not out.is_contiguous()):
        raise ValueError("crop_stats: out must be a contiguous int32 or int64 tensor [%d] on luma's device" % (H + W))
    words = out if out is not None and out.dtype == torch.int32 else torch.empty(H + W, dtype=torch.int32, device=t.device)
    _lib.check(_fn("dcvc_crop_stats", [_vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp])(
        _vp(t.data_ptr()), t.stride(0), code, int(bit_depth), H, W, int(limit), _vp(words.data_ptr()),
        _vp(torch.cuda.current_stream(t.device).cuda_stream)))
    if out is None:
        return words
    if out is not words:
        out.copy_(words)
    return out


def window_planes(src, out_h, out_w, ox, oy, fill, out=None):
    """src: [P, Hs, Ws] or [Hs, Ws] CUDA samples, unit stride along a row (row and plane strides may be larger). The result's
    planes are [out_h, out_w]: out[p][y][x] = src[p][y + oy][x + ox] inside the source, fill[p] outside; ox, oy are signed. fill:
    one value for every plane, or one per plane. out: a tensor of the result's shape to write into (rows at unit stride), else
    a new contiguous one. Returns out."""
    import torch
    squeeze = src.dim() == 2
    ts = src[None] if squeeze else src
    if ts.dim() != 3 or not ts.is_cuda:
        raise ValueError("window_planes: CUDA planes [P, H, W] or [H, W] expected, got %s" % (tuple(src.shape),))
    code, out_dtype = _code(ts, "window_planes")
    if ts.stride(2) != 1:
        ts = ts.contiguous()
    P, Hs, Ws = ts.shape
    out_h, out_w = int(out_h), int(out_w)
    fills = [int(fill)] * P if isinstance(fill, int) else [int(v) for v in fill]
    if len(fills) != P:
        raise ValueError("window_planes: %d fill values for %d planes" % (len(fills), P))
    if out is None:
        if not (1 <= out_h <= MAX_SIDE and 1 <= out_w <= MAX_SIDE):
            raise ValueError("window_planes: the window must be in 1..%d a side, got %dx%d" % (MAX_SIDE, out_w, out_h))
        o = torch.empty((P, out_h, out_w), dtype=out_dtype, device=ts.device)
    else:
        o = out[None] if out.dim() == 2 else out
        if (tuple(o.shape) != (P, out_h, out_w) or o.device != ts.device or o.stride(2) != 1 or o.element_size() != ts.element_size()
                or o.dtype.is_floating_point):
            raise ValueError("window_planes: out must hold [%d, %d, %d] samples of src's width on src's device, rows at unit stride"
                             % (P, out_h, out_w))
    _lib.check(_fn("dcvc_window_planes", [_vp, _ci, _ll, _ci, _ci, _vp, _ci, _ll, _ci, _ci, _ci, _ci, _ci, _ci, ctypes.POINTER(_ci), _vp])(
        _vp(ts.data_ptr()), ts.stride(1), ts.stride(0), Hs, Ws, _vp(o.data_ptr()), o.stride(1), o.stride(0), out_h, out_w, code, P,
        int(ox), int(oy), (_ci * P)(*fills), _vp(torch.cuda.current_stream(ts.device).cuda_stream)))
    if out is not None:
        return out
    return o[0] if squeeze else o


class CropDetect:
    """dcvc_cropdet_* in Python. Pictures are pushed with the H + W words of ``crop_stats``. Row r is active iff
    rowcnt[r] * 256 > W * frac, column c iff colcnt[c] * 256 > H * frac; a picture without an active row or column casts no
    vote; the result is the union of the voting pictures' rectangles, its bars below min_bar dropped and the others rounded
    down to multiples of ay (top, bottom) and ax (left, right)."""

    def __init__(self, H, W, frac, min_bar, ax, ay):
        H, W, frac, min_bar, ax, ay = int(H), int(W), int(frac), int(min_bar), int(ax), int(ay)
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError("H and W must be in 1..16384")
        if not 0 <= frac <= MAX_FRAC:
            raise ValueError("frac must be in 0..255")
        if not 0 <= min_bar <= MAX_MIN_BAR:
            raise ValueError("min_bar must be in 0..4096")
        if ax not in (1, 2, 4) or ay not in (1, 2, 4):
            raise ValueError("ax and ay must be 1, 2 or 4")
        if H % ay or W % ax:
            raise ValueError("H must be a multiple of ay and W of ax")
        self.H, self.W, self.frac, self.min_bar, self.ax, self.ay = H, W, frac, min_bar, ax, ay
        self.votes = 0
        self._rect = None          # top, bottom, left, right of the union

    def push(self, counts):
        """True: the picture voted. A refused push (ValueError) changes nothing."""
        m = [int(v) for v in counts]
        H, W = self.H, self.W
        if len(m) != H + W:
            raise ValueError("%d words expected" % (H + W))
        if any(v < 0 or v > W for v in m[:H]):
            raise ValueError("a row count is above the width")
        if any(v < 0 or v > H for v in m[H:]):
            raise ValueError("a column count is above the height")
        rows = [r for r in range(H) if m[r] * 256 > W * self.frac]
        cols = [c for c in range(W) if m[H + c] * 256 > H * self.frac]
        if not rows or not cols:
            return False
        rect = (rows[0], rows[-1], cols[0], cols[-1])
        if self._rect is not None:
            u = self._rect
            rect = (min(u[0], rect[0]), max(u[1], rect[1]), min(u[2], rect[2]), max(u[3], rect[3]))
        self._rect = rect
        self.votes += 1
        return True

    def result(self):
        """(x, y, w, h, votes)"""
        T = B = L = R = 0
        if self._rect is not None:
            top, bottom, left, right = self._rect
            T, B, L, R = top, self.H - 1 - bottom, left, self.W - 1 - right

        def bar(v, a):
            return 0 if v < self.min_bar else v - v % a

        T, B, L, R = bar(T, self.ay), bar(B, self.ay), bar(L, self.ax), bar(R, self.ax)
        return L, T, self.W - L - R, self.H - T - B, self.votes


__all__ = ["crop_stats", "window_planes", "CropDetect", "MAX_LIMIT", "MAX_FRAC", "MAX_MIN_BAR"]
