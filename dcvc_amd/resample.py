"""Planes of integer samples at another size on the GPU (no reference counterpart): a separable Lanczos-3
filter with 12-bit integer coefficients, every output sample defined exactly.

``taps`` restates the host table of ``dcvc_resample_taps`` (include/dcvc_amd_ops.h, csrc/kernels/resample.hip) operation for
operation in numpy float64; the tests hold the two against each other with ``==``. ``Plan`` and ``resample_planes`` are thin
wrappers over ``dcvc_resample_plan_create`` / ``dcvc_resample_planes``; the kernels run on ``torch.cuda.current_stream()``.

Sample tensors are ``torch.uint8``, or 16-bit as yuv16.py takes and returns them: ``torch.uint16`` or ``torch.int16`` storage
read as unsigned in, ``yuv16.u16_dtype()`` out.
"""
import ctypes
import math

import numpy as np

from . import _lib
from .yuv16 import DCVC_SAMPLE_U8, DCVC_SAMPLE_U16, _u16_dtypes, u16_dtype

MAX_RATIO = 8

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_fns = {}
_SIGS = {
    "dcvc_resample_ntaps": (_ci, [_ci, _ci]),
    "dcvc_resample_taps": (_ci, [_ci, _ci, _vp, _vp]),
    "dcvc_resample_plan_create": (_ci, [_ci, _ci, _ci, _ci, ctypes.POINTER(_vp)]),
    "dcvc_resample_plan_free": (_ci, [_vp]),
    "dcvc_resample_workspace_bytes": (_ll, [_vp, _ci]),
    "dcvc_resample_planes": (_ci, [_vp, _vp, _ci, _ci, _ll, _vp, _ci, _ci, _ll, _ci, _ci, _vp, _ll, _vp]),
}


def _fn(name):
    if name not in _fns:
        _fns[name] = _lib.fn(name, *_SIGS[name])
    return _fns[name]


def ntaps(n_in, n_out):
    """T of a pass n_in -> n_out: 2 ceil(3 max(1, n_in / n_out)); ValueError outside the ratios [1/8, 8]"""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1 or n_in > MAX_RATIO * n_out or n_out > MAX_RATIO * n_in:
        raise ValueError("resample: lengths must be positive at a ratio in [1/8, 8], got %d -> %d" % (n_in, n_out))
    scale = np.float64(n_in) / np.float64(n_out)
    fs = scale if scale > 1.0 else np.float64(1.0)
    return 2 * int(math.ceil(3.0 * fs))


def _lanczos3(t):
    a = np.pi * t
    b = np.pi * (t / 3.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (np.sin(a) / a) * (np.sin(b) / b)
    return np.where(np.abs(t) < 3.0, np.where(t == 0.0, 1.0, v), 0.0)


def taps(n_in, n_out):
    """The filter table of one pass: (coef int16 [n_out, T], first int32 [n_out]). Every row sums to 4096."""
    T = ntaps(n_in, n_out)
    scale = np.float64(n_in) / np.float64(n_out)
    fs = scale if scale > 1.0 else np.float64(1.0)
    support = 3.0 * fs
    centre = (np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5
    first = np.floor(centre - support).astype(np.int64) + 1
    w = np.empty((n_out, T), dtype=np.float64)
    total = np.zeros(n_out, dtype=np.float64)
    for k in range(T):
        w[:, k] = _lanczos3(((first + k).astype(np.float64) - centre) / fs)
        total = total + w[:, k]
    c = np.rint(w * 4096.0 / total[:, None]).astype(np.int64)
    c[np.arange(n_out), np.argmax(c, axis=1)] += 4096 - c.sum(axis=1)      # the largest, the first one on a tie
    return c.astype(np.int16), first.astype(np.int32)


def native_taps(n_in, n_out):
    """dcvc_resample_taps itself (host code, no GPU): (coef int16 [n_out, T], first int32 [n_out])"""
    T = _fn("dcvc_resample_ntaps")(int(n_in), int(n_out))
    if T < 0:
        raise ValueError("resample: lengths must be positive at a ratio in [1/8, 8], got %d -> %d" % (n_in, n_out))
    coef = np.empty((n_out, T), dtype=np.int16)
    first = np.empty(n_out, dtype=np.int32)
    _lib.check(_fn("dcvc_resample_taps")(int(n_in), int(n_out), _vp(coef.ctypes.data), _vp(first.ctypes.data)))
    return coef, first


class Plan:
    """The device tables of in_h x in_w -> out_h x out_w on the current CUDA device, made once and used call after call."""

    def __init__(self, in_h, in_w, out_h, out_w):
        self.in_h, self.in_w, self.out_h, self.out_w = int(in_h), int(in_w), int(out_h), int(out_w)
        self._p = _vp()
        _lib.check(_fn("dcvc_resample_plan_create")(self.in_h, self.in_w, self.out_h, self.out_w, ctypes.byref(self._p)))

    def workspace_bytes(self, n_planes):
        return int(_fn("dcvc_resample_workspace_bytes")(self._p, int(n_planes)))

    def close(self):
        if self._p:
            _lib.check(_fn("dcvc_resample_plan_free")(self._p))
            self._p = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, t, max_val, out=None, workspace=None):
        """t: [P, in_h, in_w] or [in_h, in_w] CUDA samples, unit stride along a row (row and plane strides may be larger).
        out: a tensor of the output shape to write into (strided likewise), else a new contiguous one. Returns out."""
        import torch
        squeeze = t.dim() == 2
        if squeeze:
            t = t[None]
        if t.dim() != 3 or not t.is_cuda or tuple(t.shape[1:]) != (self.in_h, self.in_w):
            raise ValueError("resample: CUDA planes [P, %d, %d] or [%d, %d] expected, got %s"
                             % (self.in_h, self.in_w, self.in_h, self.in_w, tuple(t.shape)))
        if t.dtype == torch.uint8:
            code, out_dtype = DCVC_SAMPLE_U8, torch.uint8
        elif t.dtype in _u16_dtypes():
            code, out_dtype = DCVC_SAMPLE_U16, u16_dtype()
        else:
            raise TypeError("resample: planes must be uint8 or uint16 / int16 (unsigned samples), got %s" % t.dtype)
        if t.stride(2) != 1:
            t = t.contiguous()
        P = t.shape[0]
        if out is None:
            o = torch.empty((P, self.out_h, self.out_w), dtype=out_dtype, device=t.device)
        else:
            o = out[None] if out.dim() == 2 else out
            if (tuple(o.shape) != (P, self.out_h, self.out_w) or o.device != t.device or o.stride(2) != 1
                    or o.element_size() != t.element_size() or o.dtype.is_floating_point):
                raise ValueError("resample: out must hold [%d, %d, %d] samples of t's width on t's device, rows at unit stride"
                                 % (P, self.out_h, self.out_w))
        need = self.workspace_bytes(P)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=t.device)
        _lib.check(_fn("dcvc_resample_planes")(
            self._p, _vp(t.data_ptr()), code, t.stride(1), t.stride(0), _vp(o.data_ptr()), code, o.stride(1), o.stride(0), P,
            int(max_val), _vp(workspace.data_ptr()), workspace.numel() * workspace.element_size(),
            _vp(torch.cuda.current_stream(t.device).cuda_stream)))
        if out is not None:
            return out
        return o[0] if squeeze else o


def resample_planes(t, out_h, out_w, max_val):
    """t: [P, H, W] or [H, W] CUDA samples (uint8; uint16 or int16 storage read as unsigned) -> the planes at out_h x out_w,
    every plane on its own, in one call. max_val: 255, or 2^bit_depth - 1 for 16-bit samples."""
    plan = Plan(t.shape[-2], t.shape[-1], out_h, out_w)
    try:
        return plan.run(t, max_val)
    finally:
        plan.close()


__all__ = ["ntaps", "taps", "native_taps", "Plan", "resample_planes", "MAX_RATIO"]
