"""The integer Lanczos-3 resampler of DESIGN.md 17 in numpy, for the tests: the filter table of a 1-D pass and
``resample_plane`` in int64. Written from the filter's definition and independent of the library (it imports nothing of it).

One pass n_in -> n_out: scale = n_in / n_out, fs = max(1, scale), support = 3 fs, T = 2 ceil(support); output j has
centre = (j + 0.5) scale - 0.5, first = floor(centre - support) + 1, w[k] = L((first + k - centre) / fs) with
L(t) = sinc(t) sinc(t / 3) inside |t| < 3; c[k] = rint(w[k] * 4096 / sum w), the rest of 4096 goes to the largest c (the first one
on a tie). out[j] = clamp((sum_k c[k] in[clamp(first + k, 0, n_in - 1)] + 2048) >> 12, 0, max_val). Horizontal pass first."""
import math

import numpy as np


def ntaps(n_in, n_out):
    if n_in < 1 or n_out < 1 or n_in > 8 * n_out or n_out > 8 * n_in:
        raise ValueError("ratio outside [1/8, 8]: %d -> %d" % (n_in, n_out))
    return 2 * int(math.ceil(3.0 * max(1.0, n_in / n_out)))


def _sinc(t):
    x = np.pi * t
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(t == 0.0, 1.0, np.sin(x) / x)


def taps(n_in, n_out):
    """(coef int16 [n_out, T], first int32 [n_out])"""
    T = ntaps(n_in, n_out)
    scale = n_in / n_out
    fs = max(1.0, scale)
    support = 3.0 * fs
    centre = (np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5
    first = np.floor(centre - support).astype(np.int64) + 1
    pos = first[:, None] + np.arange(T, dtype=np.int64)[None, :]
    t = (pos.astype(np.float64) - centre[:, None]) / fs
    w = np.where(np.abs(t) < 3.0, _sinc(t) * _sinc(t / 3.0), 0.0)
    total = np.zeros(n_out, dtype=np.float64)
    for k in range(T):                      # in tap order, as a loop adds them
        total = total + w[:, k]
    c = np.rint(w * 4096.0 / total[:, None]).astype(np.int64)
    rows = np.arange(n_out)
    c[rows, np.argmax(c, axis=1)] += 4096 - c.sum(axis=1)       # argmax: the first of equal maxima
    return c.astype(np.int16), first.astype(np.int32)


def _pass(a, n_out, max_val):
    """the last axis of the int64 array a, n_in -> n_out"""
    n_in = a.shape[-1]
    c, first = taps(n_in, n_out)
    idx = np.clip(first.astype(np.int64)[:, None] + np.arange(c.shape[1])[None, :], 0, n_in - 1)      # [n_out, T]
    acc = (a[..., idx] * c.astype(np.int64)).sum(axis=-1)
    return np.clip((acc + 2048) >> 12, 0, max_val)


def resample_plane(a, out_h, out_w, max_val):
    """a: [H, W] unsigned samples -> [out_h, out_w] of a's dtype; the horizontal pass, its clamp, then the vertical pass"""
    a = np.asarray(a)
    mid = _pass(a.astype(np.int64), out_w, max_val)                       # [H, out_w]
    out = _pass(np.ascontiguousarray(mid.T), out_h, max_val).T            # [out_h, out_w]
    return np.ascontiguousarray(out).astype(a.dtype)
