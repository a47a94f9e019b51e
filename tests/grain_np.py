"""Film grain restated in numpy: signed 64-bit integers and Python ints. The template, the block offsets, the
synthesis (dcvc_grain_apply), the measurement (dcvc_grain_stats) and the fit (dcvc_grain_fit) - what the kernels, the C host
code and dcvc_amd/grain.py are held against with ==.

sh = bit_depth - 8, max_val = 2^bit_depth - 1; u32 arithmetic wraps modulo 2^32; shifts of signed values are arithmetic."""
import functools
import math

import numpy as np

I64 = np.int64
M32 = 0xFFFFFFFF
MAX_SIZE = 37


def _dtype(bit_depth):
    if not 8 <= bit_depth <= 16:
        raise ValueError("bit_depth must be 8..16")
    return np.uint8 if bit_depth == 8 else np.uint16


@functools.lru_cache(maxsize=None)
def _white(seed, plane):
    """the 64 x 64 white samples of (seed, plane): the same for every size"""
    s = (seed * 0x9E3779B1 + plane * 0xC2B2AE3D + 1) & M32
    w = np.empty(4096, I64)
    for i in range(4096):
        t = 0
        for _ in range(4):
            s = (s * 1664525 + 1013904223) & M32
            t += s >> 24
        w[i] = t - 510
    return w.reshape(64, 64)


def template(seed, plane, size):
    """-> int16 [64, 64]"""
    if not 0 <= plane <= 2 or not 0 <= size <= MAX_SIZE:
        raise ValueError("plane 0..2 and size 0..37 expected")
    w = _white(seed, plane)
    a, b = I64(size), I64(128 - 2 * size)
    h = a * np.roll(w, 1, axis=1) + b * w + a * np.roll(w, -1, axis=1)
    f = a * np.roll(h, 1, axis=0) + b * h + a * np.roll(h, -1, axis=0)
    Q = sum(int(v) * int(v) for v in f.ravel())
    rms = math.isqrt(Q // 4096)
    if rms == 0:
        raise ValueError("the filtered noise is zero")
    T = np.floor_divide(128 * f + rms, 2 * rms)
    assert np.abs(T).max() <= 1023
    return T.astype(np.int16)


def block_offsets(seed, pic, p, nby, nbx):
    """-> (ox, oy), int64 [nby, nbx] each: the template offsets of the 32 x 32 blocks of plane p of picture pic"""
    by, bx = np.mgrid[0:nby, 0:nbx].astype(np.uint64)
    m = np.uint64(M32)
    base = np.uint64((seed * 0x9E3779B1 + pic * 0x85EBCA77 + p * 0xC2B2AE3D) & M32)
    h = (base + by * np.uint64(0x27D4EB2F) + bx * np.uint64(0x165667B1)) & m          # products below 2^46: no 64-bit wrap
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    return (h & np.uint64(63)).astype(I64), ((h >> np.uint64(8)) & np.uint64(63)).astype(I64)


def collocated_luma(luma, H, W, sx, sy):
    """luma [Hl, Wl] -> L int64 [H, W] for a plane subsampled by (sx, sy), indexes clamped into the luma plane"""
    Yl = np.asarray(luma).astype(I64)
    Hl, Wl = Yl.shape
    if Hl < ((H - 1) << sy) + 1 or Wl < ((W - 1) << sx) + 1:
        raise ValueError("the luma plane is too small")
    ys = np.minimum(np.arange(H) << sy, Hl - 1)
    xs = np.arange(W) << sx
    if sx == 0:
        return Yl[np.ix_(ys, np.minimum(xs, Wl - 1))]
    return (Yl[np.ix_(ys, np.minimum(xs, Wl - 1))] + Yl[np.ix_(ys, np.minimum(xs + 1, Wl - 1))] + 1) >> 1


def _intensity(L, sh):
    return np.minimum(L >> sh, 255)          # the min binds only for samples above max_val


def grain_samples(shape, luma, T, lut, seed, pic, p, bit_depth, sx, sy):
    """-> n int64 [H, W]: what apply adds to plane p before the clamp"""
    H, W = shape
    sh = bit_depth - 8
    ox, oy = block_offsets(seed, pic, p, (H + 31) // 32, (W + 31) // 32)
    y, x = np.mgrid[0:H, 0:W]
    t = np.asarray(T).astype(I64).reshape(64, 64)[(oy[y >> 5, x >> 5] + (y & 31)) & 63, (ox[y >> 5, x >> 5] + (x & 31)) & 63]
    i = _intensity(collocated_luma(luma, H, W, sx, sy), sh)
    k, fr = i >> 5, i & 31
    lt = np.asarray(lut).astype(I64)
    assert lt.shape == (9,) and lt.min() >= 0 and lt.max() <= 255
    v = (lt[k] * (32 - fr) + lt[k + 1] * fr + 16) >> 5
    return (t * v + (1 << (9 - sh))) >> (10 - sh)


def apply_plane(rec, luma, T, lut, seed, pic, p, bit_depth, sx, sy):
    """rec [H, W] (plane p of Y, U, V), the UNGRAINED luma plane, the plane's template and table -> the grained plane"""
    r = np.asarray(rec)
    n = grain_samples(r.shape, luma, T, lut, seed, pic, p, bit_depth, sx, sy)
    return np.clip(r.astype(I64) + n, 0, (1 << bit_depth) - 1).astype(_dtype(bit_depth))


def stats_plane(src, den, luma, bit_depth, sx, sy, flat):
    """-> 16 Python ints: n[0..7], S[0..7]"""
    s, d = np.asarray(src).astype(I64), np.asarray(den).astype(I64)
    H, W = d.shape
    sh = bit_depth - 8
    if not 0 <= flat <= 255:
        raise ValueError("flat 0..255 expected")
    lim = flat << sh
    p = np.pad(d, 1, mode="edge")
    ok = ((np.abs(p[:-2, 1:-1] - d) <= lim) & (np.abs(p[2:, 1:-1] - d) <= lim) & (np.abs(p[1:-1, :-2] - d) <= lim)
          & (np.abs(p[1:-1, 2:] - d) <= lim))
    bn = _intensity(collocated_luma(luma, H, W, sx, sy), sh) >> 5
    dd = (s - d) ** 2
    words = [0] * 16
    assert H * W < 1 << 30                    # d^2 < 2^32: the int64 sums below cannot wrap
    for k in range(8):
        m = ok & (bn == k)
        words[k] = int(m.sum())
        words[8 + k] = int(dd[m].sum(dtype=I64))
    return words


def fit_bins(w, bit_depth, gain_percent, min_count):
    """the 16 words of one plane -> {bin: value} of the bins with n >= min_count (step 1 of the fit)"""
    if not 8 <= bit_depth <= 16 or not 1 <= gain_percent <= 400 or min_count < 1:
        raise ValueError("bit_depth 8..16, gain 1..400 and min_count >= 1 expected")
    sh = bit_depth - 8
    n, S = [int(v) for v in w[:8]], [int(v) for v in w[8:]]
    return {k: min(255, math.isqrt((256 * S[k] * gain_percent * gain_percent) // ((n[k] * 10000) << (2 * sh))))
            for k in range(8) if n[k] >= min_count}


def fit(words, bit_depth, gain_percent, min_count):
    """words: three lists of 16 ints (Y, U, V) -> three tables of nine ints"""
    luts = []
    for w in words:
        val = fit_bins(w, bit_depth, gain_percent, min_count)
        valid = sorted(val)
        if not valid:
            luts.append([0] * 9)
            continue
        full = [val[min(valid, key=lambda j: (abs(j - k), j))] for k in range(8)]
        luts.append([full[0]] + [(full[k - 1] + full[k] + 1) >> 1 for k in range(1, 8)] + [full[7]])
    return luts
