"""The deinterlacer of DESIGN.md 27 (csrc/kernels/deinterlace.hip, dcvc encode --deinterlace) restated in numpy, operation for
operation, in signed 32-bit integers: the GPU tests hold the kernel and the tool against it with ==.

Per plane, T = threshold << (bit_depth - 8). Rows y with y % 2 == keep are copied from cur. For a missing row y:
  ya = y - 1 (y + 1 at the top), yb = y + 1 (y - 1 at the bottom), A = cur[ya], B = cur[yb], column indexes clamped.
  spatial: for d in 0, -1, +1: score_d = sum over j in -1..1 of |A[x + j + d] - B[x + j - d]|,
           pred_d = (A[x + d] + B[x - d] + 1) >> 1; the smallest score wins, a later d only when strictly smaller; sp = pred_best.
  no prev or T == 0: out = sp. Else m = max over rows {ya, y, yb}, columns x - 1 .. x + 1 of |cur - prev|,
           k = (256 max(0, T - m)) // T, wv = prev[y][x] if weave_from_prev else cur[y][x],
           out = sp + ((k (wv - sp) + 128) >> 8).
"""
import numpy as np

I32 = np.int32
DIRECTIONS = (0, -1, 1)


def _dtype(bit_depth):
    if not 8 <= bit_depth <= 16:
        raise ValueError("bit_depth must be 8..16")
    return np.uint8 if bit_depth == 8 else np.uint16


def _cols(row, shift):
    """row[clamp(x + shift)] for every x"""
    W = row.shape[-1]
    return row[..., np.clip(np.arange(W) + shift, 0, W - 1)]


def neighbour_rows(y, H):
    """(ya, yb) of a missing row"""
    return (y - 1 if y - 1 >= 0 else y + 1), (y + 1 if y + 1 < H else y - 1)


def scores_row(A, B):
    """A, B [W] int32 -> the scores of the three directions, in the order of DIRECTIONS"""
    out = []
    for d in DIRECTIONS:
        score = np.zeros(A.shape, I32)
        for j in (-1, 0, 1):
            score = score + np.abs(_cols(A, j + d) - _cols(B, j - d))
        out.append(score)
    return out


def spatial_row(A, B):
    """A, B [W] int32: the rows above and below -> (sp [W] int32, the winning direction [W])"""
    best = pred = which = None
    for d, score in zip(DIRECTIONS, scores_row(A, B)):
        p = (_cols(A, d) + _cols(B, -d) + I32(1)) >> I32(1)
        if best is None:
            best, pred, which = score, p, np.full(A.shape, d, I32)
        else:
            take = score < best
            best, pred, which = np.where(take, score, best), np.where(take, p, pred), np.where(take, I32(d), which)
    return pred.astype(I32), which


def deinterlace_plane(cur, prev, keep, weave_from_prev, threshold, bits):
    """one woven plane (uint8 at 8 bits, uint16 above) and the same plane of the previous INPUT frame (or None) -> the output"""
    if keep not in (0, 1) or weave_from_prev not in (0, 1) or not 0 <= threshold <= 64:
        raise ValueError("keep and weave_from_prev are 0 or 1, threshold is 0..64")
    c = np.asarray(cur).astype(I32)
    H, W = c.shape
    if H < 2 or W < 1:
        raise ValueError("H >= 2 and W >= 1")
    T = I32(int(threshold) << (bits - 8))
    p = None if prev is None or threshold == 0 else np.asarray(prev).astype(I32)
    out = c.copy()
    if p is not None:
        diff = np.abs(c - p)
        colmax = np.maximum(np.maximum(_cols(diff, -1), diff), _cols(diff, 1))      # max over x - 1 .. x + 1 of every row
    for y in range(1 - keep, H, 2):
        ya, yb = neighbour_rows(y, H)
        sp, _ = spatial_row(c[ya], c[yb])
        if p is None:
            out[y] = sp
            continue
        m = np.maximum(np.maximum(colmax[ya], colmax[y]), colmax[yb])
        k = (I32(256) * np.maximum(I32(0), T - m)) // T
        wv = p[y] if weave_from_prev else c[y]
        out[y] = sp + ((k * (wv - sp) + I32(128)) >> I32(8))
    assert out.dtype == I32
    return out.astype(_dtype(bits))


def picture_params(mode, order):
    """the (keep, weave_from_prev) of the coded pictures a source frame gives, in order"""
    if mode not in ("frame", "field") or order not in ("tff", "bff"):
        raise ValueError("mode is frame or field, order tff or bff")
    p0 = 0 if order == "tff" else 1
    return [(p0, 0)] if mode == "frame" else [(p0, 1), (1 - p0, 0)]


def deinterlace_clip(frames, mode, order, threshold, bits):
    """frames: a list of woven frames, each a plane or a tuple of planes -> the coded pictures in order (a frame's prev is the
    previous frame, none for the first), every plane on its own: one picture a frame (frame), or two (field)"""
    out, prev = [], None
    for f in frames:
        planes = f if isinstance(f, (tuple, list)) else (f,)
        for keep, weave in picture_params(mode, order):
            pic = tuple(deinterlace_plane(pl, None if prev is None else prev[i], keep, weave, threshold, bits) for i, pl in enumerate(planes))
            out.append(pic if isinstance(f, (tuple, list)) else pic[0])
        prev = planes
    return out
