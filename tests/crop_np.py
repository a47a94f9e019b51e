"""Black-bar cropping restated in numpy int64: the measurement dcvc_crop_stats, the copy dcvc_window_planes and
the decision dcvc_cropdet_*. The kernels and the host code are held against these with ==."""
import numpy as np


def crop_stats(luma, limit, bit_depth):
    """luma [H, W] unsigned samples -> int64 [H + W]: per row, then per column, the samples above limit << (bit_depth - 8)"""
    y = np.asarray(luma).astype(np.int64)
    above = y > (int(limit) << (int(bit_depth) - 8))
    return np.concatenate([above.sum(axis=1), above.sum(axis=0)]).astype(np.int64)


def window_planes(src, out_h, out_w, ox, oy, fill):
    """src [P, Hs, Ws] -> [P, out_h, out_w]: out[p][y][x] = src[p][y + oy][x + ox] inside the source, fill[p] outside"""
    src = np.asarray(src)
    P, Hs, Ws = src.shape
    fills = [int(fill)] * P if np.isscalar(fill) else [int(v) for v in fill]
    out = np.empty((P, out_h, out_w), dtype=src.dtype)
    ys, xs = np.arange(out_h) + int(oy), np.arange(out_w) + int(ox)
    inside = ((ys >= 0) & (ys < Hs))[:, None] & ((xs >= 0) & (xs < Ws))[None, :]
    yc, xc = np.clip(ys, 0, Hs - 1), np.clip(xs, 0, Ws - 1)
    for p in range(P):
        out[p] = np.where(inside, src[p][yc[:, None], xc[None, :]], np.asarray(fills[p], dtype=src.dtype))
    return out


def picture_vote(counts, H, W, frac):
    """(top, bottom, left, right) of a picture's active rows and columns, or None: no vote"""
    m = np.asarray(counts).astype(np.int64)
    rows = np.nonzero(m[:H] * 256 > W * int(frac))[0]
    cols = np.nonzero(m[H:] * 256 > H * int(frac))[0]
    if rows.size == 0 or cols.size == 0:
        return None
    return int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])


def crop_window(all_counts, H, W, frac, min_bar, ax, ay):
    """the counts of the probed pictures -> (x, y, w, h, votes)"""
    votes = [v for v in (picture_vote(c, H, W, frac) for c in all_counts) if v is not None]
    T = B = L = R = 0
    if votes:
        T = min(v[0] for v in votes)
        B = H - 1 - max(v[1] for v in votes)
        L = min(v[2] for v in votes)
        R = W - 1 - max(v[3] for v in votes)

    def bar(v, a):
        return 0 if v < min_bar else v // a * a

    T, B, L, R = bar(T, ay), bar(B, ay), bar(L, ax), bar(R, ax)
    return L, T, W - L - R, H - T - B, len(votes)


def probe_indexes(N, M):
    """the source frames dcvc encode --crop auto probes: N' = min(N, M) of M, spread over the clip"""
    n = min(int(N), int(M))
    return [((2 * k + 1) * M) // (2 * n) for k in range(n)]
