"""The block motion search and the motion compensation of DESIGN.md 31 (csrc/kernels/motion.hip, dcvc encode --denoise-mc)
restated in numpy, operation for operation, in signed integers: the GPU tests hold the kernels and the tool against it with ==.
Vectorised over blocks, the candidate loop outside.

sh = bit_depth - 8, L = lambda << sh; blocks are 16x16 luma samples, Bh = ceil(H / 16), Bw = ceil(W / 16).
  half resolution: a1[y][x] = (a[2y][2x] + a[2y][2x+1] + a[2y+1][2x] + a[2y+1][2x+1] + 2) >> 2, indexes clamped to the plane.
  block SAD:       over the block's samples inside cur; the reference index (y + dy, x + dx) is clamped to the plane.
  order:           the smallest tuple (cost, |dx| + |dy|, dy, dx) wins.
  level 1:         the 8x8 block of the half-resolution planes, every dx, dy in -R..R, cost = SAD + L (|dx| + |dy|) -> (dx1, dy1).
  level 0:         the 16x16 block, candidates (2 dx1 + ex, 2 dy1 + ey), ex, ey in -1..1, and (0, 0),
                   cost = SAD + 4 L (|dx| + |dy|) -> mv, and the winner's SAD without the penalty.
  compensation:    a plane subsampled by (sx, sy): the block of (y, x) is (y // (16 >> sy), x // (16 >> sx)),
                   dxc = dx >> sx, dyc = dy >> sy (floor), dst[y][x] = prev[clamp(y + dyc)][clamp(x + dxc)].
"""
import numpy as np

import denoise_np

I64 = np.int64
BLOCK = 16


def grid(H, W):
    return (H + BLOCK - 1) // BLOCK, (W + BLOCK - 1) // BLOCK


def half_plane(a):
    """[H, W] integer samples -> [ceil(H / 2), ceil(W / 2)] int64"""
    a = np.asarray(a).astype(I64)
    H, W = a.shape
    a = np.pad(a, ((0, H & 1), (0, W & 1)), mode="edge")
    return (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2


def _gather(ref, DY, DX):
    """ref[clamp(y + DY[y, x]), clamp(x + DX[y, x])]; DY, DX scalars or [H, W]"""
    H, W = ref.shape
    if np.ndim(DY) == 0:
        return ref[np.clip(np.arange(H) + DY, 0, H - 1)][:, np.clip(np.arange(W) + DX, 0, W - 1)]
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    return ref[np.clip(yy + DY, 0, H - 1), np.clip(xx + DX, 0, W - 1)]


def _block_sums(d, B):
    """[H, W] -> [ceil(H / B), ceil(W / B)] sums over B x B blocks; a partial block sums the samples it has"""
    H, W = d.shape
    d = np.pad(d, ((0, -H % B), (0, -W % B)))
    return d.reshape(d.shape[0] // B, B, d.shape[1] // B, B).sum(axis=(1, 3))


def _per_sample(v, B, H, W):
    return np.repeat(np.repeat(v, B, axis=0), B, axis=1)[:H, :W]


def _key(cost, dy, dx):
    # (cost, |dx| + |dy|, dy, dx) as one integer; |dx|, |dy| <= 31
    return (cost << 20) | ((np.abs(dx) + np.abs(dy)) << 14) | ((dy + 64) << 7) | (dx + 64)


def _best(cur, ref, B, pen, candidates):
    """candidates: (dy, dx) pairs, scalars or per-block arrays -> the winning (dx, dy, sad) per block"""
    H, W = cur.shape
    best = bdx = bdy = bsad = None
    for dy, dx in candidates:
        per_block = np.ndim(dy) > 0
        DY = _per_sample(dy, B, H, W) if per_block else dy
        DX = _per_sample(dx, B, H, W) if per_block else dx
        sad = _block_sums(np.abs(cur - _gather(ref, DY, DX)), B)
        dyb, dxb = np.broadcast_to(dy, sad.shape).astype(I64), np.broadcast_to(dx, sad.shape).astype(I64)
        cost = sad + pen * (np.abs(dxb) + np.abs(dyb))
        assert cost.max() < 2 ** 31
        key = _key(cost, dyb, dxb)
        if best is None:
            best, bdx, bdy, bsad = key, dxb.copy(), dyb.copy(), sad
        else:
            w = key < best
            best, bdx, bdy, bsad = np.where(w, key, best), np.where(w, dxb, bdx), np.where(w, dyb, bdy), np.where(w, sad, bsad)
    return bdx, bdy, bsad


def motion_search(cur, ref, bit_depth, R=7, lam=4):
    """cur, ref [H, W] integer samples -> (mv int16 [Bh, Bw, 2] holding (dx, dy), sad uint32 [Bh, Bw])"""
    assert 0 <= R <= 15 and 0 <= lam <= 255 and 8 <= bit_depth <= 16
    cur, ref = np.asarray(cur).astype(I64), np.asarray(ref).astype(I64)
    L = lam << (bit_depth - 8)
    c1, r1 = half_plane(cur), half_plane(ref)
    dx1, dy1, _ = _best(c1, r1, BLOCK // 2, L, [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)])
    assert dx1.shape == grid(*cur.shape)
    zero = np.zeros_like(dx1)
    cands = [(2 * dy1 + ey, 2 * dx1 + ex) for ey in (-1, 0, 1) for ex in (-1, 0, 1)] + [(zero, zero)]
    dx, dy, sad = _best(cur, ref, BLOCK, 4 * L, cands)
    return np.stack([dx, dy], axis=-1).astype(np.int16), sad.astype(np.uint32)


def compensate_plane(prev, mv, sx=0, sy=0):
    """prev [H, W] samples of a plane subsampled by (sx, sy) against the searched luma, mv [Bh, Bw, 2] -> dst of prev's type"""
    prev = np.asarray(prev)
    H, W = prev.shape
    mv = np.asarray(mv).astype(I64)
    by, bx = np.arange(H) // (BLOCK >> sy), np.arange(W) // (BLOCK >> sx)
    assert by[-1] < mv.shape[0] and bx[-1] < mv.shape[1]
    v = mv[by[:, None], bx[None, :]]
    return _gather(prev, v[..., 1] >> sy, v[..., 0] >> sx)


def mc_denoise_clip(clip, spatial, temporal, bit_depth, R, lam, sx=1, sy=1):
    """clip: a list of pictures (y, u, v), chroma subsampled by (sx, sy) -> (the filtered pictures, the vectors and SADs of
    every picture that had a previous output; None where none was searched), as dcvc encode --denoise S:T --denoise-mc R:LAMBDA"""
    out, mvs, prev = [], [], None
    for pic in clip:
        if prev is None or temporal == 0:
            comp, found = prev, None
        else:
            found = motion_search(pic[0], prev[0], bit_depth, R, lam)
            comp = (compensate_plane(prev[0], found[0]),) + tuple(compensate_plane(p, found[0], sx, sy) for p in prev[1:])
        prev = tuple(denoise_np.denoise_plane(p, None if comp is None else comp[i], spatial, temporal, bit_depth)
                     for i, p in enumerate(pic))
        out.append(prev)
        mvs.append(found)
    return out, mvs
