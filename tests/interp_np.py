"""The frame-rate conversion of DESIGN.md 32 (csrc/kernels/interp.hip, dcvc decode --interpolate) restated in numpy on top of
motion_np.py, operation for operation, in signed integers: the GPU tests hold the kernels and the tool against it with ==.

A is the earlier picture, B the later; N in 2..8, k in 1..N-1: the picture at k / N of the way from A to B. sh = bit_depth - 8.
Blocks are 16x16 luma samples; indexes into a plane are clamped to it; divisions are floor divisions.
  vectors:       mv = motion_search(cur = B, ref = A), so B[p] ~ A[p + v]; each component is clamped to -31..31 when read.
  split:         per component a = (2 k v + N) // (2 N), b = a - v: the in-between sample at p is seen at A[p + a], B[p + b].
  selection:     luma; candidates: the clamped vectors of the 3x3 neighbourhood of mv[by][bx] (grid indexes clamped) and (0, 0);
                 SAD(v) = sum |A[p + a] - B[p + b]| over the block's samples inside the plane; the smallest tuple
                 (SAD, |vx| + |vy|, vy, vx) wins; the block falls back when SAD > (LIMIT << sh) * n, n the samples summed.
                 plan = (ax, ay, bx, by), wb = k; a fallen block: offsets 0, wb = 0 when 2 k <= N, else N.
  interpolation: a plane subsampled by (sx, sy): the block of (y, x) is (y // (16 >> sy), x // (16 >> sx)), offsets
                 ax >> sx, ay >> sy, bx >> sx, by >> sy, w = min(wb, N), dst = ((N - w) A[..] + w B[..] + (N >> 1)) // N.
  picture rule:  with fallen and n_blocks given and 2 * fallen > n_blocks every block is treated as fallen.
"""
import numpy as np

import motion_np
from motion_np import BLOCK, I64, _block_sums, _gather, _key, _per_sample, grid

MAX_VEC = 31


def split(v, k, N):
    """a component (or an array of them) of a vector -> (a, b), the offsets into A and B"""
    v = np.asarray(v).astype(I64)
    a = (2 * k * v + N) // (2 * N)
    return a, a - v


def key(sad, vy, vx):
    """the tuple (SAD, |vx| + |vy|, vy, vx) as one integer: 31's key with cost = SAD"""
    return _key(np.asarray(sad).astype(I64), np.asarray(vy).astype(I64), np.asarray(vx).astype(I64))


def interp_select(A, B, mv, bit_depth, k, N, limit=8):
    """A, B [H, W] luma samples, mv [>= Bh, >= Bw, 2] any int16 values holding (dx, dy) ->
    (plan int16 [Bh, Bw, 4] = (ax, ay, bx, by), wb uint8 [Bh, Bw], sad uint32 [Bh, Bw], fallen: the number of fallen blocks)"""
    assert 2 <= N <= 8 and 1 <= k <= N - 1 and 0 <= limit <= 255 and 8 <= bit_depth <= 16
    A, B = np.asarray(A).astype(I64), np.asarray(B).astype(I64)
    H, W = A.shape
    Bh, Bw = grid(H, W)
    mv = np.clip(np.asarray(mv).astype(I64)[:Bh, :Bw], -MAX_VEC, MAX_VEC)
    assert mv.shape == (Bh, Bw, 2)
    gy, gx = np.arange(Bh), np.arange(Bw)
    cands = []
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            c = mv[np.clip(gy + j, 0, Bh - 1)][:, np.clip(gx + i, 0, Bw - 1)]
            cands.append((c[..., 0], c[..., 1]))
    zero = np.zeros((Bh, Bw), I64)
    cands.append((zero, zero))
    best = bvx = bvy = None
    for vx, vy in cands:
        ax, bx = split(vx, k, N)
        ay, by = split(vy, k, N)
        sa = _gather(A, _per_sample(ay, BLOCK, H, W), _per_sample(ax, BLOCK, H, W))
        sb = _gather(B, _per_sample(by, BLOCK, H, W), _per_sample(bx, BLOCK, H, W))
        sad = _block_sums(np.abs(sa - sb), BLOCK)
        assert sad.max() < 2 ** 24
        kk = key(sad, vy, vx)
        if best is None:
            best, bvx, bvy = kk, vx.copy(), vy.copy()
        else:
            w = kk < best
            best, bvx, bvy = np.where(w, kk, best), np.where(w, vx, bvx), np.where(w, vy, bvy)
    sad = best >> 20
    n = _block_sums(np.ones((H, W), I64), BLOCK)
    fell = sad > (limit << (bit_depth - 8)) * n
    ax, bx = split(bvx, k, N)
    ay, by = split(bvy, k, N)
    plan = np.stack([ax, ay, bx, by], axis=-1)
    plan[fell] = 0
    wb = np.where(fell, 0 if 2 * k <= N else N, k)
    return plan.astype(np.int16), wb.astype(np.uint8), sad.astype(np.uint32), int(fell.sum())


def interp_plane(A, B, plan, wb, k, N, sx=0, sy=0, fallen=None, n_blocks=None):
    """A, B [H, W] samples of a plane subsampled by (sx, sy) against the luma of the selection; plan [>= bh, >= bw, 4] any int16
    values, wb [>= bh, >= bw] any uint8 values -> the in-between plane, of A's type"""
    assert 2 <= N <= 8 and 1 <= k <= N - 1
    A = np.asarray(A)
    H, W = A.shape
    a, b = A.astype(I64), np.asarray(B).astype(I64)
    by, bx = np.arange(H) // (BLOCK >> sy), np.arange(W) // (BLOCK >> sx)
    plan, wb = np.asarray(plan).astype(I64), np.asarray(wb).astype(I64)
    assert by[-1] < plan.shape[0] and bx[-1] < plan.shape[1] and plan.shape[:2] == wb.shape
    if fallen is not None and 2 * fallen > n_blocks:
        plan, wb = np.zeros_like(plan), np.full_like(wb, 0 if 2 * k <= N else N)
    p = plan[by[:, None], bx[None, :]]
    w = np.minimum(wb[by[:, None], bx[None, :]], N)
    sa = _gather(a, p[..., 1] >> sy, p[..., 0] >> sx)
    sb = _gather(b, p[..., 3] >> sy, p[..., 2] >> sx)
    out = ((N - w) * sa + w * sb + (N >> 1)) // N
    assert out.max() <= max(a.max(), b.max())
    return out.astype(A.dtype)


def interp_between(a_planes, b_planes, mv, bit_depth, k, N, limit=8, sx=1, sy=1, picture_rule=True):
    """pictures (y, u, v), chroma subsampled by (sx, sy), and the vectors of the search of B's luma against A's ->
    (the picture at k / N, fallen, the sum of the winners' SADs), as dcvc decode --interpolate makes it"""
    plan, wb, sad, fallen = interp_select(a_planes[0], b_planes[0], mv, bit_depth, k, N, limit)
    f, nb = (fallen, wb.size) if picture_rule else (None, None)
    pic = (interp_plane(a_planes[0], b_planes[0], plan, wb, k, N, 0, 0, f, nb),) + \
        tuple(interp_plane(pa, pb, plan, wb, k, N, sx, sy, f, nb) for pa, pb in zip(a_planes[1:], b_planes[1:]))
    return pic, fallen, int(sad.astype(I64).sum())


def interpolate(a_planes, b_planes, bit_depth, N, R=7, lam=4, limit=8, sx=1, sy=1, picture_rule=True):
    """-> the N - 1 in-between pictures, k = 1..N-1: one search, then selection and interpolation per phase"""
    mv, _ = motion_np.motion_search(b_planes[0], a_planes[0], bit_depth, R, lam)
    return [interp_between(a_planes, b_planes, mv, bit_depth, k, N, limit, sx, sy, picture_rule)[0] for k in range(1, N)]


def interpolate_clip(clip, bit_depth, N, R=7, lam=4, limit=8, sx=1, sy=1):
    """a list of pictures (y, u, v) -> (the N (n - 1) + 1 output pictures in output order, a record
    {out_idx, after, k, blocks, fallen, repeated, sum_sad} per in-between picture); a change of size restarts"""
    out, log, prev = [], [], None
    for i, pic in enumerate(clip):
        if prev is not None and prev[0].shape == pic[0].shape:
            mv, _ = motion_np.motion_search(pic[0], prev[0], bit_depth, R, lam)
            for k in range(1, N):
                mid, fallen, sum_sad = interp_between(prev, pic, mv, bit_depth, k, N, limit, sx, sy)
                nb = int(np.prod(grid(*pic[0].shape)))
                log.append(dict(out_idx=len(out), after=i - 1, k=k, blocks=nb, fallen=fallen, repeated=int(2 * fallen > nb), sum_sad=sum_sad))
                out.append(mid)
        out.append(tuple(np.asarray(p) for p in pic))
        prev = pic
    return out, log


def psnr(a, b, bit_depth):
    d = np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)
    mse = float((d * d).mean())
    return float("inf") if mse == 0 else 10 * np.log10(((1 << bit_depth) - 1) ** 2 / mse)
