"""The deinterlacer of DESIGN.md 27 without a GPU: the properties of its numpy restatement (tests/deinterlace_np.py) and the
three claims of the design - a static scene is rewoven bit for bit, a pan comes out at least 8 dB above the woven frame, and on
a noisy static scene the motion-adaptive blend beats the purely spatial interpolator by at least 3 dB - at 8 and at 10 bits."""
import numpy as np
import pytest

import deinterlace_np as dnp

KINDS = [(8, np.uint8), (10, np.uint16), (16, np.uint16)]


def _random(bits, dtype, shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << bits, shape).astype(dtype)


def _near(cur, bits, seed, spread=6):
    """cur plus noise of a few code values (scaled by the depth)"""
    n = np.random.default_rng(seed).integers(-spread, spread + 1, cur.shape) * (1 << (bits - 8))
    return np.clip(cur.astype(np.int64) + n, 0, (1 << bits) - 1).astype(cur.dtype)


# ------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("bits,dtype", KINDS)
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("shape", [(2, 1), (7, 9), (12, 33)])
def test_kept_rows_are_untouched(bits, dtype, keep, shape):
    cur = _random(bits, dtype, shape, 1)
    for prev, weave, thr in ((None, 0, 10), (_near(cur, bits, 2), 0, 10), (_near(cur, bits, 2), 1, 64), (_random(bits, dtype, shape, 3), 1, 1)):
        out = dnp.deinterlace_plane(cur, prev, keep, weave, thr, bits)
        assert out.dtype == dtype and out.shape == cur.shape
        assert np.array_equal(out[keep::2], cur[keep::2])


def _scalar(cur, prev, keep, weave, threshold, bits):
    """the contract, sample by sample in Python integers"""
    H, W = cur.shape
    c = [[int(v) for v in row] for row in cur]
    p = None if prev is None else [[int(v) for v in row] for row in prev]
    T = threshold << (bits - 8)
    cl = lambda x: min(max(x, 0), W - 1)
    out = [row[:] for row in c]
    for y in range(1 - keep, H, 2):
        ya = y - 1 if y - 1 >= 0 else y + 1
        yb = y + 1 if y + 1 < H else y - 1
        A, B = c[ya], c[yb]
        for x in range(W):
            best = sp = None
            for d in (0, -1, 1):
                score = sum(abs(A[cl(x + j + d)] - B[cl(x + j - d)]) for j in (-1, 0, 1))
                if best is None or score < best:
                    best, sp = score, (A[cl(x + d)] + B[cl(x - d)] + 1) >> 1
            if p is None or T == 0:
                out[y][x] = sp
                continue
            m = max(abs(c[r][cl(x + j)] - p[r][cl(x + j)]) for r in (ya, y, yb) for j in (-1, 0, 1))
            k = (256 * max(0, T - m)) // T
            wv = p[y][x] if weave else c[y][x]
            out[y][x] = sp + ((k * (wv - sp) + 128) >> 8)
    return np.array(out, dtype=cur.dtype)


@pytest.mark.parametrize("bits,dtype", KINDS)
@pytest.mark.parametrize("shape", [(2, 1), (2, 5), (3, 4), (5, 1), (8, 11)])
def test_the_vectorised_restatement_is_the_scalar_contract(bits, dtype, shape):
    cur = (_random(bits, dtype, shape, 4) >> (bits - 4) << (bits - 4)).astype(dtype)      # 16 levels: many score ties
    for keep in (0, 1):
        for weave in (0, 1):
            for thr in (0, 1, 10, 64):
                for prev in (None, _near(cur, bits, 5), _random(bits, dtype, shape, 6)):
                    got = dnp.deinterlace_plane(cur, prev, keep, weave, thr, bits)
                    assert np.array_equal(got, _scalar(cur, prev, keep, weave, thr, bits)), (keep, weave, thr)


@pytest.mark.parametrize("bits,dtype", KINDS)
@pytest.mark.parametrize("pattern", ["random", "comb", "near"])
def test_outputs_lie_between_the_samples_they_read(bits, dtype, pattern):
    mx = (1 << bits) - 1
    H, W = 14, 19
    if pattern == "random":
        cur, prev = _random(bits, dtype, (H, W), 7), _random(bits, dtype, (H, W), 8)
    elif pattern == "comb":
        cur = np.zeros((H, W), dtype)
        cur[1::2] = mx
        prev = (mx - cur).astype(dtype)
    else:
        cur = _random(bits, dtype, (H, W), 9)
        prev = _near(cur, bits, 10)
    for keep in (0, 1):
        for weave in (0, 1):
            for thr in (0, 1, 10, 64):
                out = dnp.deinterlace_plane(cur, prev, keep, weave, thr, bits).astype(np.int64)
                assert out.max() <= mx and out.min() >= 0
                for y in range(1 - keep, H, 2):
                    ya, yb = dnp.neighbour_rows(y, H)
                    wv = (prev if weave else cur)[y].astype(np.int64)
                    rows = [dnp._cols(cur[r].astype(np.int64), s) for r in (ya, yb) for s in (-1, 0, 1)] + ([wv] if thr > 0 else [])
                    assert (out[y] >= np.minimum.reduce(rows)).all() and (out[y] <= np.maximum.reduce(rows)).all()


@pytest.mark.parametrize("bits,dtype", KINDS)
def test_threshold_0_ignores_prev(bits, dtype):
    cur = _random(bits, dtype, (10, 13), 11)
    for keep in (0, 1):
        want = dnp.deinterlace_plane(cur, None, keep, 0, 10, bits)
        for prev in (cur, _near(cur, bits, 12), _random(bits, dtype, (10, 13), 13)):
            for weave in (0, 1):
                assert np.array_equal(dnp.deinterlace_plane(cur, prev, keep, weave, 0, bits), want)


def test_nothing_moved_means_the_woven_sample():
    cur = _random(8, np.uint8, (10, 13), 14)
    for keep in (0, 1):
        assert np.array_equal(dnp.deinterlace_plane(cur, cur, keep, 0, 1, 8), cur)
        assert np.array_equal(dnp.deinterlace_plane(cur, cur, keep, 1, 64, 8), cur)


def _middle(A, B):
    cur = np.array([A, [0] * len(A), B], np.uint8)
    return int(dnp.deinterlace_plane(cur, None, 0, 0, 0, 8)[1, 2])


def test_the_tie_order_of_the_three_directions():
    # every direction scores 10: d = 0 stays (pred 15; d = -1 would give 10)
    assert _middle([10, 10, 10, 10, 10], [10, 10, 20, 10, 10]) == 15
    # d = -1 and d = +1 both score 50, d = 0 scores 100: the earlier of the two, d = -1 (pred 65; d = +1 would give 85)
    assert _middle([50, 40, 50, 60, 50], [50, 110, 50, 90, 50]) == 65
    # a diagonal: A[i] = B[i + 2], so d = -1 matches exactly (A[x - 1] = B[x + 1]) ...
    p = [3, 97, 41, 200, 12, 150, 77, 30, 251]
    A, B = p[2:7], p[0:5]
    assert _middle(A, B) == A[1] == B[3]
    # ... and the other way round, d = +1 (A[x + 1] = B[x - 1])
    assert _middle(B, A) == B[3] == A[1]
    _, which = dnp.spatial_row(np.array(p[2:], np.int32), np.array(p[:-2], np.int32))
    assert which[2] == -1 and set(np.unique(which)) <= {0, -1, 1}
    _, which = dnp.spatial_row(np.array(p[:-2], np.int32), np.array(p[2:], np.int32))
    assert which[2] == 1


@pytest.mark.parametrize("H", [2, 3, 4, 5, 9, 10])
def test_the_rows_above_and_below_at_the_top_and_the_bottom(H):
    assert dnp.neighbour_rows(0, H) == (1, 1)
    assert dnp.neighbour_rows(H - 1, H) == ((H - 2, H - 2) if H > 1 else None)
    if H > 2:
        assert dnp.neighbour_rows(1, H) == (0, 2)
    cur = _random(8, np.uint8, (H, 6), 15 + H)
    top = dnp.deinterlace_plane(cur, None, 1, 0, 10, 8)          # row 0 is missing: both neighbours are row 1
    assert np.array_equal(top[0], cur[1])
    keep = H % 2                                                   # the last row is missing: both neighbours are row H - 2
    bottom = dnp.deinterlace_plane(cur, None, keep, 0, 10, 8)
    assert np.array_equal(bottom[H - 1], cur[H - 2])
    with pytest.raises(ValueError):
        dnp.deinterlace_plane(cur[:1], None, 0, 0, 10, 8)


def _flip_clip(bits, dtype):
    frames = [_random(bits, dtype, (12, 17), 20)]
    return frames + [_near(frames[0], bits, 21), _near(frames[0], bits, 22)]


@pytest.mark.parametrize("mode", ["frame", "field"])
@pytest.mark.parametrize("bits,dtype", [(8, np.uint8), (10, np.uint16)])
def test_bff_is_tff_on_the_clip_with_its_rows_flipped(mode, bits, dtype):
    # Flipping the rows swaps A and B, and with them the directions -1 and +1. Where those two tie below d = 0 the order of the
    # contract (-1 first) picks the other one of the pair, so there - and only there - the two clips may differ.
    frames = _flip_clip(bits, dtype)
    bff = dnp.deinterlace_clip(frames, mode, "bff", 10, bits)
    tff = dnp.deinterlace_clip([f[::-1] for f in frames], mode, "tff", 10, bits)
    assert len(bff) == len(frames) * (2 if mode == "field" else 1)
    params = dnp.picture_params(mode, "bff")
    ties = 0
    for i, (a, b) in enumerate(zip(bff, tff)):
        f, keep = frames[i // len(params)].astype(np.int32), params[i % len(params)][0]
        same = np.ones(a.shape, bool)
        for y in range(1 - keep, a.shape[0], 2):
            ya, yb = dnp.neighbour_rows(y, a.shape[0])
            s0, sm, sp = dnp.scores_row(f[ya], f[yb])
            same[y] = ~((sm == sp) & (sm < s0))
        ties += int((~same).sum())
        assert np.array_equal(a[same], b[::-1][same])
    assert ties < a.size // 10                                     # the exception is rare


@pytest.mark.parametrize("mode", ["frame", "field"])
@pytest.mark.parametrize("bits,dtype", [(8, np.uint8), (10, np.uint16)])
def test_bff_is_tff_on_the_clip_turned_by_180_degrees(mode, bits, dtype):
    # with the columns flipped as well the directions map onto themselves: equal everywhere
    frames = _flip_clip(bits, dtype)
    bff = dnp.deinterlace_clip(frames, mode, "bff", 10, bits)
    tff = dnp.deinterlace_clip([f[::-1, ::-1] for f in frames], mode, "tff", 10, bits)
    for a, b in zip(bff, tff):
        assert np.array_equal(a, b[::-1, ::-1])


def test_the_picture_mapping():
    assert dnp.picture_params("frame", "tff") == [(0, 0)] and dnp.picture_params("frame", "bff") == [(1, 0)]
    assert dnp.picture_params("field", "tff") == [(0, 1), (1, 0)] and dnp.picture_params("field", "bff") == [(1, 1), (0, 0)]
    frames = [(_random(8, np.uint8, (8, 6), 30 + i), _random(8, np.uint8, (4, 3), 40 + i)) for i in range(3)]
    out = dnp.deinterlace_clip(frames, "field", "tff", 10, 8)
    assert len(out) == 6 and all(isinstance(p, tuple) and len(p) == 2 for p in out)
    for i, plane in enumerate(frames[1]):                          # picture 2: frame 1's top field, woven with frame 0
        assert np.array_equal(out[2][i], dnp.deinterlace_plane(plane, frames[0][i], 0, 1, 10, 8))
        assert np.array_equal(out[3][i], dnp.deinterlace_plane(plane, frames[0][i], 1, 0, 10, 8))
        assert np.array_equal(out[0][i], dnp.deinterlace_plane(frames[0][i], None, 0, 1, 10, 8))


# ------------------------------------------------------------------------------------ the three claims
SH, SW, FRAMES = 48, 64, 4


def _truth(n, speed, bits):
    """the progressive scene at field time n"""
    y, x = np.mgrid[0:SH, 0:SW]
    x = x + speed * n
    v = 128 + 60 * np.sin(x / 9) * np.cos(y / 7) + 40 * ((x // 16 + y // 16) % 2) - 20 + 30 * np.sin((x + y) / 3)
    return np.clip(np.round(v * (1 << (bits - 8))), 0, (1 << bits) - 1)


def _weave(top, bottom, dtype):
    f = np.empty((SH, SW), dtype)
    f[0::2], f[1::2] = top[0::2], bottom[1::2]
    return f


def _scene(speed, bits, sigma=0.0, seed=0):
    """top field first: frame f holds the even rows of field time 2 f and the odd rows of field time 2 f + 1
    -> (the woven frames, the truth at every field time)"""
    dtype = np.uint8 if bits == 8 else np.uint16
    rng = np.random.default_rng(seed)
    truth = [_truth(n, speed, bits) for n in range(2 * FRAMES)]
    seen = [np.clip(np.round(t + rng.normal(0, sigma * (1 << (bits - 8)), t.shape)), 0, (1 << bits) - 1) if sigma else t for t in truth]
    return [_weave(seen[2 * f], seen[2 * f + 1], dtype) for f in range(FRAMES)], truth


def _psnr(a, b, bits):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(((1 << bits) - 1) ** 2 / mse)


def _pictures(mode):
    """(the index of an output picture, its source frame, its field time) for frames 1 .. 3"""
    if mode == "frame":
        return [(f, f, 2 * f) for f in range(1, FRAMES)]
    return [(n, n // 2, n) for n in range(2, 2 * FRAMES)]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("mode", ["frame", "field"])
def test_a_static_scene_is_rewoven_bit_for_bit(mode, bits):
    frames, truth = _scene(0, bits)
    out = dnp.deinterlace_clip(frames, mode, "tff", 6, bits)
    for i, _, n in _pictures(mode):
        assert np.array_equal(out[i], truth[n])
    assert not np.array_equal(out[0], truth[0])                   # the first frame has no history: spatial only


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("mode", ["frame", "field"])
def test_a_pan_is_8_db_above_the_woven_frame(mode, bits):
    frames, truth = _scene(3, bits)
    out = dnp.deinterlace_clip(frames, mode, "tff", 10, bits)
    for i, f, n in _pictures(mode):
        got, woven = _psnr(out[i], truth[n], bits), _psnr(frames[f], truth[n], bits)
        print("pan %s %d bits, picture %d: %.2f dB, woven %.2f dB" % (mode, bits, i, got, woven))
        assert got >= woven + 8


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("mode", ["frame", "field"])
def test_noise_on_a_static_scene_is_3_db_above_spatial_only(mode, bits):
    frames, truth = _scene(0, bits, sigma=2.0, seed=27)
    out = dnp.deinterlace_clip(frames, mode, "tff", 10, bits)
    bob = dnp.deinterlace_clip(frames, mode, "tff", 0, bits)
    for i, _, n in _pictures(mode):
        got, spatial = _psnr(out[i], truth[n], bits), _psnr(bob[i], truth[n], bits)
        print("noise %s %d bits, picture %d: %.2f dB, spatial only %.2f dB" % (mode, bits, i, got, spatial))
        assert got >= spatial + 3
