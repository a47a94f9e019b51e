"""The block motion search and the motion-compensated denoiser of DESIGN.md 31 without a GPU: the properties of the numpy
restatement (tests/motion_np.py) - the claim on a panning noisy scene, the static scene, exact recovery of a translation, and the
tie order."""
import numpy as np
import pytest

import denoise_np
import motion_np


def _psnr(a, ref, peak):
    mse = float(((a.astype(np.float64) - ref) ** 2).mean())
    return 10 * np.log10(peak * peak / mse)


def _scene(bits, pan, n=6):
    """the scene of test_denoise_cpu.py, 96x128, moving `pan` samples a picture, plus noise of sigma 3 at 8 bits"""
    Hh, Ww = 96, 128
    s = 1 << (bits - 8)
    peak = float((1 << bits) - 1)
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:Hh, 0:Ww + pan * n]
    wide = (128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)) * s
    clean = [wide[:, pan * i:pan * i + Ww] for i in range(n)]
    dtype = np.uint8 if bits == 8 else np.uint16
    noisy = [np.clip(np.rint(c + rng.normal(0, 3 * s, c.shape)), 0, peak).astype(dtype) for c in clean]
    return clean, noisy, peak


def _mc_clip(noisy, bits, R=7, lam=4):
    out, mvs = motion_np.mc_denoise_clip([(p,) for p in noisy], 8, 8, bits, R, lam)
    return [o[0] for o in out], mvs


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("pan", [3, 8, 13])
def test_compensation_beats_the_plain_filter_on_a_pan(bits, pan):
    """sixth picture, strengths 8:8, R 7, lambda 4, PSNR against the clean picture. Measured with this restatement
    (plain -> compensated; the noisy input is at 38.5 to 38.6 dB): 8 bits, pan 3 / 8 / 13: 39.77 -> 43.37, 39.56 -> 42.84,
    39.44 -> 42.82 dB; 10 bits: 39.92 -> 43.68, 39.70 -> 43.14, 39.58 -> 43.09 dB. The smallest margin is 3.28 dB; 2 dB, about
    two thirds of it, is asked for."""
    clean, noisy, peak = _scene(bits, pan)
    plain = denoise_np.denoise_clip([(p,) for p in noisy], 8, 8, bits)[5][0]
    mc = _mc_clip(noisy, bits)[0][5]
    a, b = _psnr(plain, clean[5], peak), _psnr(mc, clean[5], peak)
    print(bits, pan, round(_psnr(noisy[5], clean[5], peak), 2), round(a, 2), round(b, 2))
    assert b >= a + 2.0, (a, b)


@pytest.mark.parametrize("bits", [8, 10])
def test_a_static_scene_has_zero_vectors_and_the_plain_output(bits):
    clean, noisy, peak = _scene(bits, 0, n=4)
    plain = [o[0] for o in denoise_np.denoise_clip([(p,) for p in noisy], 8, 8, bits)]
    out, mvs = _mc_clip(noisy, bits)
    assert mvs[0] is None
    for found in mvs[1:]:
        assert not found[0].any()
    for a, b in zip(plain, out):
        assert np.array_equal(a, b)


def _texture(H, W, bits, seed=5):
    """a random texture with features of about 4 samples, so that it survives the half-resolution stage: full-range random
    cells of 4 x 4 samples under a 4 x 4 box filter, in integers"""
    cells = np.random.default_rng(seed).integers(0, 1 << bits, (H // 4 + 2, W // 4 + 2)).astype(np.int64)
    a = np.kron(cells, np.ones((4, 4), np.int64))
    c = np.pad(a, ((1, 0), (1, 0))).cumsum(0).cumsum(1)
    box = c[4:, 4:] - c[:-4, 4:] - c[4:, :-4] + c[:-4, :-4]
    return (box >> 4)[:H, :W]


@pytest.mark.parametrize("bits,dtype", [(8, np.uint8), (10, np.uint16), (16, np.uint16)])
@pytest.mark.parametrize("shift,R", [((1, 0), 7), ((0, -1), 7), ((5, -3), 7), ((14, 14), 7), ((-30, 30), 15)])
def test_a_translation_is_found_exactly(shift, R, bits, dtype):
    """cur[y][x] = ref[y + dy][x + dx] of a noise-free random texture: every block whose window stays inside the plane gets
    exactly (dx, dy)"""
    dx, dy = shift
    H, W, M = 112, 144, 32
    big = _texture(H + 2 * M, W + 2 * M, bits).astype(dtype)
    ref = big[M:M + H, M:M + W]
    cur = big[M + dy:M + dy + H, M + dx:M + dx + W]
    mv, sad = motion_np.motion_search(cur, ref, bits, R, 4)
    Bh, Bw = motion_np.grid(H, W)
    assert mv.shape == (Bh, Bw, 2) and mv.dtype == np.int16 and sad.shape == (Bh, Bw) and sad.dtype == np.uint32
    checked = 0
    for by in range(Bh):
        for bx in range(Bw):
            # the level-1 window reaches 2 R + 1 full-resolution samples around the block, the level-0 one 2 R + 1 as well
            if by * 16 - (2 * R + 2) >= 0 and by * 16 + 16 + 2 * R + 2 <= H and bx * 16 - (2 * R + 2) >= 0 and bx * 16 + 16 + 2 * R + 2 <= W:
                assert tuple(mv[by, bx]) == (dx, dy), (by, bx, mv[by, bx])
                assert sad[by, bx] == 0
                checked += 1
    assert checked >= 4
    assert np.abs(mv).max() <= 2 * R + 1
    # compensating ref with the vectors gives cur in those blocks
    comp = motion_np.compensate_plane(ref, mv)
    assert comp.dtype == dtype and np.array_equal(comp[48:64, 48:80], cur[48:64, 48:80])


@pytest.mark.parametrize("bits,dtype", [(8, np.uint8), (10, np.uint16)])
@pytest.mark.parametrize("pattern", ["constant", "period 4"])
def test_ties_go_to_the_zero_vector(pattern, bits, dtype):
    """lambda 0: every candidate of a constant plane ties at cost 0, and so does every multiple of the period of a periodic
    one; the order (cost, |dx| + |dy|, dy, dx) gives (0, 0)"""
    H, W = 50, 70
    yy, xx = np.mgrid[0:H, 0:W]
    s = 1 << (bits - 8)
    a = np.full((H, W), 77 * s, dtype) if pattern == "constant" else ((((xx & 3) * 40) + ((yy & 3) * 10) + 16) * s).astype(dtype)
    for R in (0, 3, 7):
        mv, sad = motion_np.motion_search(a, a, bits, R, 0)
        assert not mv.any() and not sad.any()


def test_the_order_prefers_short_then_small_dy_then_small_dx():
    # a constant plane with penalty 0 ties everywhere: the key alone decides. The packed key must order as the tuple does
    c = np.zeros((), np.int64)
    k = lambda cost, dy, dx: int(motion_np._key(c + cost, c + dy, c + dx))
    assert k(0, 0, 0) < k(0, 0, -1) < k(0, 0, 1)                 # shorter first, then dx
    assert k(0, -1, 0) < k(0, 0, -1)                              # equal length: the smaller dy first
    assert k(0, -31, 31) < k(1, 0, 0)                             # the cost first
    assert k(5, 1, -1) < k(5, 1, 1) < k(5, 2, -31)


def test_half_resolution_and_partial_blocks():
    a = np.arange(15, dtype=np.int64).reshape(3, 5) * 10
    h = motion_np.half_plane(a)
    assert h.shape == (2, 3)
    assert h[0, 0] == (0 + 10 + 50 + 60 + 2) >> 2 and h[1, 2] == 140 and h[0, 2] == (40 + 40 + 90 + 90 + 2) >> 2
    # 17 x 33: the second block row has one luma row, the third block column one luma column
    rng = np.random.default_rng(2)
    cur, ref = rng.integers(0, 256, (17, 33)), rng.integers(0, 256, (17, 33))
    mv, sad = motion_np.motion_search(cur, ref, 8, 2, 0)
    assert mv.shape == (2, 3, 2)
    dx, dy = (int(v) for v in mv[1, 2])
    assert sad[1, 2] == abs(int(cur[16, 32]) - int(ref[np.clip(16 + dy, 0, 16), np.clip(32 + dx, 0, 32)]))


def test_compensation_floors_the_chroma_vector_and_clamps():
    prev = np.arange(8 * 8, dtype=np.uint16).reshape(8, 8)
    mv = np.array([[[-3, -1]]], np.int16)
    got = motion_np.compensate_plane(prev, mv, 1, 1)             # (-3 >> 1, -1 >> 1) = (-2, -1)
    yy, xx = np.mgrid[0:8, 0:8]
    assert np.array_equal(got, prev[np.clip(yy - 1, 0, 7), np.clip(xx - 2, 0, 7)])
    far = motion_np.compensate_plane(prev, np.array([[[32767, -32767]]], np.int16), 0, 0)
    assert (far == prev[0, 7]).all()
    assert np.array_equal(motion_np.compensate_plane(prev, np.zeros((1, 1, 2), np.int16), 1, 0), prev)
