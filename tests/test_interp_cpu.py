"""The frame-rate conversion of DESIGN.md 32 without a GPU: the properties of the numpy restatement (tests/interp_np.py) - the
split, the static pair, the claim on pans against the plain blend, the two fallbacks on an unrelated pair, and the key's order."""
import itertools

import numpy as np
import pytest

import interp_np
import motion_np

H, W = 96, 128


def _texture(yy, xx):
    """the scene of test_motion_cpu.py, a smooth texture over a 16x16 checkerboard, in 0..1"""
    return 0.5 + 0.235 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 0.157 * (((xx // 16).astype(np.int64) + (yy // 16).astype(np.int64)) & 1)


def _picture(bits, t, pan, rng):
    """the scene after t output pictures of a pan of `pan` = (dx, dy) samples an output picture, with noise of sigma 2 at 8 bits"""
    peak = (1 << bits) - 1
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    clean = _texture(yy + 40 + t * pan[1], xx + 40 + t * pan[0]) * peak
    noisy = clean + rng.normal(0, 2.0 * (1 << (bits - 8)), clean.shape)
    return np.clip(np.rint(noisy), 0, peak).astype(np.uint8 if bits == 8 else np.uint16)


def _pan_case(bits, pan, N):
    """-> per phase (compensated, blend, repeat) luma PSNR against the true in-between picture"""
    rng = np.random.default_rng(1000 * bits + 100 * N + 10 * pan[0] + pan[1])
    A, B = _picture(bits, 0, pan, rng), _picture(bits, N, pan, rng)
    # B[p] = scene(p + N pan) = A[p + N pan]: the search of B against A finds v = N pan, inside its reach of 2 R + 1 = 15
    mids = interp_np.interpolate((A,), (B,), bits, N)
    rows = []
    for k, mid in zip(range(1, N), mids):
        true = _picture(bits, k, pan, rng)
        blend = ((N - k) * A.astype(np.int64) + k * B.astype(np.int64) + (N >> 1)) // N
        rows.append((interp_np.psnr(mid[0], true, bits), interp_np.psnr(blend, true, bits), interp_np.psnr(A if 2 * k <= N else B, true, bits)))
    return rows


def test_the_split():
    for N in range(2, 9):
        for k in range(1, N):
            for v in range(-31, 32):
                a, b = interp_np.split(v, k, N)
                assert a - b == v
                assert a == np.floor(k * v / N + 0.5), (v, k, N)          # k v / N is exact in a double here: N <= 8
    a, b = interp_np.split(np.array([-31, -1, 0, 1, 31]), 1, 2)
    assert a.tolist() == [-15, 0, 0, 1, 16] and b.tolist() == [16, 1, 0, 0, -15]


@pytest.mark.parametrize("bits", [8, 10])
def test_a_static_pair_returns_a(bits):
    rng = np.random.default_rng(3)
    A = _picture(bits, 0, (0, 0), rng)
    for N in (2, 3, 8):
        for mid in interp_np.interpolate((A, A[::2, ::2], A[1::2, 1::2]), (A, A[::2, ::2], A[1::2, 1::2]), bits, N):
            assert np.array_equal(mid[0], A) and np.array_equal(mid[1], A[::2, ::2]) and np.array_equal(mid[2], A[1::2, 1::2])
            assert mid[0].dtype == A.dtype


PANS = [(2, (2, 0)), (2, (4, 2)), (2, (3, -1)), (2, (6, 6)), (3, (2, 0)), (3, (4, 2)), (3, (3, -1))]
# measured with this restatement on this scene: the smallest margin of the compensated picture over the plain blend
MEASURED_SMALLEST_MARGIN_DB = 4.79
ASKED_DB = max(MEASURED_SMALLEST_MARGIN_DB - 3.0, 3.0)


def test_pans_beat_the_plain_blend():
    """R 7, lambda 4, LIMIT 8; luma PSNR against the true in-between picture, every phase of every pan at 8 and 10 bits; a pan is
    in samples an output picture, so B lies N pans from A, inside the search's reach of 2 R + 1 = 15. Measured with this
    restatement (compensated / plain blend / repeat of the nearer picture, dB; the phases of N = 3 differ by less than 0.3 dB
    except where noted):
      8 bits   N 2: (2,0) 40.1 / 27.9 / 24.0   (4,2) 28.3 / 22.9 / 19.3   (3,-1) 39.8 / 24.8 / 21.2   (6,6) 22.8 / 18.0 / 15.9
               N 3: (2,0) 39.8, 39.6 / 26.6 / 24.0   (4,2) 28.2 / 21.0 / 19.3   (3,-1) 30.0, 31.9 / 23.4 / 21.2
      10 bits  N 2: (2,0) 40.2 / 27.9 / 24.0   (4,2) 28.2 / 22.9 / 19.3   (3,-1) 39.8 / 24.8 / 21.2   (6,6) 22.9 / 18.0 / 16.0
               N 3: (2,0) 39.9 / 26.6 / 24.0   (4,2) 28.2 / 21.0 / 19.3   (3,-1) 30.0, 33.6 / 23.4 / 21.2
    The smallest margin over the blend is 4.79 dB, at (6,6), N 2, 8 bits: there B lies (12, 12) from A and the blocks along two
    sides of this 6 x 8 block picture see samples that one of the pictures does not hold. That margin minus 3 dB is below 3 dB,
    so 3 dB is asked for."""
    margins = []
    for bits in (8, 10):
        for N, pan in PANS:
            for k, (mc, blend, rep) in enumerate(_pan_case(bits, pan, N), 1):
                print("bits %2d N %d pan %-8s k %d: compensated %.2f blend %.2f repeat %.2f dB" % (bits, N, pan, k, mc, blend, rep))
                margins.append(mc - blend)
    print("smallest margin %.2f dB" % min(margins))
    assert min(margins) >= ASKED_DB, min(margins)


def _unrelated(bits):
    """a picture, and an inverted, shifted other texture that shows the first picture again in its top left 32 x 48 samples: there
    the blocks agree, everywhere else they cannot"""
    rng = np.random.default_rng(17)
    peak = (1 << bits) - 1
    A = _picture(bits, 0, (0, 0), rng)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    other = 0.5 + 0.3 * np.sin((xx + 31) / 4.1 + (yy + 11) / 6.3) * np.cos((yy + 5) / 3.3)
    B = np.clip(np.rint((1.0 - other) * peak + rng.normal(0, 2.0 * (1 << (bits - 8)), other.shape)), 0, peak).astype(A.dtype)
    B[:32, :48] = _picture(bits, 0, (0, 0), rng)[:32, :48]
    return A, B


@pytest.mark.parametrize("bits", [8, 10])
def test_an_unrelated_pair_repeats_the_nearer_picture(bits):
    A, B = _unrelated(bits)
    a, b = (A, A[::2, ::2], A[1::2, ::2]), (B, B[::2, ::2], B[1::2, ::2])
    mv, _ = motion_np.motion_search(B, A, bits)
    for N in (2, 3, 8):
        for k in range(1, N):
            plan, wb, sad, fallen = interp_np.interp_select(A, B, mv, bits, k, N)
            assert 2 * fallen > wb.size, (fallen, wb.size)       # the picture rule applies: more than half of the 48 blocks
            assert fallen < wb.size                               # ... but not every block fell, so the rule decides
            mid, f, _ = interp_np.interp_between(a, b, mv, bits, k, N)
            want = a if 2 * k <= N else b
            assert f == fallen and all(np.array_equal(m, w) for m, w in zip(mid, want)), (N, k)


@pytest.mark.parametrize("bits", [8, 10])
def test_without_the_counter_the_pair_repeats_block_by_block(bits):
    A, B = _unrelated(bits)
    mv, _ = motion_np.motion_search(B, A, bits)
    some_kept = False
    for N, k in ((2, 1), (3, 1), (3, 2)):
        plan, wb, sad, fallen = interp_np.interp_select(A, B, mv, bits, k, N, limit=8)
        mid = interp_np.interp_plane(A, B, plan, wb, k, N)
        near = A if 2 * k <= N else B
        fell = np.repeat(np.repeat(wb != k, 16, axis=0), 16, axis=1)
        assert fell.sum() == fallen * 256 and not plan[wb != k].any()
        assert np.array_equal(mid[fell], near[fell])
        some_kept |= bool((~fell).any() and not np.array_equal(mid[~fell], near[~fell]))
        # with limit 0 every block with a difference falls; with 255 none can: a difference is at most the peak
        assert interp_np.interp_select(A, B, mv, bits, k, N, limit=255)[3] == 0
        assert interp_np.interp_select(A, B, mv, bits, k, N, limit=0)[3] == wb.size
    assert some_kept


def test_the_key_orders_as_the_tuple():
    rng = np.random.default_rng(2)
    items = [(int(s), int(vy), int(vx)) for s, vy, vx in zip(rng.integers(0, 4, 300), rng.integers(-31, 32, 300), rng.integers(-31, 32, 300))]
    items += [(256 * 65535, 31, 31), (256 * 65535, -31, -31), (0, 0, 0), (0, -31, 31), (1, 0, 0), (0, 31, -31)]
    tup = lambda it: (it[0], abs(it[2]) + abs(it[1]), it[1], it[2])
    k = lambda it: int(interp_np.key(it[0], it[1], it[2]))
    for p, q in itertools.combinations(items, 2):
        assert (k(p) < k(q)) == (tup(p) < tup(q)) and (k(p) == k(q)) == (tup(p) == tup(q))
    assert k((256 * 65535, 31, 31)) < 2 ** 63
