"""dcvc_interp_select and dcvc_interp_planes on a real MI355X against the numpy restatement (tests/interp_np.py) with ==: u8, 10-bit
and 16-bit full-range samples over sizes with one sample, one block, partial blocks on either axis and several blocks; every
phase of N = 2, 3 and 8; vectors from the search, all-zero and random int16 (the clamp to +-31); limits 0, 8 and 255; strided
inputs; grids wider than needed; sad and fallen given and NULL. The interpolation at all four subsamplings, both store paths,
plane strides, plans of +-32767 and wb = 255, the accumulator's top, the picture rule on both sides of its threshold, guard
samples; the Python interpolate end to end at 352x288."""
import ctypes

import numpy as np
import pytest
import torch

import interp_np
import motion_np
from dcvc_amd import _lib, interp, motion

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (16, 16), (17, 33), (50, 70), (96, 128)]
KINDS = [("u8", np.uint8, 8), ("u10", np.uint16, 10), ("u16", np.uint16, 16)]
PHASES = [(k, n) for n in (2, 3, 8) for k in range(1, n)]
vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


def _dev(a):
    """numpy u8 / u16 / int16 -> CUDA tensor (16-bit samples as int16 storage, which every torch has)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _host(t, dtype):
    if dtype == np.uint8:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _pair(H, W, dtype, bits, seed):
    """(A, B): a smooth texture moved by (6, -4) samples plus noise and full-range outliers; the right third of B is another
    texture, so blocks there fall back at limit 8 while the rest agree"""
    rng = np.random.default_rng(seed)
    m = (1 << bits) - 1
    yy, xx = np.mgrid[0:H + 16, 0:W + 16]
    base = (0.5 + 0.3 * np.sin(xx / 3.1) * np.cos(yy / 2.3) + 0.2 * ((xx // 5 + yy // 7) & 1)) * m
    A = base[8:8 + H, 8:8 + W] + rng.normal(0, m / 256.0, (H, W))
    B = base[4:4 + H, 14:14 + W] + rng.normal(0, m / 256.0, (H, W))
    cut = W - W // 3
    B[:, cut:] = (0.5 - 0.4 * np.cos(xx[:H, cut:W] / 1.7 + yy[:H, cut:W] / 2.9)) * m
    for a in (A, B):
        q = rng.random((H, W))
        a[q < 0.002] = 0
        a[q > 0.998] = m
    return np.clip(np.rint(A), 0, m).astype(dtype), np.clip(np.rint(B), 0, m).astype(dtype)


def _select(A, B, mv, bits, k, n, limit):
    fallen = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan, wb, sad = interp.interp_select(_dev(A), _dev(B), _dev(mv), bits, k, n, limit, fallen=fallen)
    return plan.cpu().numpy(), wb.cpu().numpy(), sad.cpu().numpy().view(np.uint32), int(fallen.item())


def _same_select(got, want, what):
    for g, w, name in zip(got, want, ("plan", "wb", "sad", "fallen")):
        assert np.array_equal(g, w), (what, name, np.argwhere(np.asarray(g) != np.asarray(w))[:4].tolist())
    assert got[0].dtype == np.int16 and got[1].dtype == np.uint8


def _mvs(A, B, bits, seed):
    Bh, Bw = motion_np.grid(*A.shape)
    rng = np.random.default_rng(seed)
    wild = rng.integers(-32768, 32768, (Bh, Bw, 2)).astype(np.int16)
    wild.reshape(-1, 2)[::3] = rng.integers(-40, 41, (len(wild.reshape(-1, 2)[::3]), 2))     # some around the clamp, some inside
    return [("search", motion_np.motion_search(B, A, bits, 7, 4)[0]), ("zero", np.zeros((Bh, Bw, 2), np.int16)), ("random", wild)]


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_the_selection_equals_the_numpy_restatement(size, kind):
    H, W = size
    _, dtype, bits = kind
    A, B = _pair(H, W, dtype, bits, seed=H * 100 + W)
    fell = set()
    for name, mv in _mvs(A, B, bits, seed=H + W):
        for k, n in PHASES:
            for limit in (0, 8, 255):
                want = interp_np.interp_select(A, B, mv, bits, k, n, limit)
                _same_select(_select(A, B, mv, bits, k, n, limit), want, (name, k, n, limit))
                fell.add(0 < want[3] < want[1].size)
    if H * W >= 50 * 70:
        assert True in fell                     # a case where some blocks fell and some did not was among them


def test_the_search_finds_the_pan_and_the_selection_splits_it():
    """the content of this pair moves by (6, -4): inside the agreeing part the plan is the split of (6, -4) ... as the search
    names it, B[p] ~ A[p + v]"""
    A, B = _pair(96, 128, np.uint8, 8, seed=1)
    mv = motion_np.motion_search(B, A, 8, 7, 4)[0]
    assert tuple(mv[2, 2]) == (6, -4)
    plan, wb, sad, fallen = _select(A, B, mv, 8, 1, 2, 8)
    assert tuple(plan[2, 2]) == (3, -2, -3, 2) and wb[2, 2] == 1 and 0 < fallen < 48
    plan, wb, _, _ = _select(A, B, mv, 8, 1, 3, 8)
    assert tuple(plan[2, 2]) == (2, -1, -4, 3) and wb[2, 2] == 1


def test_full_range_16_bit_extremes():
    """an all-0 plane against an all-65535 one: every candidate has the largest SAD, 256 * 65535; at limit 255 it still falls"""
    A, B = np.zeros((33, 47), np.uint16), np.full((33, 47), 65535, np.uint16)
    mv = np.full((3, 3, 2), 31, np.int16)
    for limit in (0, 255):
        want = interp_np.interp_select(A, B, mv, 16, 3, 8, limit)
        assert want[2].max() == 256 * 65535 and want[3] == 9
        _same_select(_select(A, B, mv, 16, 3, 8, limit), want, limit)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_strided_rows_larger_grids_and_optional_outputs(kind):
    _, dtype, bits = kind
    H, W = 50, 70
    A, B = _pair(H, W, dtype, bits, seed=11)
    Bh, Bw = motion_np.grid(H, W)
    mv = motion_np.motion_search(B, A, bits, 7, 4)[0]
    want = interp_np.interp_select(A, B, mv, bits, 2, 3, 8)
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5
    af, bf = np.full((H, W + 7), guard, dtype), np.full((H + 1, W + 13), guard, dtype)
    af[:, :W], bf[:H, :W] = A, B
    ta, tb = _dev(af), _dev(bf)
    # the wrapper on strided views
    fallen = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan, wb, sad = interp.interp_select(ta[:, :W], tb[:H, :W], _dev(mv), bits, 2, 3, fallen=fallen)
    _same_select((plan.cpu().numpy(), wb.cpu().numpy(), sad.cpu().numpy().view(np.uint32), int(fallen.item())), want, "strided")
    # the C call: an mv grid and a plan grid wider than needed, whose rest is left alone; sad and fallen given and NULL
    f = _lib.fn("dcvc_interp_select", ci, [vp, ci, vp, ci, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp])
    big_mv = np.full((Bh + 2, Bw + 3, 2), 77, np.int16)
    big_mv[:Bh, :Bw] = mv
    tm = _dev(big_mv)
    tplan = torch.full((Bh + 1, Bw + 2, 4), 999, dtype=torch.int16, device="cuda")
    twb = torch.full((Bh + 1, Bw + 2), 200, dtype=torch.uint8, device="cuda")
    tsad = torch.full((Bh + 1, Bw + 2), -5, dtype=torch.int32, device="cuda")
    tf = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    code = 0 if dtype == np.uint8 else 3
    for with_sad, with_fallen in ((True, True), (False, True), (True, False), (False, False)):
        _lib.check(f(vp(ta.data_ptr()), W + 7, vp(tb.data_ptr()), W + 13, code, bits, H, W, vp(tm.data_ptr()), Bh + 2, Bw + 3, 2, 3, 8,
                     vp(tplan.data_ptr()), vp(twb.data_ptr()), Bh + 1, Bw + 2, vp(tsad.data_ptr()) if with_sad else None,
                     vp(tf.data_ptr()) if with_fallen else None, st))
    gp, gw, gs = tplan.cpu().numpy(), twb.cpu().numpy(), tsad.cpu().numpy()
    assert np.array_equal(gp[:Bh, :Bw], want[0]) and np.array_equal(gw[:Bh, :Bw], want[1]) and np.array_equal(gs[:Bh, :Bw].view(np.uint32), want[2])
    assert (gp[Bh:] == 999).all() and (gp[:, Bw:] == 999).all() and (gw[Bh:] == 200).all() and (gw[:, Bw:] == 200).all()
    assert (gs[Bh:] == -5).all() and (gs[:, Bw:] == -5).all()
    assert int(tf.item()) == 2 * want[3] and want[3] > 0                 # two of the four calls count
    assert np.array_equal(_host(ta, dtype), af) and np.array_equal(_host(tb, dtype), bf)


# ------------------------------------------------------------------------------------ interpolation
def _plans(bh, bw, n, seed):
    """ordinary offsets, negative odd ones, +-32767, and weights 0..n, above n and 255"""
    rng = np.random.default_rng(seed)
    plan = rng.integers(-31, 32, (bh, bw, 4)).astype(np.int16)
    wb = rng.integers(0, n + 1, (bh, bw)).astype(np.uint8)
    fp, fw = plan.reshape(-1, 4), wb.reshape(-1)
    special = [((-1, -1, 1, 1), 1), ((-3, 5, 7, -9), n), ((32767, -32767, -32767, 32767), 1), ((-32767, 32767, 32767, -32767), 255),
               ((0, 0, 0, 0), 0), ((1, -32767, -31, 31), n + 1), ((0, 0, 0, 0), 255)]
    for i, (p, w) in enumerate(special):
        fp[(i * 5) % len(fp)] = p
        fw[(i * 5) % len(fw)] = w
    return plan, wb


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("sub", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["444", "422", "440", "420"])
@pytest.mark.parametrize("size", SIZES + [(40, 130), (33, 260)], ids=lambda s: "%dx%d" % s)
def test_interpolation_equals_the_numpy_restatement(size, sub, kind):
    H, W = size
    sx, sy = sub
    _, dtype, bits = kind
    bh, bw = -(-H // (16 >> sy)), -(-W // (16 >> sx))
    rng = np.random.default_rng(H + W)
    A = rng.integers(0, 1 << bits, (2, H, W)).astype(dtype)
    B = rng.integers(0, 1 << bits, (2, H, W)).astype(dtype)
    ta, tb = _dev(A), _dev(B)
    for k, n in [(1, 2), (2, 3), (1, 8), (7, 8), (3, 5), (5, 6), (4, 7)]:
        plan, wb = _plans(bh, bw, n, seed=3 + n)
        want = np.stack([interp_np.interp_plane(a, b, plan, wb, k, n, sx, sy) for a, b in zip(A, B)])
        tp, tw = _dev(plan), _dev(wb)
        got = _host(interp.interp_planes(ta, tb, tp, tw, k, n, sx, sy), dtype)          # two planes in one call
        assert got.dtype == dtype and np.array_equal(got, want), (k, n)
        one = _host(interp.interp_planes(ta[1], tb[1], tp, tw, k, n, sx, sy), dtype)     # a plane on its own, as a 2-D tensor
        assert np.array_equal(one, want[1])
    zero, wk = torch.zeros_like(tp), torch.full_like(tw, 0)
    assert np.array_equal(_host(interp.interp_planes(ta, tb, zero, wk, 1, 2, sx, sy), dtype), A)       # weight 0 copies a
    assert np.array_equal(_host(interp.interp_planes(ta, tb, zero, wk + 2, 1, 2, sx, sy), dtype), B)   # weight n copies b
    assert np.array_equal(_host(ta, dtype), A) and np.array_equal(_host(tb, dtype), B)


def test_the_top_of_the_accumulator():
    """all-65535 planes at N = 8: (8 - w) 65535 + w 65535 + 4 = 8 * 65535 + 4 for every weight"""
    H, W = 33, 47
    A = np.full((H, W), 65535, np.uint16)
    plan, wb = _plans(3, 3, 8, seed=1)
    for k in range(1, 8):
        got = _host(interp.interp_planes(_dev(A), _dev(A), _dev(plan), _dev(wb), k, 8, 0, 0), np.uint16)
        assert (got == 65535).all()
    lo, hi = np.zeros((H, W), np.uint16), A
    for k in (1, 4, 7):
        w = np.full((3, 3), k, np.uint8)
        got = _host(interp.interp_planes(_dev(lo), _dev(hi), _dev(np.zeros((3, 3, 4), np.int16)), _dev(w), k, 8, 0, 0), np.uint16)
        assert (got == (k * 65535 + 4) // 8).all()


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("how", ["odd", "vector"])
def test_strided_interpolation_leaves_the_guard_samples_alone(how, kind):
    _, dtype, bits = kind
    H, W, sx, sy = 33, 130, 1, 1
    a_row, d_row = (W + 5, W + 3) if how == "odd" else (W + 14, (W + 15) // 16 * 16 + 16)
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5
    rng = np.random.default_rng(9)
    a_full = rng.integers(0, 1 << bits, (2, H + 1, a_row)).astype(dtype)
    b_full = rng.integers(0, 1 << bits, (2, H + 2, a_row + 1)).astype(dtype)
    dst_full = np.full((2, H + 2, d_row), guard, dtype)
    plan, wb = _plans(-(-H // 8), -(-W // 8), 3, seed=4)
    want = np.stack([interp_np.interp_plane(a[:H, :W], b[:H, :W], plan, wb, 2, 3, sx, sy) for a, b in zip(a_full, b_full)])
    ta, tb, to = _dev(a_full), _dev(b_full), _dev(dst_full)
    assert interp.interp_planes(ta[:, :H, :W], tb[:, :H, :W], _dev(plan), _dev(wb), 2, 3, sx, sy, out=to[:, :H, :W]).data_ptr() == to.data_ptr()
    got = _host(to, dtype)
    assert np.array_equal(got[:, :H, :W], want)
    mask = np.ones(dst_full.shape, bool)
    mask[:, :H, :W] = False
    assert (got[mask] == guard).all(), "samples outside the destination planes were written"
    # a destination one sample off a 16-byte boundary takes the sample-by-sample stores
    flat = _dev(np.full(H * W + 32, guard, dtype))
    view = flat[1:1 + H * W].view(H, W)
    assert view.data_ptr() % 16 == np.dtype(dtype).itemsize
    interp.interp_planes(ta[0, :H, :W], tb[0, :H, :W], _dev(plan), _dev(wb), 2, 3, sx, sy, out=view)
    gf = _host(flat, dtype)
    assert np.array_equal(gf[1:1 + H * W].reshape(H, W), want[0]) and gf[0] == guard and (gf[1 + H * W:] == guard).all()


def test_the_picture_rule_on_both_sides_of_its_threshold():
    H, W = 50, 70                                   # 4 x 5 = 20 blocks
    rng = np.random.default_rng(5)
    A = rng.integers(0, 256, (H, W)).astype(np.uint8)
    B = rng.integers(0, 256, (H, W)).astype(np.uint8)
    ta, tb = _dev(A), _dev(B)
    for k, n in ((1, 2), (1, 3), (2, 3)):
        plan, wb = _plans(4, 5, n, seed=6)
        tp, tw = _dev(plan), _dev(wb)
        per_block = interp_np.interp_plane(A, B, plan, wb, k, n)
        near = A if 2 * k <= n else B
        assert not np.array_equal(per_block, near)
        for fallen, n_blocks in ((0, 20), (9, 20), (10, 20), (11, 20), (20, 20), (1, 1), (1, 2), (2 ** 31 - 1, 20)):
            tf = torch.tensor([fallen], dtype=torch.int32, device="cuda")
            got = interp.interp_planes(ta, tb, tp, tw, k, n, 0, 0, fallen=tf, n_blocks=n_blocks).cpu().numpy()
            want = interp_np.interp_plane(A, B, plan, wb, k, n, 0, 0, fallen, n_blocks)
            assert np.array_equal(got, want), (k, n, fallen, n_blocks)
            assert np.array_equal(got, near if 2 * fallen > n_blocks else per_block)
            assert int(tf.item()) == fallen          # the counter is only read
        assert np.array_equal(interp.interp_planes(ta, tb, tp, tw, k, n, 0, 0).cpu().numpy(), per_block)     # fallen = NULL


def test_the_c_call_takes_a_larger_grid():
    H, W = 20, 40
    rng = np.random.default_rng(1)
    A, B = rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)
    plan, wb = _plans(4, 6, 2, seed=5)                                       # the plane needs 2 x 3
    f = _lib.fn("dcvc_interp_planes", ci, [vp, ci, cll, vp, ci, cll, vp, ci, cll, ci, ci, ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp, ci, vp])
    ta, tb, tp, tw = _dev(A), _dev(B), _dev(plan), _dev(wb)
    out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    _lib.check(f(vp(ta.data_ptr()), W, 0, vp(tb.data_ptr()), W, 0, vp(out.data_ptr()), W, 0, 0, H, W, 1, 0, 0, vp(tp.data_ptr()), vp(tw.data_ptr()),
                 4, 6, 1, 2, None, 0, vp(torch.cuda.current_stream().cuda_stream)))
    assert np.array_equal(out.cpu().numpy(), interp_np.interp_plane(A, B, plan, wb, 1, 2))


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[1]], ids=["u8", "u10"])
def test_interpolate_end_to_end_at_cif(kind):
    """352x288, 4:2:0: a pan of (5, 3) a picture with a part that does not agree, N = 2 and 3, against the restatement"""
    _, dtype, bits = kind
    A, B = _pair(288, 352, dtype, bits, seed=21)
    a = (A, A[::2, ::2].copy(), (A[1::2, 1::2] ^ 5).copy())
    b = (B, B[::2, ::2].copy(), (B[1::2, 1::2] ^ 5).copy())
    da, db = tuple(_dev(p) for p in a), tuple(_dev(p) for p in b)
    for n in (2, 3):
        want = interp_np.interpolate(a, b, bits, n)
        got = interp.interpolate(da, db, bits, n)
        assert len(got) == n - 1
        for g, w in zip(got, want):
            for gp, wp in zip(g, w):
                assert np.array_equal(_host(gp, dtype), wp), n
    # an unrelated pair: the picture rule repeats a
    C = np.ascontiguousarray(((1 << bits) - 1 - B[::-1, ::-1]))
    c = (C, C[::2, ::2].copy(), C[1::2, 1::2].copy())
    want = interp_np.interpolate(a, c, bits, 2)[0]
    got = interp.interpolate(da, tuple(_dev(p) for p in c), bits, 2)[0]
    for gp, wp, ap in zip(got, want, a):
        assert np.array_equal(_host(gp, dtype), wp)
    assert all(np.array_equal(wp, ap) for wp, ap in zip(want, a))


def test_the_wrappers_refuse_what_they_cannot_pass():
    t = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    mv = torch.zeros((1, 1, 2), dtype=torch.int16, device="cuda")
    plan = torch.zeros((1, 1, 4), dtype=torch.int16, device="cuda")
    wb = torch.zeros((1, 1), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        interp.interp_select(t.to(torch.float16), t.to(torch.float16), mv, 8, 1, 2)
    with pytest.raises(ValueError):
        interp.interp_select(t, t[:8], mv, 8, 1, 2)
    with pytest.raises(ValueError):
        interp.interp_planes(t, t, plan.to(torch.int32), wb, 1, 2, 0, 0)
    with pytest.raises(ValueError):
        interp.interp_planes(t, t, plan, wb.to(torch.int16), 1, 2, 0, 0)
    with pytest.raises(_lib.DcvcError):
        interp.interp_select(t, t, mv, 8, 2, 2)
    with pytest.raises(_lib.DcvcError):
        interp.interp_select(t, t, mv, 8, 1, 2, limit=256)
    with pytest.raises(_lib.DcvcError):
        interp.interp_planes(t, t, plan, wb, 1, 9, 0, 0)
    with pytest.raises(_lib.DcvcError):
        interp.interp_planes(t, t, plan, wb, 1, 2, 1, 1)              # 8 x 8 blocks: a 2 x 2 grid is needed
    with pytest.raises(_lib.DcvcError):
        interp.interp_planes(t, t, plan, wb, 1, 2, 0, 0, out=t)       # dst is a
