"""dcvc_motion_search and dcvc_motion_compensate_planes on a real MI355X against the numpy restatement (tests/motion_np.py) with
==: u8, 10-bit and 16-bit full-range samples over sizes with one block, partial blocks on either axis and several blocks, windows
that exceed the plane (48x80 at range 15), range 0, lambda 0 and 255, row strides above the width, a misaligned base, cur == ref;
the compensation at all four subsamplings with negative odd vectors, vectors of +-32767, three planes in one call, strided
operands with guard samples and zero vectors; the Python wrappers against the C calls."""
import ctypes

import numpy as np
import pytest
import torch

import motion_np
from dcvc_amd import _lib, motion

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (15, 17), (16, 16), (17, 33), (33, 31)]
KINDS = [("u8", np.uint8, 8), ("u10", np.uint16, 10), ("u16", np.uint16, 16)]
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
    """(cur, ref): a smooth texture moved by a few samples plus full-range outliers and noise - the costs of neighbouring
    candidates differ, and the samples reach 0 and the largest value of the depth"""
    rng = np.random.default_rng(seed)
    m = (1 << bits) - 1
    yy, xx = np.mgrid[0:H + 8, 0:W + 8]
    base = (0.5 + 0.3 * np.sin(xx / 3.1) * np.cos(yy / 2.3) + 0.2 * ((xx // 5 + yy // 7) & 1)) * m
    ref = base[4:4 + H, 4:4 + W] + rng.normal(0, m / 64.0, (H, W))
    cur = base[2:2 + H, 7:7 + W] + rng.normal(0, m / 64.0, (H, W))
    for a in (ref, cur):
        k = rng.random((H, W))
        a[k < 0.02] = 0
        a[k > 0.98] = m
    return np.clip(np.rint(cur), 0, m).astype(dtype), np.clip(np.rint(ref), 0, m).astype(dtype)


def _search(cur, ref, dtype, bits, R, lam):
    mv, sad = motion.motion_search(_dev(cur), _dev(ref), bits, R, lam)
    return mv.cpu().numpy(), sad.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    mv, sad = got
    wmv, wsad = want
    assert mv.shape == wmv.shape and mv.dtype == np.int16 and sad.shape == wsad.shape
    bad = np.argwhere((mv != wmv).any(axis=-1))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), mv[tuple(bad[0])].tolist(), wmv[tuple(bad[0])].tolist())
    assert np.array_equal(sad, wsad), what


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_the_search_equals_the_numpy_restatement(size, kind):
    H, W = size
    _, dtype, bits = kind
    cur, ref = _pair(H, W, dtype, bits, seed=H * 100 + W)
    for R, lam in [(7, 4), (0, 4), (3, 0), (5, 255), (15, 1)]:
        want = motion_np.motion_search(cur, ref, bits, R, lam)
        _same(_search(cur, ref, dtype, bits, R, lam), want, (R, lam))
        assert np.abs(want[0]).max() <= 2 * R + 1
    # cur == ref is allowed: every vector is zero, every SAD too
    t = _dev(cur)
    mv, sad = motion.motion_search(t, t, bits, 7, 4)
    assert not mv.any() and not sad.any()


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_windows_that_exceed_the_plane(kind):
    """48x80 at range 15: the level-1 window of 38 half-resolution samples is wider than the 24x40 half-resolution plane"""
    _, dtype, bits = kind
    cur, ref = _pair(48, 80, dtype, bits, seed=7)
    for lam in (0, 4):
        _same(_search(cur, ref, dtype, bits, 15, lam), motion_np.motion_search(cur, ref, bits, 15, lam), lam)
    # a pure translation by (-30, 30), found at the far corner of the range in the block whose window stays inside
    big = _pair(48 + 64, 80 + 64, dtype, bits, seed=8)[1]
    ref2, cur2 = big[32:80, 32:112], big[62:110, 2:82]
    got = _search(cur2, ref2, dtype, bits, 15, 4)
    _same(got, motion_np.motion_search(cur2, ref2, bits, 15, 4), "translation")


def test_full_range_16_bit_extremes():
    """0 / 65535 checkerboards against each other, and an all-0 plane against an all-65535 one: there every candidate has the
    largest SAD, 256 * 65535 in a whole block, and with lambda 255 and range 15 the largest penalties are added to it"""
    yy, xx = np.mgrid[0:33, 0:47]
    cur = (((yy + xx) & 1) * 65535).astype(np.uint16)
    ref = (65535 - cur).astype(np.uint16)
    for R in (0, 2):
        want = motion_np.motion_search(cur, ref, 16, R, 255)
        _same(_search(cur, ref, np.uint16, 16, R, 255), want, R)
    cur, ref = np.zeros((33, 47), np.uint16), np.full((33, 47), 65535, np.uint16)
    want = motion_np.motion_search(cur, ref, 16, 15, 255)
    assert want[1].max() == 256 * 65535 and not want[0].any()
    _same(_search(cur, ref, np.uint16, 16, 15, 255), want, "constant")


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_strided_rows_and_a_misaligned_base(kind):
    _, dtype, bits = kind
    H, W = 33, 50
    cur, ref = _pair(H, W, dtype, bits, seed=11)
    want = motion_np.motion_search(cur, ref, bits, 7, 4)
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5
    cf, rf = np.full((H, W + 7), guard, dtype), np.full((H + 1, W + 13), guard, dtype)
    cf[:, :W], rf[:H, :W] = cur, ref
    tc, tr = _dev(cf), _dev(rf)
    mv, sad = motion.motion_search(tc[:, :W], tr[:H, :W], bits, 7, 4)
    _same((mv.cpu().numpy(), sad.cpu().numpy().view(np.uint32)), want, "strided")
    flat = np.full(H * W + 16, guard, dtype)
    flat[1:1 + H * W] = cur.reshape(-1)
    tf = _dev(flat)
    view = tf[1:1 + H * W].view(H, W)
    assert view.data_ptr() % 16 == cur.itemsize
    mv, sad = motion.motion_search(view, _dev(ref), bits, 7, 4)
    _same((mv.cpu().numpy(), sad.cpu().numpy().view(np.uint32)), want, "misaligned")
    assert np.array_equal(_host(tc, dtype), cf) and np.array_equal(_host(tr, dtype), rf)


def test_the_c_call_fills_a_larger_grid_sad_is_optional_and_moved_counts():
    H, W, bits = 40, 70, 8
    cur, ref = _pair(H, W, np.uint8, bits, seed=13)
    wmv, wsad = motion_np.motion_search(cur, ref, bits, 7, 4)
    Bh, Bw = motion_np.grid(H, W)
    f = _lib.fn("dcvc_motion_search", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp, vp, vp, cll, vp])
    need = _lib.fn("dcvc_motion_search_workspace_bytes", cll, [ci, ci])(H, W)
    tc, tr = _dev(cur), _dev(ref)
    mv = torch.full((Bh + 1, Bw + 2, 2), 999, dtype=torch.int16, device="cuda")
    sad = torch.full((Bh + 1, Bw + 2), -5, dtype=torch.int32, device="cuda")
    moved = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(need + 64, dtype=torch.uint8, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    for with_sad in (True, False):
        _lib.check(f(vp(tc.data_ptr()), W, vp(tr.data_ptr()), W, 0, 8, H, W, 7, 4, vp(mv.data_ptr()), Bh + 1, Bw + 2,
                     vp(sad.data_ptr()) if with_sad else None, vp(moved.data_ptr()), vp(ws.data_ptr()), need, st))
    got, gsad = mv.cpu().numpy(), sad.cpu().numpy()
    assert np.array_equal(got[:Bh, :Bw], wmv) and np.array_equal(gsad[:Bh, :Bw].view(np.uint32), wsad)
    assert (got[Bh:] == 999).all() and (got[:, Bw:] == 999).all() and (gsad[Bh:] == -5).all() and (gsad[:, Bw:] == -5).all()
    assert int(moved.item()) == 2 * int(wmv.any(axis=-1).sum())          # two calls, each adds its count
    # the wrapper gives what the C call gave
    pmv, psad = motion.motion_search(tc, tr, bits)                       # the defaults are range 7, lambda 4
    assert np.array_equal(pmv.cpu().numpy(), wmv) and np.array_equal(psad.cpu().numpy().view(np.uint32), wsad)
    out = torch.empty((Bh, Bw, 2), dtype=torch.int16, device="cuda")
    assert motion.motion_search(tc, tr, bits, out=out)[0] is out and np.array_equal(out.cpu().numpy(), wmv)


# ------------------------------------------------------------------------------------ compensation
def _vectors(Bh, Bw, seed):
    """negative odd components, large ones and +-32767 among ordinary ones"""
    rng = np.random.default_rng(seed)
    mv = rng.integers(-31, 32, (Bh, Bw, 2)).astype(np.int16)
    flat = mv.reshape(-1, 2)
    special = [(-1, -1), (-3, 5), (7, -9), (32767, -32767), (-32767, 32767), (0, 0), (-31, -31), (1, -32767)]
    for i, v in enumerate(special):
        flat[(i * 5) % len(flat)] = v
    return mv


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("sub", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["444", "422", "440", "420"])
@pytest.mark.parametrize("size", [(1, 1), (15, 17), (33, 31), (40, 150), (50, 260)], ids=lambda s: "%dx%d" % s)
def test_compensation_equals_the_numpy_restatement(size, sub, kind):
    H, W = size
    sx, sy = sub
    _, dtype, bits = kind
    Bh, Bw = -(-H // (16 >> sy)), -(-W // (16 >> sx))
    rng = np.random.default_rng(H + W)
    prev = rng.integers(0, 1 << bits, (3, H, W)).astype(dtype)
    mv = _vectors(Bh, Bw, seed=3)
    want = np.stack([motion_np.compensate_plane(p, mv, sx, sy) for p in prev])
    tp, tm = _dev(prev), _dev(mv)
    got = _host(motion.motion_compensate_planes(tp, tm, sx, sy), dtype)      # three planes in one call
    assert got.dtype == dtype and np.array_equal(got, want)
    one = _host(motion.motion_compensate_planes(tp[1], tm, sx, sy), dtype)   # a plane on its own, as a 2-D tensor
    assert np.array_equal(one, want[1])
    zero = _host(motion.motion_compensate_planes(tp, torch.zeros_like(tm), sx, sy), dtype)
    assert np.array_equal(zero, prev)                                        # the copy
    assert np.array_equal(_host(tp, dtype), prev)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("how", ["odd", "vector"])
def test_strided_compensation_leaves_the_guard_samples_alone(how, kind):
    _, dtype, bits = kind
    H, W, sx, sy = 33, 130, 1, 1
    p_row, d_row = (W + 5, W + 3) if how == "odd" else (W + 14, (W + 15) // 16 * 16 + 16)
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5
    rng = np.random.default_rng(9)
    prev_full = rng.integers(0, 1 << bits, (2, H + 1, p_row)).astype(dtype)
    dst_full = np.full((2, H + 2, d_row), guard, dtype)
    mv = _vectors(-(-H // 8), -(-W // 8), seed=4)
    want = np.stack([motion_np.compensate_plane(p[:H, :W], mv, sx, sy) for p in prev_full])
    tp, to = _dev(prev_full), _dev(dst_full)
    assert motion.motion_compensate_planes(tp[:, :H, :W], _dev(mv), sx, sy, out=to[:, :H, :W]).data_ptr() == to.data_ptr()
    got = _host(to, dtype)
    assert np.array_equal(got[:, :H, :W], want)
    mask = np.ones(dst_full.shape, bool)
    mask[:, :H, :W] = False
    assert (got[mask] == guard).all(), "samples outside the destination planes were written"
    # a destination one sample off a 16-byte boundary takes the sample-by-sample stores
    flat = _dev(np.full(H * W + 32, guard, dtype))
    view = flat[1:1 + H * W].view(H, W)
    motion.motion_compensate_planes(tp[0, :H, :W], _dev(mv), sx, sy, out=view)
    gf = _host(flat, dtype)
    assert np.array_equal(gf[1:1 + H * W].reshape(H, W), want[0]) and gf[0] == guard and (gf[1 + H * W:] == guard).all()


def test_the_c_call_takes_a_larger_grid():
    H, W = 20, 40
    prev = np.random.default_rng(1).integers(0, 256, (H, W)).astype(np.uint8)
    mv = _vectors(4, 6, seed=5)                                              # the plane needs 2 x 3
    f = _lib.fn("dcvc_motion_compensate_planes", ci, [vp, ci, cll, vp, ci, cll, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp])
    tp, tm = _dev(prev), _dev(mv)
    out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    _lib.check(f(vp(tp.data_ptr()), W, 0, vp(out.data_ptr()), W, 0, 0, H, W, 1, 0, 0, vp(tm.data_ptr()), 4, 6,
                 vp(torch.cuda.current_stream().cuda_stream)))
    assert np.array_equal(out.cpu().numpy(), motion_np.compensate_plane(prev, mv))
    assert np.array_equal(motion.motion_compensate_planes(tp, tm, 0, 0).cpu().numpy(), out.cpu().numpy())


def test_search_then_compensate_then_denoise_is_the_numpy_clip():
    """the chain the tool runs, on three pictures of a panning noisy scene, 4:2:0"""
    import denoise_np
    from dcvc_amd import denoise
    H, W, bits = 48, 80, 8
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:H, 0:W + 16]
    wide = 128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)
    clip = []
    for i in range(3):
        y = wide[:, 5 * i:5 * i + W]
        c = y[::2, ::2]
        clip.append(tuple(np.clip(np.rint(p + rng.normal(0, 3, p.shape)), 0, 255).astype(np.uint8) for p in (y, c, 255 - c)))
    want, mvs = motion_np.mc_denoise_clip(clip, 8, 8, bits, 7, 4)
    assert mvs[2][0].any()
    prev = None
    for i, pic in enumerate(clip):
        y, uv = _dev(pic[0]), _dev(np.stack(pic[1:]))
        if prev is None:
            cy, cuv = None, None
        else:
            mv, _ = motion.motion_search(y, prev[0], bits, 7, 4)
            assert np.array_equal(mv.cpu().numpy(), mvs[i][0])
            cy, cuv = motion.motion_compensate_planes(prev[0], mv, 0, 0), motion.motion_compensate_planes(prev[1], mv, 1, 1)
        prev = (denoise.denoise_planes(y, cy, 8, 8, bits), denoise.denoise_planes(uv, cuv, 8, 8, bits))
        assert np.array_equal(prev[0].cpu().numpy(), want[i][0])
        assert np.array_equal(prev[1].cpu().numpy(), np.stack(want[i][1:]))
    assert not np.array_equal(want[2][0], denoise_np.denoise_clip(clip, 8, 8, bits)[2][0])      # the compensation counts


def test_the_wrappers_refuse_what_they_cannot_pass():
    t = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    mv = torch.zeros((1, 1, 2), dtype=torch.int16, device="cuda")
    with pytest.raises(TypeError):
        motion.motion_search(t.to(torch.float16), t.to(torch.float16), 8)
    with pytest.raises(ValueError):
        motion.motion_search(t, t[:8], 8)
    with pytest.raises(ValueError):
        motion.motion_compensate_planes(t, mv.to(torch.int32), 0, 0)
    with pytest.raises(_lib.DcvcError):
        motion.motion_search(t, t, 8, search_range=16)
    with pytest.raises(_lib.DcvcError):
        motion.motion_compensate_planes(t, mv, 2, 0)
    with pytest.raises(_lib.DcvcError):
        motion.motion_compensate_planes(t, mv, 1, 1)              # 8 x 8 blocks: a 2 x 2 grid is needed
