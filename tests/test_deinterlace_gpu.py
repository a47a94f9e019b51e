"""dcvc_deinterlace_planes on a real MI355X against the numpy restatement (tests/deinterlace_np.py) with ==: u8, 10-bit and
16-bit samples over sizes with H = 2, an odd H, W = 1, widths that are no multiple of a vector and tiles that meet on both axes
(the kernel's tile is 128 x 16), random samples, an all-max_val plane, a full comb and diagonal stripes on which every one of the
three directions wins somewhere and scores tie, both parities, both weave sources, thresholds 0, 1, 10 and 64, with and without
history; a three-frame clip in field mode, strided operands with guard samples, misaligned bases, a non-default stream and one
1080p plane."""
import numpy as np
import pytest
import torch

import deinterlace_np as dnp
from dcvc_amd import deinterlace

pytestmark = pytest.mark.gpu

SIZES = [(2, 1), (2, 37), (3, 5), (37, 1), (50, 46), (33, 130), (72, 200), (35, 260)]
KINDS = [("u8", np.uint8, 8), ("u10", np.uint16, 10), ("u16", np.uint16, 16)]
THRESHOLDS = [0, 1, 10, 64]
NAMES = ("random", "all max_val", "comb", "diagonal stripes")


def _dev(a):
    """numpy u8 / u16 -> CUDA tensor (16-bit samples as int16 storage, which every torch has)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()


def _host(t, dtype):
    if dtype == np.uint8:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _stripes(H, W, m):
    """stripes three samples wide: leaning left in the first third of the columns, upright in the second, leaning right in the
    last, so that d = -1, 0 and +1 each match exactly somewhere; two levels only, so scores tie all over"""
    yy, xx = np.mgrid[0:H, 0:W]
    t = np.where(xx < W // 3, xx - yy, np.where(xx < 2 * W // 3, xx, xx + yy))
    return ((t // 3) % 2) * m


def _inputs(H, W, dtype, bits, seed):
    """[4, H, W] woven frames and a previous frame for each: the samples plus noise of a few code values (scaled by the depth),
    so that k is neither all 0 nor all 256"""
    rng = np.random.default_rng(seed)
    m = (1 << bits) - 1
    s = 1 << (bits - 8)
    yy, _ = np.mgrid[0:H, 0:W]
    cur = np.stack([rng.integers(0, m + 1, (H, W)), np.full((H, W), m), (yy & 1) * m, _stripes(H, W, m)])
    prev = np.clip(cur + rng.integers(-5 * s, 5 * s + 1, cur.shape), 0, m)
    return cur.astype(dtype), prev.astype(dtype)


def _reference(cur, prev, keep, weave, thr, bits):
    return np.stack([dnp.deinterlace_plane(cur[p], None if prev is None else prev[p], keep, weave, thr, bits) for p in range(len(cur))])


def _check(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    for p in range(len(want)):
        bad = np.argwhere(got[p] != want[p])
        assert bad.size == 0, (what, NAMES[p] if len(want) == len(NAMES) else p, len(bad), bad[:4].tolist())


def test_the_stripes_exercise_every_direction_and_ties():
    cur = _stripes(50, 46, 255).astype(np.int32)
    seen, ties = set(), 0
    for y in range(1, 49):
        _, which = dnp.spatial_row(cur[y - 1], cur[y + 1])
        s0, sm, sp = dnp.scores_row(cur[y - 1], cur[y + 1])
        seen |= set(np.unique(which).tolist())
        ties += int(((s0 == sm) | (s0 == sp) | (sm == sp)).sum())
    assert seen == {0, -1, 1} and ties > 100


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_planes_equal_the_numpy_restatement(size, kind):
    H, W = size
    _, dtype, bits = kind
    cur, prev = _inputs(H, W, dtype, bits, seed=H * 1000 + W)
    t, p = _dev(cur), _dev(prev)
    mixed = False
    for keep in (0, 1):
        for weave in (0, 1):
            for thr in THRESHOLDS:
                for hist in (None, prev):
                    want = _reference(cur, hist, keep, weave, thr, bits)
                    got = _host(deinterlace.deinterlace_planes(t, None if hist is None else p, keep, weave, thr, bits), dtype)
                    _check(got, want, (keep, weave, thr, hist is not None))
                    assert np.array_equal(got[:, keep::2], cur[:, keep::2])          # kept rows are copies
                    lo = np.minimum(cur.min(), prev.min()) if hist is not None else cur.min()
                    hi = np.maximum(cur.max(), prev.max()) if hist is not None else cur.max()
                    assert got.min() >= lo and got.max() <= hi                        # no clamp needed: never outside what was read
                if thr == 10 and H * W > 1000:
                    spatial = _reference(cur[:1], None, keep, weave, thr, bits)
                    woven = (prev if weave else cur)[:1]
                    blend = _reference(cur[:1], prev[:1], keep, weave, thr, bits)
                    mixed = mixed or ((blend != spatial) & (blend != woven)).any()
    assert mixed or H * W <= 1000                                  # k was neither all 0 nor all 256
    # one plane on its own, as a 2-D tensor, gives the same plane
    one = _host(deinterlace.deinterlace_planes(t[0], p[0], 1, 1, 10, bits), dtype)
    assert np.array_equal(one, _reference(cur[:1], prev[:1], 1, 1, 10, bits)[0])
    assert np.array_equal(_host(t, dtype), cur) and np.array_equal(_host(p, dtype), prev)


@pytest.mark.parametrize("order", ["tff", "bff"])
@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_a_three_frame_clip_in_field_mode(kind, order):
    _, dtype, bits = kind
    H, W = 40, 150
    s = 1 << (bits - 8)
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(21)

    def field(n):
        v = (100 + 50 * np.sin((xx + 2 * (n // 3)) / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)) * s
        return np.clip(np.rint(v + rng.normal(0, s, v.shape)), 0, (1 << bits) - 1).astype(dtype)

    frames = []
    for f in range(3):
        a, b = field(2 * f), field(2 * f + 1)
        w = a.copy()
        w[1::2] = b[1::2]
        frames.append(w)
    want = dnp.deinterlace_clip(frames, "field", order, 10, bits)
    dev = [_dev(f) for f in frames]
    got = []
    for f in range(3):
        for keep, weave in dnp.picture_params("field", order):
            got.append(_host(deinterlace.deinterlace_planes(dev[f], dev[f - 1] if f else None, keep, weave, 10, bits), dtype))
    assert len(got) == len(want) == 6
    for i in range(6):
        assert np.array_equal(got[i], want[i]), i
    assert not np.array_equal(want[2], dnp.deinterlace_plane(frames[1], None, dnp.picture_params("field", order)[0][0], 1, 10, bits))


def _pitch(W, how):
    return {"odd": W + 5, "vector": (W + 15) // 16 * 16 + 16, "tail": (W + 7) // 8 * 8 + 8}[how]


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("how", ["odd", "vector", "tail"])
@pytest.mark.parametrize("size", [(50, 46), (33, 130)], ids=["50x46", "33x130"])
def test_strided_planes_leave_the_guard_samples_alone(size, how, kind):
    """row strides above the width and n_planes = 2 at a plane stride, for cur, prev and dst, each with its own strides"""
    H, W = size
    _, dtype, bits = kind
    m = (1 << bits) - 1
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5
    rng = np.random.default_rng(7)
    c_row, p_row, d_row = _pitch(W, how), _pitch(W, how) + (16 if how == "vector" else 3), _pitch(W, how)
    cur_full = rng.integers(0, m + 1, (2, H + 3, c_row)).astype(dtype)
    prev_full = np.clip(cur_full[:, :H, :W].astype(np.int64) + rng.integers(-4, 5, (2, H, W)) * (1 << (bits - 8)), 0, m).astype(dtype)
    prev_full = np.pad(prev_full, ((0, 0), (0, 1), (0, p_row - W)), constant_values=guard)
    dst_full = np.full((2, H + 2, d_row), guard, dtype)
    t, p, o = _dev(cur_full), _dev(prev_full), _dev(dst_full)
    for keep, hist in ((0, None), (1, p), (0, p)):
        want = _reference(cur_full[:, :H, :W], None if hist is None else prev_full[:, :H, :W], keep, 1, 10, bits)
        o.copy_(_dev(dst_full))
        deinterlace.deinterlace_planes(t[:, :H, :W], None if hist is None else p[:, :H, :W], keep, 1, 10, bits, out=o[:, :H, :W])
        got = _host(o, dtype)
        _check(got[:, :H, :W], want, (how, keep, hist is not None))
        mask = np.ones(dst_full.shape, bool)
        mask[:, :H, :W] = False
        assert (got[mask] == guard).all(), "samples outside the destination planes were written"
    assert np.array_equal(_host(t, dtype), cur_full) and np.array_equal(_host(p, dtype), prev_full)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("which", ["cur", "prev", "dst"])
def test_misaligned_bases_take_the_sample_path(which, kind):
    """a base one sample off a 16-byte boundary, at a width and strides the vector paths would take otherwise"""
    _, dtype, bits = kind
    H, W = 33, 144
    cur, prev = _inputs(H, W, dtype, bits, seed=3)
    cur, prev = cur[0], prev[0]
    want = dnp.deinterlace_plane(cur, prev, 1, 0, 10, bits)
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5

    def shifted(a, off):
        flat = np.full(H * W + 32, guard, dtype)
        flat[off:off + H * W] = a.reshape(-1)
        return _dev(flat)

    offs = {k: (1 if k == which else 0) for k in ("cur", "prev", "dst")}
    fc, fp, fd = shifted(cur, offs["cur"]), shifted(prev, offs["prev"]), shifted(np.full((H, W), guard, dtype), offs["dst"])
    view = lambda f, off: f[off:off + H * W].view(H, W)
    assert view(fc, offs["cur"]).data_ptr() % 16 == (offs["cur"] * cur.itemsize)
    deinterlace.deinterlace_planes(view(fc, offs["cur"]), view(fp, offs["prev"]), 1, 0, 10, bits, out=view(fd, offs["dst"]))
    got = _host(fd, dtype)
    o = offs["dst"]
    assert np.array_equal(got[o:o + H * W].reshape(H, W), want)
    assert (got[:o] == guard).all() and (got[o + H * W:] == guard).all()


def test_a_side_stream():
    H, W, bits = 72, 200, 10
    cur, prev = _inputs(H, W, np.uint16, bits, seed=5)
    want = _reference(cur, prev, 0, 1, 10, bits)
    base, p = _dev(cur), _dev(prev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the input is made on the side stream right before the call and read right after it: only stream order protects them
        t = (base.to(torch.int32) + 0).to(torch.int16)
        got = deinterlace.deinterlace_planes(t, p, 0, 1, 10, bits).clone()
        t.zero_()
    side.synchronize()
    _check(_host(got, np.uint16), want, "side stream")


def test_1080p_u8_with_history():
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:1080, 0:1920]
    clean = 128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)
    cur, prev = (np.clip(np.rint(clean + rng.normal(0, 2, clean.shape)), 0, 255).astype(np.uint8) for _ in range(2))
    for keep, weave in ((0, 1), (1, 0)):
        want = dnp.deinterlace_plane(cur, prev, keep, weave, 10, 8)
        got = _host(deinterlace.deinterlace_planes(_dev(cur), _dev(prev), keep, weave, 10, 8), np.uint8)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (len(bad), bad[:4].tolist())
        assert not np.array_equal(got, cur)


def test_the_wrapper_refuses_what_it_cannot_pass():
    t = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        deinterlace.deinterlace_planes(t.to(torch.float16), None, 0, 0, 10, 8)
    with pytest.raises(ValueError):
        deinterlace.deinterlace_planes(t, torch.zeros((8, 9), dtype=torch.uint8, device="cuda"), 0, 0, 10, 8)
    with pytest.raises(ValueError):
        deinterlace.deinterlace_planes(t, None, 0, 0, 10, 8, out=torch.zeros((8, 9), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        deinterlace.deinterlace_planes(t.cpu(), None, 0, 0, 10, 8)
    from dcvc_amd import _lib
    for bad in (dict(keep=2), dict(weave_from_prev=2), dict(threshold=65), dict(bit_depth=10)):
        args = dict(keep=0, weave_from_prev=0, threshold=10, bit_depth=8)
        args.update(bad)
        with pytest.raises(_lib.DcvcError, match="deinterlace:"):
            deinterlace.deinterlace_planes(t, None, **args)
    with pytest.raises(_lib.DcvcError, match="H must be in 2"):
        deinterlace.deinterlace_planes(t[:1], None, 0, 0, 10, 8)
