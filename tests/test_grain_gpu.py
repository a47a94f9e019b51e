"""dcvc_grain_apply and dcvc_grain_stats on a real MI355X against the numpy restatement (tests/grain_np.py) with ==: u8, 10-bit
and 16-bit samples; planes of 1 x 1, 33 x 65, 64 x 64 (whole blocks), 70 x 100 (3 x 4 blocks with ragged edges) and 67 x 300
(more than one tile of either kernel along x, two along y); the luma plane itself and planes subsampled by (1, 0) and (1, 1)
against luma planes of the smallest size allowed (the clamp binds) and of twice the plane; row strides above the width with
guard samples, plane strides, bases one sample off alignment; tables of zeros (a copy), tables of 255 on pictures of 0 and of
max_val (the clamp binds on both sides), two picture indexes, Y in place; for the measurement flat 0 and 255, a luma that leaves
bins empty, accumulation, and two runs."""
import numpy as np
import pytest
import torch

import grain_np as gnp
from dcvc_amd import _lib, grain

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (33, 65), (64, 64), (70, 100), (67, 300)]
KINDS = [("u8", np.uint8, 8), ("u10", np.uint16, 10), ("u16", np.uint16, 16)]
SUBS = [(0, 0), (1, 0), (1, 1)]
SEED, SIZE = 1234, 12
GUARD = {np.uint8: 0xA5, np.uint16: 0xA5A5}


def _dev(a):
    """numpy u8 / u16 -> CUDA tensor (16-bit samples as int16 storage, which every torch has)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()


def _host(t, dtype):
    if dtype == np.uint8:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


_cache = {}


def _templates():
    """(numpy int16 [3, 64, 64], the same on the device): made once"""
    if "t" not in _cache:
        T = np.stack([gnp.template(SEED, p, SIZE) for p in range(3)])
        _cache["t"] = (T, torch.from_numpy(T).cuda())
    return _cache["t"]


def _luma_shape(H, W, sx, sy, how):
    if how == "min":
        return ((H - 1) << sy) + 1, ((W - 1) << sx) + 1
    return H << sy, W << sx


def _rand(rng, shape, bits, dtype):
    return rng.integers(0, 1 << bits, shape).astype(dtype)


def _want_apply(rec, luma, lut, pic, first, bits, sx, sy):
    T, _ = _templates()
    return np.stack([gnp.apply_plane(rec[i], luma, T[first + i], lut[first + i], SEED, pic, first + i, bits, sx, sy) for i in range(len(rec))])


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_apply_equals_the_numpy_restatement(size, kind):
    H, W = size
    _, dtype, bits = kind
    m = (1 << bits) - 1
    rng = np.random.default_rng(H * 1000 + W + bits)
    _, tpl = _templates()
    lut = rng.integers(0, 256, (3, 9)).tolist()
    zeros, full = [[0] * 9] * 3, [[255] * 9] * 3
    # the luma plane: rec is its own luma
    y = _rand(rng, (H, W), bits, dtype)
    ty = _dev(y)
    pics = []
    for pic in (0, 1, 0xFFFFFFFF):
        got = _host(grain.grain_apply(ty, ty, tpl, lut, SEED, pic, 0, bits, 0, 0), dtype)
        _same(got, _want_apply(y[None], y, lut, pic, 0, bits, 0, 0)[0], ("Y", pic))
        pics.append(got)
    if H * W >= 64:
        assert not np.array_equal(pics[0], pics[1]) and not np.array_equal(pics[0], y)        # pic moves the blocks
    assert np.array_equal(_host(grain.grain_apply(ty, ty, tpl, zeros, SEED, 0, 0, bits, 0, 0), dtype), y)      # a copy
    assert np.array_equal(_host(ty, dtype), y)                   # out of place leaves rec alone
    for level in (0, m):                                         # the clamp binds: half of the grain points outside 0..max_val
        flat = np.full((H, W), level, dtype)
        n = gnp.grain_samples((H, W), flat, _templates()[0][0], full[0], SEED, 0, 0, bits, 0, 0)
        got = _host(grain.grain_apply(_dev(flat), _dev(flat), tpl, full, SEED, 0, 0, bits, 0, 0), dtype)
        _same(got, np.clip(level + n, 0, m).astype(dtype), ("clamp", level))
        if H * W >= 64:
            assert (level + n).min() < 0 if level == 0 else (level + n).max() > m
            assert got.min() == 0 if level == 0 else got.max() == m
    # in place: rec, luma and dst are one plane
    t = _dev(y)
    assert grain.grain_apply(t, t, tpl, lut, SEED, 1, 0, bits, 0, 0, out=t) is t
    _same(_host(t, dtype), pics[1], "Y in place")
    # two chroma planes against a luma plane of their own, every subsampling
    for sx, sy in SUBS:
        for how in ("min", "twice"):
            if (sx, sy) == (0, 0) and how == "twice":
                continue
            luma = _rand(rng, _luma_shape(H, W, sx, sy, how), bits, dtype)
            uv = _rand(rng, (2, H, W), bits, dtype)
            tl, tuv = _dev(luma), _dev(uv)
            for table in (lut, zeros):
                got = _host(grain.grain_apply(tuv, tl, tpl, table, SEED, 3, 1, bits, sx, sy), dtype)
                _same(got, _want_apply(uv, luma, table, 3, 1, bits, sx, sy), ("UV", sx, sy, how))
                if table is zeros:
                    assert np.array_equal(got, uv)
            # V alone, as a 2-D tensor, and U and V in place
            one = _host(grain.grain_apply(tuv[1], tl, tpl, lut, SEED, 3, 2, bits, sx, sy), dtype)
            _same(one, _want_apply(uv[1:], luma, lut, 3, 2, bits, sx, sy)[0], ("V", sx, sy, how))
            grain.grain_apply(tuv, tl, tpl, lut, SEED, 3, 1, bits, sx, sy, out=tuv)
            _same(_host(tuv, dtype), _want_apply(uv, luma, lut, 3, 1, bits, sx, sy), ("UV in place", sx, sy, how))
            assert np.array_equal(_host(tl, dtype), luma)
    # all three planes of a 4:4:4 picture in one call, out of place
    yuv = _rand(rng, (3, H, W), bits, dtype)
    t3 = _dev(yuv)
    got = _host(grain.grain_apply(t3, t3[0], tpl, lut, SEED, 2, 0, bits, 0, 0), dtype)
    _same(got, _want_apply(yuv, yuv[0], lut, 2, 0, bits, 0, 0), "4:4:4")


def _pitch(W, how):
    return {"odd": W + 5, "vector": (W + 15) // 16 * 16 + 16}[how]


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("how", ["odd", "vector"])
@pytest.mark.parametrize("sub", SUBS, ids=["%d%d" % s for s in SUBS])
@pytest.mark.parametrize("size", [(33, 65), (70, 100)], ids=["33x65", "70x100"])
def test_apply_on_strided_planes_leaves_the_guard_samples_alone(size, sub, how, kind):
    """row strides above the width and a plane stride above the plane, for rec, the luma and dst, each with its own strides"""
    H, W = size
    sx, sy = sub
    _, dtype, bits = kind
    guard = GUARD[dtype]
    rng = np.random.default_rng(7)
    _, tpl = _templates()
    lut = rng.integers(0, 256, (3, 9)).tolist()
    Hl, Wl = _luma_shape(H, W, sx, sy, "min")
    r_row, l_row, d_row = _pitch(W, how), _pitch(Wl, how) + (16 if how == "vector" else 3), _pitch(W, how) + (32 if how == "vector" else 1)
    rec_full = _rand(rng, (2, H + 3, r_row), bits, dtype)
    luma_full = _rand(rng, (Hl + 1, l_row), bits, dtype)
    dst_full = np.full((2, H + 2, d_row), guard, dtype)
    r, l, o = _dev(rec_full), _dev(luma_full), _dev(dst_full)
    grain.grain_apply(r[:, :H, :W], l[:Hl, :Wl], tpl, lut, SEED, 5, 1, bits, sx, sy, out=o[:, :H, :W])
    got = _host(o, dtype)
    _same(got[:, :H, :W], _want_apply(rec_full[:, :H, :W], luma_full[:Hl, :Wl], lut, 5, 1, bits, sx, sy), (how, sub))
    mask = np.ones(dst_full.shape, bool)
    mask[:, :H, :W] = False
    assert (got[mask] == guard).all(), "samples outside the destination planes were written"
    assert np.array_equal(_host(r, dtype), rec_full) and np.array_equal(_host(l, dtype), luma_full)


def _shifted(a, off, guard):
    """a's samples from `off` on in a flat guard-filled device buffer, and the view of them"""
    flat = np.full(a.size + 32, guard, a.dtype)
    flat[off:off + a.size] = a.reshape(-1)
    t = _dev(flat)
    return t, t[off:off + a.size].view(*a.shape)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("which", ["rec", "luma", "dst", "all"])
@pytest.mark.parametrize("sub", SUBS, ids=["%d%d" % s for s in SUBS])
def test_apply_with_a_base_one_sample_off_alignment(sub, which, kind):
    """at a width and strides the vector path would take otherwise"""
    sx, sy = sub
    _, dtype, bits = kind
    H, W = 33, 144
    guard = GUARD[dtype]
    rng = np.random.default_rng(3)
    _, tpl = _templates()
    lut = rng.integers(0, 256, (3, 9)).tolist()
    rec, luma = _rand(rng, (H, W), bits, dtype), _rand(rng, _luma_shape(H, W, sx, sy, "twice"), bits, dtype)
    off = {k: (1 if which in (k, "all") else 0) for k in ("rec", "luma", "dst")}
    _, vr = _shifted(rec, off["rec"], guard)
    _, vl = _shifted(luma, off["luma"], guard)
    fd, vd = _shifted(np.full((H, W), guard, dtype), off["dst"], guard)
    assert vr.data_ptr() % 16 == off["rec"] * rec.itemsize and vd.data_ptr() % 16 == off["dst"] * rec.itemsize
    grain.grain_apply(vr, vl, tpl, lut, SEED, 0, 1, bits, sx, sy, out=vd)
    got = _host(fd, dtype)
    o = off["dst"]
    _same(got[o:o + H * W].reshape(H, W), _want_apply(rec[None], luma, lut, 0, 1, bits, sx, sy)[0], (sub, which))
    assert (got[:o] == guard).all() and (got[o + H * W:] == guard).all()
    if which == "all" and sub == (0, 0):                         # the luma plane in place at a misaligned base
        _, v = _shifted(rec, 1, guard)
        grain.grain_apply(v, v, tpl, lut, SEED, 0, 0, bits, 0, 0, out=v)
        _same(_host(v.contiguous(), dtype), _want_apply(rec[None], rec, lut, 0, 0, bits, 0, 0)[0], "Y in place, misaligned")


# ------------------------------------------------------------------------------------ the measurement
def _den_src(rng, shape, bits, dtype, lo=0, hi=256):
    """a denoised picture with flat areas (4 x 4 blocks of one level, the left half without any noise) and a source around it"""
    H, W = shape[-2:]
    s = 1 << (bits - 8)
    m = (1 << bits) - 1
    levels = rng.integers(lo * s, hi * s, shape[:-2] + ((H + 3) // 4, (W + 3) // 4))
    den = np.repeat(np.repeat(levels, 4, axis=-2), 4, axis=-1)[..., :H, :W]
    noise = rng.integers(-2 * s, 2 * s + 1, shape)
    noise[..., :, :W // 2] = 0
    den = np.clip(den + noise, lo * s, hi * s - 1)
    src = np.clip(den + rng.integers(-6 * s, 6 * s + 1, shape), 0, m)
    return den.astype(dtype), src.astype(dtype)


def _want_stats(src, den, luma, bits, sx, sy, flat):
    return [gnp.stats_plane(src[i], den[i], luma, bits, sx, sy, flat) for i in range(len(src))]


def _words(t):
    return t.cpu().numpy().tolist()


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_stats_equal_the_numpy_restatement(size, kind):
    H, W = size
    _, dtype, bits = kind
    rng = np.random.default_rng(H * 1000 + W + bits + 1)
    den, src = _den_src(rng, (H, W), bits, dtype)
    td, ts = _dev(den), _dev(src)
    counted = 0
    for flat in (0, 4, 255):
        want = gnp.stats_plane(src, den, den, bits, 0, 0, flat)
        got = grain.grain_stats(ts, td, td, bits, 0, 0, flat)
        assert got.dtype == torch.int64 and tuple(got.shape) == (16,)
        assert _words(got) == want, ("Y", flat)
        assert sum(want[:8]) >= counted                          # a larger flat counts no fewer samples
        counted = sum(want[:8])
        if flat == 255 and bits == 8:
            assert counted == H * W
    if H * W >= 64:
        assert 0 < sum(gnp.stats_plane(src, den, den, bits, 0, 0, 0)[:8]) < H * W
    # two runs, and accumulation into words that are not zeroed
    out = torch.full((16,), -7, dtype=torch.int64, device="cuda")
    assert grain.grain_stats(ts, td, td, bits, 0, 0, 4, out=out) is out
    once = _words(out)
    assert once == gnp.stats_plane(src, den, den, bits, 0, 0, 4)
    grain.grain_stats(ts, td, td, bits, 0, 0, 4, out=out, accumulate=True)
    assert _words(out) == [2 * v for v in once]
    grain.grain_stats(ts, td, td, bits, 0, 0, 4, out=out)
    assert _words(out) == once
    # two chroma planes against den's luma, every subsampling
    for sx, sy in SUBS:
        for how in ("min", "twice"):
            if (sx, sy) == (0, 0) and how == "twice":
                continue
            luma = _rand(rng, _luma_shape(H, W, sx, sy, how), bits, dtype)
            den2, src2 = _den_src(rng, (2, H, W), bits, dtype)
            got = grain.grain_stats(_dev(src2), _dev(den2), _dev(luma), bits, sx, sy, 4)
            assert tuple(got.shape) == (2, 16)
            assert _words(got) == _want_stats(src2, den2, luma, bits, sx, sy, 4), (sx, sy, how)
    assert np.array_equal(_host(td, dtype), den) and np.array_equal(_host(ts, dtype), src)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_stats_of_a_luma_that_leaves_bins_empty(kind):
    _, dtype, bits = kind
    H, W = 70, 100
    rng = np.random.default_rng(9)
    den, src = _den_src(rng, (H, W), bits, dtype, lo=64, hi=128)             # bins 2 and 3 only
    got = _words(grain.grain_stats(_dev(src), _dev(den), _dev(den), bits, 0, 0, 255))
    assert got == gnp.stats_plane(src, den, den, bits, 0, 0, 255)
    assert [k for k in range(8) if got[k]] == [2, 3] and [k for k in range(8) if got[8 + k]] == [2, 3]
    # the largest differences: src 0 against den max_val in every sample, d^2 = max_val^2 (past 32 bits for one wave at 16 bits)
    m = (1 << bits) - 1
    hi, lo = np.full((H, W), m, dtype), np.zeros((H, W), dtype)
    got = _words(grain.grain_stats(_dev(lo), _dev(hi), _dev(hi), bits, 0, 0, 0))
    assert got == [0] * 7 + [H * W] + [0] * 7 + [H * W * m * m] == gnp.stats_plane(lo, hi, hi, bits, 0, 0, 0)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("how", ["odd", "vector", "off by one"])
@pytest.mark.parametrize("sub", SUBS, ids=["%d%d" % s for s in SUBS])
def test_stats_on_strided_and_misaligned_planes(sub, how, kind):
    sx, sy = sub
    _, dtype, bits = kind
    H, W = 33, 144
    rng = np.random.default_rng(13)
    Hl, Wl = _luma_shape(H, W, sx, sy, "min")
    den, src = _den_src(rng, (2, H, W), bits, dtype)
    luma = _rand(rng, (Hl, Wl), bits, dtype)
    want = _want_stats(src, den, luma, bits, sx, sy, 4)
    if how == "off by one":
        vs, vd, vl = (_shifted(a, 1, GUARD[dtype])[1] for a in (src, den, luma))
    else:
        pad = lambda a, row: _dev(np.pad(a, [(0, 0)] * (a.ndim - 2) + [(0, 2), (0, row - a.shape[-1])], constant_values=GUARD[dtype]))      # noqa: E731
        vs = pad(src, _pitch(W, how))[:, :H, :W]
        vd = pad(den, _pitch(W, how) + (16 if how == "vector" else 3))[:, :H, :W]
        vl = pad(luma, _pitch(Wl, how))[:Hl, :Wl]
    assert _words(grain.grain_stats(vs, vd, vl, bits, sx, sy, 4)) == want


def test_a_side_stream():
    H, W, bits = 70, 300, 10
    rng = np.random.default_rng(5)
    _, tpl = _templates()
    lut = rng.integers(0, 256, (3, 9)).tolist()
    y = _rand(rng, (H, W), bits, np.uint16)
    base = _dev(y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the input is made on the side stream right before the calls and cleared right after them: only stream order protects it
        t = (base.to(torch.int32) + 0).to(torch.int16)
        got = grain.grain_apply(t, t, tpl, lut, SEED, 0, 0, bits, 0, 0)
        words = grain.grain_stats(got, t, t, bits, 0, 0, 255)
        t.zero_()
    side.synchronize()
    want = _want_apply(y[None], y, lut, 0, 0, bits, 0, 0)[0]
    _same(_host(got, np.uint16), want, "side stream")
    assert _words(words) == gnp.stats_plane(want, y, y, bits, 0, 0, 255)


def test_the_wrappers_refuse_what_they_cannot_pass():
    _, tpl = _templates()
    lut = [[16] * 9] * 3
    t = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        grain.grain_apply(t.to(torch.float16), t, tpl, lut, 1, 0, 0, 8, 0, 0)
    with pytest.raises(ValueError):
        grain.grain_apply(t, t, tpl[:2], lut, 1, 0, 0, 8, 0, 0)
    with pytest.raises(ValueError):
        grain.grain_apply(t, t, tpl, [[256] * 9] * 3, 1, 0, 0, 8, 0, 0)
    with pytest.raises(ValueError):
        grain.grain_stats(t, torch.zeros((8, 9), dtype=torch.uint8, device="cuda"), t, 8, 0, 0, 4)
    with pytest.raises(TypeError):
        grain.grain_stats(t.to(torch.float32), t, t, 8, 0, 0, 4)
    with pytest.raises(_lib.DcvcError, match="luma plane"):
        grain.grain_apply(t, t, tpl, lut, 1, 0, 1, 8, 1, 1)              # a luma plane of the chroma's size
    with pytest.raises(_lib.DcvcError, match="flat"):
        grain.grain_stats(t, t, t, 8, 0, 0, 256)
    with pytest.raises(_lib.DcvcError, match="overlaps the luma"):
        u = torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda")
        grain.grain_apply(u, u[0], tpl, lut, 1, 0, 0, 8, 0, 0, out=u)     # Y would be grained while U reads it
