"""dcvc_denoise_planes on a real MI355X against the numpy restatement (tests/denoise_np.py) with ==: u8, 10-bit and 16-bit
samples over sizes where a halo is wider than the plane, a width is no multiple of a vector and tiles meet on both axes (the
kernel's tile is 128 x 16), random samples, an all-max_val plane, a 0 / max_val checkerboard and a checkerboard of half the
largest threshold (the accumulator bound), with and without history, a three-picture recursion, strided operands with guard
samples, misaligned bases, a non-default stream and one 1080p plane."""
import numpy as np
import pytest
import torch

import denoise_np
from dcvc_amd import denoise

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 37), (37, 1), (2, 3), (50, 46), (33, 130), (72, 200), (35, 260)]
KINDS = [("u8", np.uint8, 8), ("u10", np.uint16, 10), ("u16", np.uint16, 16)]
STRENGTHS = [(0, 0), (12, 0), (0, 12), (8, 8), (64, 64)]
NAMES = ("random", "all max_val", "checkerboard", "half-threshold checkerboard")


def _dev(a):
    """numpy u8 / u16 -> CUDA tensor (16-bit samples as int16 storage, which every torch has)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()


def _host(t, dtype):
    if dtype == np.uint8:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _inputs(H, W, dtype, bits, seed):
    """[4, H, W] samples and a previous output picture for each: the samples plus noise of a few code values, so that the
    temporal weights are neither all 0 nor all 192"""
    rng = np.random.default_rng(seed)
    m = (1 << bits) - 1
    s = 1 << (bits - 8)
    yy, xx = np.mgrid[0:H, 0:W]
    half = 32 * s                                     # half of Ts at strength 64: the largest w_i |n_i - c|
    src = np.stack([rng.integers(0, m + 1, (H, W)), np.full((H, W), m), ((yy + xx) & 1) * m, m - ((yy + xx) & 1) * half])
    prev = np.clip(src + rng.integers(-5 * s, 5 * s + 1, src.shape), 0, m)
    return src.astype(dtype), prev.astype(dtype)


def _reference(src, prev, S, T, bits):
    return np.stack([denoise_np.denoise_plane(src[p], None if prev is None else prev[p], S, T, bits) for p in range(len(src))])


def _check(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype
    for p in range(len(want)):
        bad = np.argwhere(got[p] != want[p])
        assert bad.size == 0, (what, NAMES[p] if len(want) == len(NAMES) else p, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_planes_equal_the_numpy_restatement(size, kind):
    H, W = size
    _, dtype, bits = kind
    src, prev = _inputs(H, W, dtype, bits, seed=H * 1000 + W)
    t, p = _dev(src), _dev(prev)
    for S, T in STRENGTHS:
        for hist in (None, prev):
            want = _reference(src, hist, S, T, bits)
            got = _host(denoise.denoise_planes(t, None if hist is None else p, S, T, bits), dtype)
            _check(got, want, (S, T, hist is not None))
            if (S, T) == (0, 0):
                assert np.array_equal(got, src)                # the copy
            lo = np.minimum(src.min(), prev.min()) if hist is not None else src.min()
            hi = np.maximum(src.max(), prev.max()) if hist is not None else src.max()
            assert got.min() >= lo and got.max() <= hi         # no clamp needed: never outside what was read
    # one plane on its own, as a 2-D tensor, gives the same plane
    one = _host(denoise.denoise_planes(t[0], p[0], 8, 8, bits), dtype)
    assert np.array_equal(one, _reference(src[:1], prev[:1], 8, 8, bits)[0])
    assert np.array_equal(_host(t, dtype), src) and np.array_equal(_host(p, dtype), prev)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_a_three_picture_recursion(kind):
    _, dtype, bits = kind
    H, W = 40, 150
    rng = np.random.default_rng(21)
    s = 1 << (bits - 8)
    yy, xx = np.mgrid[0:H, 0:W]
    clean = (100 + 50 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)) * s
    clip = [np.clip(np.rint(clean + rng.normal(0, 3 * s, clean.shape)), 0, (1 << bits) - 1).astype(dtype) for _ in range(3)]
    want = denoise_np.denoise_clip([(c,) for c in clip], 8, 8, bits)
    prev = None
    for i, c in enumerate(clip):
        prev = denoise.denoise_planes(_dev(c), prev, 8, 8, bits)
        got = _host(prev, dtype)
        assert np.array_equal(got, want[i][0]), i
        assert not np.array_equal(got, c)
    assert not np.array_equal(want[2][0], denoise_np.denoise_plane(clip[2], None, 8, 8, bits))      # the history counts


def _pitch(W, how):
    return {"odd": W + 5, "vector": (W + 15) // 16 * 16 + 16, "tail": (W + 7) // 8 * 8 + 8}[how]


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("how", ["odd", "vector", "tail"])
@pytest.mark.parametrize("size", [(50, 46), (33, 130)], ids=["50x46", "33x130"])
def test_strided_planes_leave_the_guard_samples_alone(size, how, kind):
    """row strides above the width and n_planes = 2 at a plane stride, for src, prev and dst, each with its own strides"""
    H, W = size
    _, dtype, bits = kind
    m = (1 << bits) - 1
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5
    rng = np.random.default_rng(7)
    s_row, p_row, d_row = _pitch(W, how), _pitch(W, how) + (16 if how == "vector" else 3), _pitch(W, how)
    src_full = rng.integers(0, m + 1, (2, H + 3, s_row)).astype(dtype)
    prev_full = np.clip(src_full[:, :H, :W].astype(np.int64) + rng.integers(-4, 5, (2, H, W)) * (1 << (bits - 8)), 0, m).astype(dtype)
    prev_full = np.pad(prev_full, ((0, 0), (0, 1), (0, p_row - W)), constant_values=guard)
    dst_full = np.full((2, H + 2, d_row), guard, dtype)
    t, p, o = _dev(src_full), _dev(prev_full), _dev(dst_full)
    for hist in (None, p):
        want = _reference(src_full[:, :H, :W], None if hist is None else prev_full[:, :H, :W], 8, 8, bits)
        o.copy_(_dev(dst_full))
        denoise.denoise_planes(t[:, :H, :W], None if hist is None else p[:, :H, :W], 8, 8, bits, out=o[:, :H, :W])
        got = _host(o, dtype)
        _check(got[:, :H, :W], want, (how, hist is not None))
        mask = np.ones(dst_full.shape, bool)
        mask[:, :H, :W] = False
        assert (got[mask] == guard).all(), "samples outside the destination planes were written"
    assert np.array_equal(_host(t, dtype), src_full) and np.array_equal(_host(p, dtype), prev_full)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("which", ["src", "prev", "dst"])
def test_misaligned_bases_take_the_sample_path(which, kind):
    """a base one sample off a 16-byte boundary, at a width and strides the vector paths would take otherwise"""
    _, dtype, bits = kind
    H, W = 33, 144
    src, prev = _inputs(H, W, dtype, bits, seed=3)
    src, prev = src[0], prev[0]
    want = denoise_np.denoise_plane(src, prev, 8, 8, bits)
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5

    def shifted(a, off):
        flat = np.full(H * W + 32, guard, dtype)
        flat[off:off + H * W] = a.reshape(-1)
        return _dev(flat)

    offs = {k: (1 if k == which else 0) for k in ("src", "prev", "dst")}
    fs, fp, fd = shifted(src, offs["src"]), shifted(prev, offs["prev"]), shifted(np.full((H, W), guard, dtype), offs["dst"])
    view = lambda f, off: f[off:off + H * W].view(H, W)
    assert view(fs, offs["src"]).data_ptr() % 16 == (offs["src"] * src.itemsize)
    denoise.denoise_planes(view(fs, offs["src"]), view(fp, offs["prev"]), 8, 8, bits, out=view(fd, offs["dst"]))
    got = _host(fd, dtype)
    o = offs["dst"]
    assert np.array_equal(got[o:o + H * W].reshape(H, W), want)
    assert (got[:o] == guard).all() and (got[o + H * W:] == guard).all()


def test_a_side_stream():
    H, W, bits = 72, 200, 10
    src, prev = _inputs(H, W, np.uint16, bits, seed=5)
    want = _reference(src, prev, 8, 8, bits)
    base, p = _dev(src), _dev(prev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the input is made on the side stream right before the call and read right after it: only stream order protects them
        t = (base.to(torch.int32) + 0).to(torch.int16)
        got = denoise.denoise_planes(t, p, 8, 8, bits).clone()
        t.zero_()
    side.synchronize()
    _check(_host(got, np.uint16), want, "side stream")


def test_1080p_u8_with_history():
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:1080, 0:1920]
    clean = 128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)
    src, prev = (np.clip(np.rint(clean + rng.normal(0, 3, clean.shape)), 0, 255).astype(np.uint8) for _ in range(2))
    want = denoise_np.denoise_plane(src, prev, 8, 8, 8)
    got = _host(denoise.denoise_planes(_dev(src), _dev(prev), 8, 8, 8), np.uint8)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist())
    assert not np.array_equal(got, src)


def test_the_wrapper_refuses_what_it_cannot_pass():
    t = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        denoise.denoise_planes(t.to(torch.float16), None, 8, 8, 8)
    with pytest.raises(ValueError):
        denoise.denoise_planes(t, torch.zeros((8, 9), dtype=torch.uint8, device="cuda"), 8, 8, 8)
    from dcvc_amd import _lib
    with pytest.raises(_lib.DcvcError):
        denoise.denoise_planes(t, None, 65, 8, 8)
