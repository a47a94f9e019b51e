"""The 9..16-bit RGB kernels (rgb_cs.hip behind dcvc_rgb16_to_x_cs / dcvc_x_to_rgb16_cs) on a real MI355X against the numpy
restatement (tests/rgb16_np.py) with ==: x, the fp32 distortion planes as bit patterns, the u16 pixels and the planar copy.
The smallest shapes that reach every path - 6x24 aligned (vector), 6x22 (the tail), a base moved by one sample and a padded
row stride (element), packed and planar sources, ldx 3 and 24, row_pixels > W - through the C ABI on buffers with guard
samples around every output; depths 10, 12 and 16, the three matrices, both ranges and YUV depths 8 and 10 on a grey ramp of
every 10-bit value, 65536 random colours, 0 and max_val and samples above max_val; NaN, the infinities and every other fp16
pattern in x_hat."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rgb16_np
from colour_np import MATRIX_CODE, RANGE_CODE
from dcvc_amd import _lib, rgb

pytestmark = pytest.mark.gpu

vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
DEPTHS = (10, 12, 16)
COMBOS = [(m, r, d) for m in ("bt601", "bt709", "bt2020") for r, d in (("full", 8), ("limited", 8), ("limited", 10))]
GUARD = 64                 # samples in front of and behind every output: a multiple of 8, so the base keeps its alignment
BIG = (256, 264)           # 67584 pixels, rows of a multiple of 8: the ramp, 65536 random colours and the ends of the scale


def _to_x_fn():
    return _lib.fn("dcvc_rgb16_to_x_cs", ci, [vp, ll, ll, ll, ci, ci, ci, vp, ci, vp, ci, ci, ci, vp])


def _to_rgb_fn():
    return _lib.fn("dcvc_x_to_rgb16_cs", ci, [vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, vp])


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _colours(depth):
    """[3, 256, 264] u16: a grey ramp of every 10-bit value (scaled to the depth's codes and, at depth 10, the codes themselves),
    0 and max_val, 1024 samples above max_val (below depth 16) and random colours for the rest (more than 65536)"""
    H, W = BIG
    m = rgb16_np.max_val(depth)
    rng = np.random.default_rng(100 + depth)
    c = rng.integers(0, m + 1, size=(3, H * W), dtype=np.uint16)
    ramp = (np.arange(1024, dtype=np.uint32) << (depth - 10)).astype(np.uint16)
    c[:, :1024] = ramp
    c[:, 1024:1028] = np.array([[0, m, 0, m], [0, m, m, 0], [0, m, 0, 0]], dtype=np.uint16)
    if depth < 16:
        c[:, 1028:2052] = rng.integers(m + 1, 65536, size=(3, 1024), dtype=np.uint16)
        c[:, 2052] = 65535
    c = c.reshape(3, H, W)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _want_x(depth, matrix, range_, yuv_depth):
    x = rgb16_np.rgb16_to_x(_colours(depth), depth, matrix, range_, yuv_depth)
    x.setflags(write=False)
    return x


def _dev16(a):
    """u16 numpy -> int16-storage CUDA tensor"""
    return torch.from_numpy(np.array(a, order="C").view(np.int16)).cuda()


def _host16(t):
    return t.cpu().numpy().view(np.uint16)


def _f16_eq(a, b):
    """bit for bit; a NaN's payload is not part of the definition: NaN must sit where NaN is expected"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~nb])


def _f32_eq(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _guarded(n, dtype, fill, shift=0):
    """a flat buffer of GUARD + shift + n + GUARD elements filled with `fill`; the view of the n in the middle"""
    buf = torch.full((2 * GUARD + shift + n,), fill, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, buf[GUARD + shift:GUARD + shift + n]


def _guards_intact(buf, n, fill, shift=0):
    head, tail = buf[:GUARD + shift], buf[GUARD + shift + n:]
    return bool((head == fill).all()) and bool((tail == fill).all()) and tail.numel() == GUARD


def _run_to_x(c, depth, colour, layout="packed", shift=0, row_pad=0, ldx=3, slot=0, x_shift=0, want_x=True, want_planar=True,
              planar_shift=0):
    """c: [3, H, W] u16 on the host. Returns (x [H, W, 3] fp16 or None, planar [3, H, W] u16 or None) as numpy, after checking
    that nothing outside the outputs was written."""
    _, H, W = c.shape
    matrix, range_, yuv_depth = colour
    if layout == "packed":
        rs, ps, cs = 3 * W + row_pad, 3, 1
        n_src = H * rs
        host = np.full(n_src, 0xABCD, np.uint16)
        rows = host.reshape(H, rs)
        rows[:, :3 * W] = c.transpose(1, 2, 0).reshape(H, 3 * W)
    else:
        rs, ps = W + row_pad, 1
        cs = H * rs
        host = np.full(3 * cs, 0xABCD, np.uint16)
        host.reshape(3, H, rs)[:, :, :W] = c
    src_buf = torch.zeros(shift + host.size, dtype=torch.int16, device="cuda")
    src = src_buf[shift:]
    src.copy_(torch.from_numpy(host.view(np.int16)))
    xb = xv = pb = pv = None
    n_x = (H * W - 1) * ldx + 3 + (ldx - 3 if ldx > 3 else 0)
    if want_x:
        xb, xv = _guarded(n_x, torch.float16, 7.0, x_shift)
    if want_planar:
        pb, pv = _guarded(3 * H * W, torch.int16, 0x5A5A, planar_shift)
    rc = _to_x_fn()(vp(src.data_ptr()), rs, ps, cs, depth, H, W, vp(xv[3 * slot:].data_ptr()) if want_x else None, ldx,
                    vp(pv.data_ptr()) if want_planar else None, MATRIX_CODE[matrix], RANGE_CODE[range_], yuv_depth, _stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    x = planar = None
    if want_x:
        assert _guards_intact(xb, n_x, 7.0, x_shift)
        if ldx == 3:
            x = xv.cpu().numpy().reshape(H, W, 3)
        else:
            full = xv[:H * W * ldx].cpu().numpy().reshape(H, W, ldx)
            x = np.ascontiguousarray(full[..., 3 * slot:3 * slot + 3])
            rest = [k for k in range(ldx) if k // 3 != slot]
            assert (full[..., rest] == 7.0).all()
    if want_planar:
        assert _guards_intact(pb, 3 * H * W, 0x5A5A, planar_shift)
        planar = _host16(pv).reshape(3, H, W)
    assert np.array_equal(_host16(src), host)
    return x, planar


@pytest.mark.parametrize("depth", DEPTHS)
def test_to_x_every_colour_set_every_conversion(depth):
    """the vector path on the big picture, packed, against the restatement for every matrix, range and YUV depth; the planar
    source and the planar copy once per depth"""
    c = _colours(depth)
    H, W = BIG
    src = _dev16(c.transpose(1, 2, 0))
    assert src.data_ptr() % 16 == 0
    for matrix, range_, yuv_depth in COMBOS:
        x = rgb.rgb16_to_x(src, depth, matrix=matrix, range=range_, yuv_depth=yuv_depth)
        assert _f16_eq(x.cpu().numpy(), _want_x(depth, matrix, range_, yuv_depth)), (matrix, range_, yuv_depth)
    x, copy = rgb.rgb16_to_x(_dev16(c), depth, planar=True, matrix="bt2020", range="limited", yuv_depth=10)
    assert _f16_eq(x.cpu().numpy(), _want_x(depth, "bt2020", "limited", 10))
    assert np.array_equal(_host16(copy.view(torch.int16)), c)
    if depth < 16:
        # samples above max_val were neither masked nor refused: they sit at the top of x's scale
        above = (c > rgb16_np.max_val(depth)).all(axis=0)
        full = rgb.rgb16_to_x(src, depth).cpu().numpy()
        assert above.sum() >= 1024 and (full[above][:, 0] == 0.5).all()


PATHS = [
    # name, (H, W) crop, keywords of _run_to_x
    ("vector packed", (6, 24), dict()),
    ("vector planar", (6, 24), dict(layout="planar")),
    ("tail packed", (6, 22), dict()),
    ("tail planar", (6, 22), dict(layout="planar")),
    ("source moved by one sample", (6, 24), dict(shift=1)),
    ("planar source moved by one sample", (6, 24), dict(layout="planar", shift=1)),
    ("padded row stride", (6, 24), dict(row_pad=3)),
    ("padded planar row stride", (6, 24), dict(layout="planar", row_pad=2)),
    ("padded row stride of 8 samples", (6, 24), dict(row_pad=8)),
    ("x moved by one sample", (6, 24), dict(x_shift=1)),
    ("planar copy moved by one sample", (6, 24), dict(planar_shift=1)),
    ("chunk slot 0", (6, 24), dict(ldx=24, slot=0)),
    ("chunk slot 5, planar", (6, 24), dict(ldx=24, slot=5, layout="planar")),
    ("chunk slot 7, tail", (6, 22), dict(ldx=24, slot=7)),
    ("x alone", (6, 24), dict(want_planar=False)),
    ("planar copy alone", (6, 24), dict(want_x=False)),
    ("planar copy alone, tail", (6, 22), dict(want_x=False, layout="planar")),
    ("two blocks", (22, 200), dict()),
    ("two blocks, tail", (22, 198), dict(layout="planar")),
]


@pytest.mark.parametrize("depth", DEPTHS)
def test_to_x_every_path(depth):
    colour = {10: ("bt601", "limited", 8), 12: ("bt2020", "limited", 10), 16: ("bt709", "full", 8)}[depth]
    want_all = _want_x(depth, *colour)
    for name, (H, W), kw in PATHS:
        # the crop starts where the ramp, the ends of the scale and the samples above max_val sit
        c = np.ascontiguousarray(_colours(depth)[:, 3:3 + H, 240 - W:240])
        x, planar = _run_to_x(c, depth, colour, **kw)
        if kw.get("want_x", True):
            assert _f16_eq(x, want_all[3:3 + H, 240 - W:240]), (name, depth)
        if kw.get("want_planar", True):
            assert np.array_equal(planar, c), (name, depth)


# ---------------------------------------------------------------------------------------------------------------- from x
def _x_hat_edges(Hp, Wp, seed):
    rng = np.random.default_rng(seed)
    x_hat = (rng.random((Hp, Wp, 3)) * 1.5 - 0.75).astype(np.float16)
    edges = np.array([-0.5, 0.5, -0.501, 0.499, 0.5005, -0.4995, 0.75, -0.75, 0.0, 0.25, np.nan, np.inf, -np.inf, 2.0, -2.0, 65504.0],
                     dtype=np.float16)
    x_hat[0, :edges.size] = edges[:, None]                  # all three channels
    x_hat[1, :edges.size, 0] = edges[::-1]                  # luma alone
    x_hat[2, :edges.size, 1] = edges                        # Cb alone
    x_hat[3, :edges.size, 2] = edges                        # Cr alone
    return x_hat


def _run_from_x(x_hat, H, W, depth, colour, want_dist=True, want_out=True, dist_shift=0, out_shift=0, x_shift=0):
    """x_hat: [Hp, Wp, 3] fp16 on the host. Returns (dist [3, H, W] fp32 or None, out [H, W, 3] u16 or None) as numpy, after
    checking that nothing outside the outputs was written."""
    matrix, range_, yuv_depth = colour
    Hp, Wp, _ = x_hat.shape
    xb = torch.zeros(x_shift + x_hat.size, dtype=torch.float16, device="cuda")
    xv = xb[x_shift:]
    xv.copy_(torch.from_numpy(x_hat.reshape(-1)))
    db = dv = ob = ov = None
    if want_dist:
        db, dv = _guarded(3 * H * W, torch.float32, -7.0, dist_shift)
    if want_out:
        ob, ov = _guarded(3 * H * W, torch.int16, 0x5A5A, out_shift)
    rc = _to_rgb_fn()(vp(xv.data_ptr()), Wp, H, W, depth, vp(dv.data_ptr()) if want_dist else None,
                      vp(ov.data_ptr()) if want_out else None, MATRIX_CODE[matrix], RANGE_CODE[range_], yuv_depth, _stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    dist = out = None
    if want_dist:
        assert _guards_intact(db, 3 * H * W, -7.0, dist_shift)
        dist = dv.cpu().numpy().reshape(3, H, W)
    if want_out:
        assert _guards_intact(ob, 3 * H * W, 0x5A5A, out_shift)
        out = _host16(ov).reshape(H, W, 3)
    return dist, out


FROM_PATHS = [
    # name, H, W, Hp, Wp, keywords of _run_from_x
    ("vector", 6, 24, 6, 24, dict()),
    ("vector, row_pixels > W", 6, 24, 16, 32, dict()),
    ("tail and crop", 6, 22, 16, 32, dict()),
    ("tail, rows that end with the picture", 6, 22, 6, 22, dict()),
    ("row_pixels no multiple of 8", 6, 24, 6, 26, dict()),
    ("planes moved by one sample", 6, 24, 6, 24, dict(dist_shift=1)),
    ("pixels moved by one sample", 6, 24, 6, 24, dict(out_shift=1)),
    ("x_hat moved by one sample", 6, 24, 6, 24, dict(x_shift=1)),
    ("planes alone", 6, 24, 6, 24, dict(want_out=False)),
    ("pixels alone", 6, 24, 6, 24, dict(want_dist=False)),
    ("pixels alone, tail", 6, 22, 6, 24, dict(want_dist=False)),
    ("two blocks", 22, 200, 32, 208, dict()),
    ("two blocks, tail", 22, 198, 32, 208, dict()),
]


@pytest.mark.parametrize("depth", DEPTHS)
def test_from_x_every_path(depth):
    m = rgb16_np.max_val(depth)
    colour = {10: ("bt601", "limited", 8), 12: ("bt2020", "limited", 10), 16: ("bt709", "full", 8)}[depth]
    for name, H, W, Hp, Wp, kw in FROM_PATHS:
        x_hat = _x_hat_edges(Hp, Wp, 31 * H + W + depth)
        want_dist, want_out = rgb16_np.x_to_rgb16(x_hat, H, W, depth, *colour)
        dist, out = _run_from_x(x_hat, H, W, depth, colour, **kw)
        if kw.get("want_dist", True):
            assert dist.dtype == np.float32 and _f32_eq(dist, want_dist), (name, depth)
        if kw.get("want_out", True):
            assert np.array_equal(out, want_out), (name, depth)
            nan = np.isnan(want_dist).transpose(1, 2, 0)
            assert nan.any() and (out[nan] == 0).all(), (name, depth)
            assert (out == 0).any() and (out == m).any(), (name, depth)


@pytest.mark.parametrize("depth", DEPTHS)
def test_from_x_every_conversion_on_the_round_trip_and_every_fp16_pattern(depth):
    """each matrix, range and YUV depth on the x of the colour set (the wrapper's path) and, once per depth, 256 x 256 x_hat whose
    channels run through all 65536 fp16 patterns (NaN, the infinities, subnormals) in orders of their own"""
    H, W = BIG
    m = rgb16_np.max_val(depth)
    for matrix, range_, yuv_depth in COMBOS:
        x = _want_x(depth, matrix, range_, yuv_depth)
        want_dist, want_out = rgb16_np.x_to_rgb16(x, H, W, depth, matrix, range_, yuv_depth)
        dist, out = rgb.x_to_rgb16(torch.from_numpy(np.array(x)).cuda(), H, W, depth, matrix=matrix, range=range_, yuv_depth=yuv_depth)
        assert dist.dtype == torch.float32 and _f32_eq(dist.cpu().numpy(), want_dist), (matrix, range_, yuv_depth)
        assert np.array_equal(_host16(out.view(torch.int16)), want_out), (matrix, range_, yuv_depth)
        # the channels-last 4-D form the codecs hand over
        dist4, out4 = rgb.x_to_rgb16(torch.from_numpy(np.array(x)).cuda().permute(2, 0, 1).unsqueeze(0), H, W, depth, matrix=matrix, range=range_,
                                     yuv_depth=yuv_depth)
        assert torch.equal(dist4.view(torch.int32), dist.view(torch.int32)) and torch.equal(out4.view(torch.int16), out.view(torch.int16))
    i = np.arange(65536, dtype=np.uint32)
    pat = np.stack([i, 65535 - i, (i * 40503 + 12345) & 65535], axis=-1).astype(np.uint16).reshape(256, 256, 3)
    host = pat.view(np.float16)
    colour = ("bt2020", "limited", 10)
    want_dist, want_out = rgb16_np.x_to_rgb16(host, 256, 256, depth, *colour)
    dist, out = _run_from_x(host, 256, 256, depth, colour)
    assert _f32_eq(dist, want_dist) and np.array_equal(out, want_out)
    nan = np.isnan(want_dist).transpose(1, 2, 0)
    assert nan.any() and (out[nan] == 0).all() and (out == 0).any() and (out == m).any()
    assert (dist == 0).any() and (dist == m).any()


def test_psnr_and_msssim_wrappers_use_the_data_range():
    """psnr_rgb16 from dcvc_sse's sums at max_val against a numpy sum; msssim_rgb16 of a picture against itself is 1"""
    depth, (H, W) = 10, (96, 104)
    c = np.ascontiguousarray(_colours(depth)[:, 100:100 + H, :W]) & 1023
    src = _dev16(c)
    x, copy = rgb.rgb16_to_x(src, depth, planar=True)
    dist, _ = rgb.x_to_rgb16(x, H, W, depth)
    d = c.astype(np.float64) - dist.cpu().numpy().astype(np.float64)
    mse = float((d * d).sum()) / d.size
    want = 10 * np.log10(1023.0 * 1023.0 / mse)
    got = rgb.psnr_rgb16(copy, dist, depth)
    assert abs(got - want) <= 1e-9 * want, (got, want)
    same = rgb.msssim_rgb16(copy, copy.view(torch.int16).float().contiguous(), depth)
    assert abs(same - 1.0) <= 1e-9


def test_stream_order_on_a_non_default_stream():
    depth, colour = 12, ("bt601", "limited", 8)
    H, W = BIG
    kw = dict(matrix=colour[0], range=colour[1], yuv_depth=colour[2])
    want = _want_x(depth, *colour)
    want_dist, want_out = rgb16_np.x_to_rgb16(want, H, W, depth, *colour)
    base = _dev16(_colours(depth).transpose(1, 2, 0))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        src = base + 0                                              # produced on s, consumed on s without a host sync
        x = rgb.rgb16_to_x(src, depth, **kw)
        dist, out = rgb.x_to_rgb16(x, H, W, depth, **kw)
    s.synchronize()
    assert _f16_eq(x.cpu().numpy(), want) and _f32_eq(dist.cpu().numpy(), want_dist)
    assert np.array_equal(_host16(out.view(torch.int16)), want_out)
