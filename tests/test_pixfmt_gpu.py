"""dcvc_pix_to_x / dcvc_x_to_pix on a real MI355X, bit for bit against the numpy restatement (tests/pixfmt_np.py): all four
formats at 8, 10 and 16 bits; sizes on the element path and on the vector path, one thread to several workgroups; ldx 3 and 24
(a chunk slot: channels 3..23 untouched); row_pixels W, W + 8 and W + 1; bases aligned and offset by one sample; every sample
code; every fp16 bit pattern as x_hat; P010 sources with non-zero low bits; guard bands around every output; and YUV420P /
NV12 against the existing dcvc_yuv420_to_x, dcvc_x_to_yuv420, dcvc_yuv420p16_to_x and dcvc_x_to_yuv420p16, which run the same
two kernels behind separate plane pointers: those entries with planes allocated apart and offset, every subset of
dcvc_x_to_yuv420's four outputs, and dcvc_x_to_yuv420p16 with one output."""
import ctypes

import numpy as np
import pytest
import torch

import pixfmt_np as pn
from dcvc_amd import _lib, pixfmt

pytestmark = pytest.mark.gpu

vp, ci = ctypes.c_void_p, ctypes.c_int
GUARD = 64              # elements either side of every output: keeps the body's alignment
SENT16, SENT8, SENT32 = 0x5A5B, 0x5B, 0x5A5B5C5D
SIZES = [(2, 2), (6, 10), (16, 24), (18, 40), (130, 72)]       # H x W: one thread; element path; vector path; several workgroups
BITS = [8, 10, 16]


def _f(name, sig):
    return _lib.fn(name, ci, sig)


def _st():
    return vp(torch.cuda.current_stream().cuda_stream)


def _np_int(a):
    """numpy unsigned / fp16 / fp32 array -> the same bits in a dtype torch takes"""
    return a.view({1: np.uint8, 2: np.int16, 4: np.int32}[a.dtype.itemsize])


class Out:
    """an output buffer of n elements behind `off` extra elements, sentinels all round"""

    def __init__(self, n, itemsize, off=0):
        self.n, self.off, self.es = n, off, itemsize
        dt, self.sent = {1: (torch.uint8, SENT8), 2: (torch.int16, SENT16), 4: (torch.int32, SENT32)}[itemsize]
        self.buf = torch.full((GUARD + off + n + GUARD,), self.sent, dtype=dt, device="cuda")

    def ptr(self):
        return vp(self.buf.data_ptr() + (GUARD + self.off) * self.es)

    def body(self, view):
        """the n elements as numpy `view` dtype, after checking the guard bands"""
        a = self.buf.cpu().numpy()
        lo = GUARD + self.off
        assert np.all(a[:lo] == self.sent) and np.all(a[lo + self.n:] == self.sent), "wrote outside the output"
        return a[lo:lo + self.n].view(view)


def _src(pic, off=0):
    """the picture on the device behind `off` samples -> (tensor that owns it, pointer)"""
    t = torch.zeros(pic.size + 16, dtype=torch.uint8 if pic.dtype == np.uint8 else torch.int16, device="cuda")
    t[off:off + pic.size] = torch.from_numpy(_np_int(pic).copy()).cuda()
    return t, vp(t.data_ptr() + off * pic.dtype.itemsize)


def gpu_to_x(pic, fmt, bits, H, W, ldx=3, off=0):
    """-> (x [H W, 3] as uint16 bits, planar samples), with every untouched element checked"""
    fn = _f("dcvc_pix_to_x", [vp, ci, ci, ci, ci, vp, ci, vp, vp])
    keep, sp = _src(pic, off)
    xo = Out((H * W - 1) * ldx + 3, 2, off)
    po = Out(pic.size, pic.dtype.itemsize, off)
    _lib.check(fn(sp, fmt, bits, H, W, xo.ptr(), ldx, po.ptr(), _st()))
    torch.cuda.synchronize()
    xb = xo.body(np.uint16)
    idx = (np.arange(H * W)[:, None] * ldx + np.arange(3)).ravel()
    rest = np.ones(xb.size, bool)
    rest[idx] = False
    assert np.all(xb[rest] == SENT16), "channels beyond the first three of a pixel were written"
    return xb[idx].reshape(H * W, 3), po.body(pic.dtype)


def gpu_from_x(x_hat, H, W, fmt, bits, off=0):
    """x_hat [Hp, Wp, 3] fp16 numpy -> (dist32 as uint32 bits, samples)"""
    fn = _f("dcvc_x_to_pix", [vp, ci, ci, ci, ci, ci, vp, vp, vp])
    flat = np.ascontiguousarray(x_hat).reshape(-1)
    keep, xp = _src(flat.view(np.uint16), off)
    n = pn.picture_samples(fmt, H, W)
    do, so = Out(n, 4, off), Out(n, 1 if bits == 8 else 2, off)
    _lib.check(fn(xp, x_hat.shape[1], H, W, fmt, bits, do.ptr(), so.ptr(), _st()))
    torch.cuda.synchronize()
    return do.body(np.uint32), so.body(pn.dtype(bits))


def _picture(fmt, bits, H, W, seed=0):
    rng = np.random.default_rng(seed)
    pic = rng.integers(0, 1 << bits, pn.picture_samples(fmt, H, W)).astype(pn.dtype(bits))
    s = pn.shift(fmt, bits)
    return (pic << s) | rng.integers(0, 1 << s, pic.size).astype(pic.dtype) if s else pic      # P010: non-zero low bits


def _x_hat(Hp, Wp, seed=1):
    rng = np.random.default_rng(seed)
    x = (rng.random((Hp, Wp, 3), dtype=np.float32) * np.float32(1.3) - np.float32(0.65)).astype(np.float16)
    x[0, 0] = [np.nan, np.inf, -np.inf]
    return x


def _bits16(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.mark.parametrize("H,W", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("fmt", pn.FORMATS)
def test_pix_to_x(fmt, bits, H, W):
    pic = _picture(fmt, bits, H, W)
    want_x = _bits16(pn.to_x(pic, fmt, bits, H, W)).reshape(H * W, 3)
    want_p = pn.planar(pic, fmt, bits, H, W)
    for ldx, off in ((3, 0), (24, 0), (3, 1), (5, 1)):
        x, planar = gpu_to_x(pic, fmt, bits, H, W, ldx, off)
        assert np.array_equal(x, want_x), (ldx, off)
        assert np.array_equal(planar, want_p), (ldx, off)


@pytest.mark.parametrize("H,W", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("fmt", pn.FORMATS)
def test_x_to_pix(fmt, bits, H, W):
    for extra, off in ((0, 0), (8, 0), (1, 0), (0, 1)):
        x_hat = _x_hat(H + 2, W + extra)
        want_d, want_s = pn.from_x(x_hat, H, W, fmt, bits)
        dist, samples = gpu_from_x(x_hat, H, W, fmt, bits, off)
        assert np.array_equal(dist, want_d.view(np.uint32)), (extra, off)
        assert np.array_equal(samples, want_s), (extra, off)


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("fmt", pn.FORMATS)
def test_every_sample_code(fmt, bits):
    H = W = 256
    for start in (7, 7 + 32768):          # 4:2:0 at 16 bits: two pictures hold every code in chroma
        pic = pn.all_codes(fmt, bits, H, W, low_bits=0x2B, chroma_start=start)
        y, c = pn.unpack(pic, fmt, bits, H, W)
        assert len(np.unique(y)) == 1 << bits and (bits == 16 or len(np.unique(c)) == 1 << bits)
        x, planar = gpu_to_x(pic, fmt, bits, H, W)
        assert np.array_equal(x, _bits16(pn.to_x(pic, fmt, bits, H, W)).reshape(H * W, 3))
        assert np.array_equal(planar, pn.planar(pic, fmt, bits, H, W))


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("fmt", pn.FORMATS)
def test_every_fp16_pattern_as_x_hat(fmt, bits):
    x_hat = pn.all_halfs()
    want_d, want_s = pn.from_x(x_hat, 256, 256, fmt, bits)
    dist, samples = gpu_from_x(x_hat, 256, 256, fmt, bits)
    assert np.array_equal(dist, want_d.view(np.uint32))
    assert np.array_equal(samples, want_s)


def _old_to_x(y, uv, bits):
    H, W = y.shape
    yd, uvd = (torch.from_numpy(_np_int(np.ascontiguousarray(p)).copy()).cuda() for p in (y, uv))
    x = torch.empty((H, W, 3), dtype=torch.float16, device="cuda")
    if bits == 8:
        fn = _f("dcvc_yuv420_to_x", [vp, vp, ci, ci, vp, ci, vp])
        _lib.check(fn(vp(yd.data_ptr()), vp(uvd.data_ptr()), H, W, vp(x.data_ptr()), 3, _st()))
    else:
        fn = _f("dcvc_yuv420p16_to_x", [vp, vp, ci, ci, ci, vp, ci, vp])
        _lib.check(fn(vp(yd.data_ptr()), vp(uvd.data_ptr()), H, W, bits, vp(x.data_ptr()), 3, _st()))
    return _bits16(x.cpu().numpy()).reshape(H * W, 3)


def _old_from_x(x_hat, H, W, bits):
    """-> (dist as fp32 values, flat; samples, flat planar)"""
    xd = torch.from_numpy(x_hat).cuda()
    n = H * W * 3 // 2
    if bits == 8:
        fn = _f("dcvc_x_to_yuv420", [vp, ci, ci, ci, vp, vp, vp, vp, vp])
        p16 = torch.empty(n, dtype=torch.float16, device="cuda")
        p8 = torch.empty(n, dtype=torch.uint8, device="cuda")
        _lib.check(fn(vp(xd.data_ptr()), x_hat.shape[1], H, W, vp(p16.data_ptr()), vp(p16.data_ptr() + 2 * H * W), vp(p8.data_ptr()),
                      vp(p8.data_ptr() + H * W), _st()))
        return p16.float().cpu().numpy(), p8.cpu().numpy()
    fn = _f("dcvc_x_to_yuv420p16", [vp, ci, ci, ci, ci, vp, vp, vp])
    d = torch.empty(n, dtype=torch.float32, device="cuda")
    s = torch.empty(n, dtype=torch.int16, device="cuda")
    _lib.check(fn(vp(xd.data_ptr()), x_hat.shape[1], H, W, bits, vp(d.data_ptr()), vp(s.data_ptr()), _st()))
    return d.cpu().numpy(), s.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("bits", BITS)
def test_420_layouts_equal_the_existing_kernels(bits):
    for H, W in ((6, 10), (18, 40)):
        planar = _picture(pn.YUV420P, bits, H, W, seed=4)
        y, uv = pn.unpack(planar, pn.YUV420P, bits, H, W)
        want = _old_to_x(y, uv, bits)
        nv = pn.pack(y, uv, pn.NV12, bits) | (0x15 if bits == 10 else 0)
        assert np.array_equal(gpu_to_x(planar, pn.YUV420P, bits, H, W)[0], want)
        x, de = gpu_to_x(nv, pn.NV12, bits, H, W)
        assert np.array_equal(x, want) and de.tobytes() == planar.tobytes()            # the de-interleaved source
    for x_hat, H, W in ((_x_hat(20, 48), 18, 40), (_x_hat(8, 11), 6, 10), (pn.all_halfs(), 256, 256)):
        want_d, want_s = _old_from_x(x_hat, H, W, bits)
        for fmt in (pn.YUV420P, pn.NV12):
            dist, samples = gpu_from_x(x_hat, H, W, fmt, bits)
            assert np.array_equal(dist, want_d.view(np.uint32)), fmt
            ys, cs = pn.unpack(samples, fmt, bits, H, W)
            assert np.concatenate([ys.ravel(), cs.ravel()]).astype(samples.dtype).tobytes() == want_s.tobytes(), fmt


PLANE_SIZES = SIZES[:4]        # one thread; element path; vector path; several rows


def _planes_to_x(y, uv, bits, ldx, ch, uv_off):
    """dcvc_yuv420_to_x / dcvc_yuv420p16_to_x with y and uv allocated apart, uv behind uv_off samples, x at channel offset ch of
    pixels of ldx halfs -> x [H W, 3] as uint16 bits, with every other element of x checked"""
    H, W = y.shape
    keep_y, yp = _src(np.ascontiguousarray(y).ravel())
    keep_uv, up = _src(np.ascontiguousarray(uv).ravel(), uv_off)
    xo = Out((H * W - 1) * ldx + 3, 2, ch)
    if bits == 8:
        _lib.check(_f("dcvc_yuv420_to_x", [vp, vp, ci, ci, vp, ci, vp])(yp, up, H, W, xo.ptr(), ldx, _st()))
    else:
        _lib.check(_f("dcvc_yuv420p16_to_x", [vp, vp, ci, ci, ci, vp, ci, vp])(yp, up, H, W, bits, xo.ptr(), ldx, _st()))
    torch.cuda.synchronize()
    xb = xo.body(np.uint16)
    idx = (np.arange(H * W)[:, None] * ldx + np.arange(3)).ravel()
    rest = np.ones(xb.size, bool)
    rest[idx] = False
    assert np.all(xb[rest] == SENT16), "x was written outside the three channels"
    return xb[idx].reshape(H * W, 3)


@pytest.mark.parametrize("H,W", PLANE_SIZES, ids=["%dx%d" % s for s in PLANE_SIZES])
@pytest.mark.parametrize("bits", BITS)
def test_separate_planes_to_x(bits, H, W):
    pic = _picture(pn.YUV420P, bits, H, W, seed=5)
    y, uv = pn.unpack(pic, pn.YUV420P, bits, H, W)
    want = _bits16(pn.to_x(pic, pn.YUV420P, bits, H, W)).reshape(H * W, 3)
    for uv_off in (0, 1):                      # both planes 16-B aligned; uv not 8-B aligned
        for ldx, ch in ((3, 0), (24, 15)):     # one picture; a chunk slot
            assert np.array_equal(_planes_to_x(y, uv, bits, ldx, ch, uv_off), want), (uv_off, ldx, ch)


def _x_to_yuv420(x_hat, H, W, mask):
    """dcvc_x_to_yuv420 with the outputs of `mask` (bit 0: y16, 1: uv16, 2: y8, 3: uv8) non-null -> their contents (None for a
    null one), guard bands checked"""
    keep, xp = _src(np.ascontiguousarray(x_hat).reshape(-1).view(np.uint16))
    ny, nc = H * W, H * W // 2
    outs = [Out(n, es) if mask >> k & 1 else None for k, (n, es) in enumerate(((ny, 2), (nc, 2), (ny, 1), (nc, 1)))]
    fn = _f("dcvc_x_to_yuv420", [vp, ci, ci, ci, vp, vp, vp, vp, vp])
    _lib.check(fn(xp, x_hat.shape[1], H, W, *[o.ptr() if o else None for o in outs], _st()))
    torch.cuda.synchronize()
    return [o.body(v) if o else None for o, v in zip(outs, (np.uint16, np.uint16, np.uint8, np.uint8))]


def _want_yuv420(x_hat, H, W):
    """pn.from_x at (YUV420P, 8): the fp32 planes cast to fp16 (exact) and the samples, as [y16, uv16, y8, uv8]"""
    d, s = pn.from_x(x_hat, H, W, pn.YUV420P, 8)
    d16 = d.astype(np.float16)
    assert np.array_equal(d16.astype(np.float32), d)
    return [_bits16(d16[:H * W]), _bits16(d16[H * W:]), s[:H * W], s[H * W:]]


@pytest.mark.parametrize("H,W", PLANE_SIZES, ids=["%dx%d" % s for s in PLANE_SIZES])
def test_x_to_yuv420_every_subset_of_outputs(H, W):
    for extra in (0, 8, 1):
        x_hat = _x_hat(H + 2, W + extra, seed=6)
        full = _x_to_yuv420(x_hat, H, W, 15)
        for got, want in zip(full, _want_yuv420(x_hat, H, W)):
            assert np.array_equal(got, want), extra
        for mask in range(1, 15):
            for k, got in enumerate(_x_to_yuv420(x_hat, H, W, mask)):
                assert (got is None) == (not mask >> k & 1)
                assert got is None or np.array_equal(got, full[k]), (extra, mask, k)


def test_x_to_yuv420_every_fp16_pattern():
    x_hat = pn.all_halfs()
    for got, want in zip(_x_to_yuv420(x_hat, 256, 256, 15), _want_yuv420(x_hat, 256, 256)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("H,W", PLANE_SIZES, ids=["%dx%d" % s for s in PLANE_SIZES])
@pytest.mark.parametrize("bits", [10, 16])
def test_x_to_yuv420p16_one_output(bits, H, W):
    x_hat = _x_hat(H + 2, W, seed=7)
    want_d, want_s = pn.from_x(x_hat, H, W, pn.YUV420P, bits)
    keep, xp = _src(np.ascontiguousarray(x_hat).reshape(-1).view(np.uint16))
    fn = _f("dcvc_x_to_yuv420p16", [vp, ci, ci, ci, ci, vp, vp, vp])
    n = H * W * 3 // 2
    for dist, yuv in ((Out(n, 4), None), (None, Out(n, 2)), (None, Out(n, 2, 1))):      # dist only; yuv only; yuv behind one sample
        _lib.check(fn(xp, x_hat.shape[1], H, W, bits, dist.ptr() if dist else None, yuv.ptr() if yuv else None, _st()))
        torch.cuda.synchronize()
        if dist:
            assert np.array_equal(dist.body(np.uint32), want_d.view(np.uint32))
        else:
            assert np.array_equal(yuv.body(np.uint16), want_s), yuv.off


def test_python_wrappers():
    H, W, bits, fmt = 18, 40, 10, pixfmt.DCVC_PIX_YUV422P
    assert pixfmt.picture_samples(fmt, H, W) == pn.picture_samples(fmt, H, W)
    assert pixfmt.plane_shapes(fmt, H, W) == pn.plane_shapes(fmt, H, W)
    pic = _picture(fmt, bits, H, W)
    x, planar = pixfmt.to_x(torch.from_numpy(pic.view(np.int16)).cuda(), fmt, bits, H, W, planar=True)
    assert np.array_equal(_bits16(x.cpu().numpy()), _bits16(pn.to_x(pic, fmt, bits, H, W)))
    x_hat = _x_hat(32, 48)
    dist, samples = pixfmt.from_x(torch.from_numpy(x_hat).cuda(), H, W, fmt, bits)
    want_d, want_s = pn.from_x(x_hat, H, W, fmt, bits)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), want_d.view(np.uint32))
    assert np.array_equal(samples.view(torch.int16).cpu().numpy().view(np.uint16), want_s)
    # PSNR of a picture against itself, and against the decoded planes: dcvc_sse on what the two kernels wrote
    p = pixfmt.psnr(planar, dist, fmt, bits, H, W)
    sy, sc = (a.astype(np.float64) for a in pn.unpack(pic, fmt, bits, H, W))
    dy, dc = want_d[:H * W].reshape(H, W).astype(np.float64), want_d[H * W:].reshape(2, H, W // 2).astype(np.float64)
    mse = [((sy - dy) ** 2).mean(), ((sc[0] - dc[0]) ** 2).mean(), ((sc[1] - dc[1]) ** 2).mean()]
    want_p = [10 * np.log10(1023.0 ** 2 / m) for m in mse]
    assert p[1:] == pytest.approx(want_p, rel=1e-12) and p[0] == pytest.approx((6 * want_p[0] + want_p[1] + want_p[2]) / 8, rel=1e-12)
    with pytest.raises(ValueError):
        pixfmt.to_x(torch.from_numpy(pic.view(np.int16)).cuda(), fmt, 8, H, W)
