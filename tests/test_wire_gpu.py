"""dcvc_wire_unpack / dcvc_wire_pack on a real MI355X against the numpy restatement (tests/wire_np.py) with ==: every format at
every depth it has, sizes from one thread to several workgroups on the element path and on the vector path, v210 rows with a
partial last group of 2 and of 4 pixels, an exactly full 128-byte block and one group into the next block; seeded samples over
the full code range; garbage in every bit unpack ignores; pack into a 0xA5 destination inside a larger buffer (ignored bits
and padding zero, nothing outside the picture written); bases 16-byte aligned and offset by one byte / one sample; a side
stream; refusals with real device pointers; and the Python wrappers (dcvc_amd/wirefmt.py)."""
import ctypes

import numpy as np
import pytest
import torch

import wire_np as wn
from dcvc_amd import _lib, wirefmt

pytestmark = pytest.mark.gpu

vp, ci = ctypes.c_void_p, ctypes.c_int
GUARD = 256               # bytes either side of every buffer: keeps the body's alignment
FILL = 0xA5
# H x W: one thread; element path (W % 8 != 0); vector path; ... several workgroups (34 x 72: 306 threads of 8 pixels)
SIZES = [(2, 2), (2, 6), (4, 8), (4, 24), (6, 40), (16, 96), (34, 72)]
# v210: a last group of 4 and of 2 pixels, a full 128-byte block, one group into the next block, two workgroups with a thread
# of 16 pixels and a thread of padding in every row
V210_SIZES = [(4, 46), (4, 48), (6, 50), (2, 94), (18, 352)]
CASES = [(w, b) for w in sorted(wn.DEPTHS) for b in wn.DEPTHS[w]]
SIG = [vp, ci, ci, ci, ci, vp, vp]


def _sizes(wire):
    return SIZES + (V210_SIZES if wire == wn.V210 else [])


def _st():
    return vp(torch.cuda.current_stream().cuda_stream)


class Buf:
    """n bytes on the device behind GUARD + off bytes, 0xA5 all round (and inside, unless `data` is given)"""

    def __init__(self, n, off=0, data=None):
        self.n, self.off = n, off
        self.t = torch.full((GUARD + off + n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        if data is not None:
            d = np.ascontiguousarray(data).view(np.uint8).ravel()
            assert d.size == n
            self.t[GUARD + off:GUARD + off + n] = torch.from_numpy(d.copy()).cuda()

    def ptr(self):
        return vp(self.t.data_ptr() + GUARD + self.off)

    def body(self):
        """the n bytes, after checking that nothing around them was written"""
        a = self.t.cpu().numpy()
        lo = GUARD + self.off
        assert np.all(a[:lo] == FILL) and np.all(a[lo + self.n:] == FILL), "wrote outside the destination"
        return a[lo:lo + self.n]


def gpu_unpack(p, wire, bits, H, W, misaligned=False):
    es = 1 if bits == 8 else 2
    src = Buf(p.size, 1 if misaligned else 0, p)
    dst = Buf(wn.carrier_samples(wire, H, W) * es, es if misaligned else 0)
    _lib.check(_lib.fn("dcvc_wire_unpack", ci, SIG)(src.ptr(), wire, bits, H, W, dst.ptr(), _st()))
    torch.cuda.synchronize()
    return dst.body().view(wn.dtype(bits))


def gpu_pack(c, wire, bits, H, W, misaligned=False):
    src = Buf(c.nbytes, c.itemsize if misaligned else 0, c)
    dst = Buf(wn.picture_bytes(wire, bits, H, W), 1 if misaligned else 0)
    _lib.check(_lib.fn("dcvc_wire_pack", ci, SIG)(src.ptr(), wire, bits, H, W, dst.ptr(), _st()))
    torch.cuda.synchronize()
    return dst.body()


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("wire,bits", CASES, ids=["%d-%d" % c for c in CASES])
def test_pack_and_unpack_equal_numpy(wire, bits, misaligned):
    rng = np.random.default_rng(100 * wire + bits)
    for H, W in _sizes(wire):
        c = wn.random_carrier(rng, wire, bits, H, W)
        want = wn.pack(c, wire, bits, H, W)
        mask = wn.ignored_mask(wire, bits, H, W)
        # pack: the picture's bytes with ignored bits and padding zero, into a destination that held 0xA5
        got = gpu_pack(c, wire, bits, H, W, misaligned)
        assert np.array_equal(got, want), (H, W)
        assert not (got & mask).any(), (H, W)
        # unpack: random garbage in every ignored bit does not change the result
        dirty = want | (rng.integers(0, 256, want.size, dtype=np.uint8) & mask)
        assert np.array_equal(wn.unpack(dirty, wire, bits, H, W), c)
        assert np.array_equal(gpu_unpack(dirty, wire, bits, H, W, misaligned), c), (H, W)
        assert np.array_equal(gpu_unpack(want, wire, bits, H, W, misaligned), c), (H, W)


def test_samples_above_max_val():
    """unpack neither checks nor masks (the library's rule); pack keeps a bad sample out of its neighbours"""
    rng = np.random.default_rng(7)
    H, W = 4, 24
    c = rng.integers(0, 65536, wn.carrier_samples(wn.V210, H, W), dtype=np.uint32).astype(np.uint16)
    assert np.array_equal(gpu_pack(c, wn.V210, 10, H, W), wn.pack(c & 1023, wn.V210, 10, H, W))
    assert np.array_equal(gpu_pack(c, wn.YUY2, 10, H, W), wn.pack(c, wn.YUY2, 10, H, W))          # (s << 6) & 0xFFFF
    p = rng.integers(0, 256, wn.picture_bytes(wn.NV16, 12, H, W), dtype=np.uint8)
    assert np.array_equal(gpu_unpack(p, wn.NV16, 12, H, W), wn.unpack(p, wn.NV16, 12, H, W))


def test_every_v210_code_and_every_u16_pattern():
    H, W = 2, 1024
    codes = np.arange(1024, dtype=np.uint16)
    c = np.concatenate([codes, codes[::-1], codes, (codes + 7) % 1024]).astype(np.uint16)
    p = gpu_pack(c, wn.V210, 10, H, W)
    assert np.array_equal(p, wn.pack(c, wn.V210, 10, H, W)) and np.array_equal(gpu_unpack(p, wn.V210, 10, H, W), c)
    H, W = 128, 256
    p = np.arange(65536, dtype="<u2").view(np.uint8)
    c = gpu_unpack(p, wn.YUY2, 16, H, W)
    assert np.array_equal(c, wn.unpack(p, wn.YUY2, 16, H, W)) and np.array_equal(gpu_pack(c, wn.YUY2, 16, H, W), p)


@pytest.mark.parametrize("name,bits", [("v210", 10), ("uyvy", 8), ("nv21", 8), ("yuy2", 10), ("nv16", 12)])
def test_the_wrappers_on_a_side_stream(name, bits):
    wire = wirefmt.WIRE[name]
    assert wire == wn.NAMES[name] and wirefmt.carrier(wire) == wn.carrier(wire)
    H, W = 18, 352
    assert wirefmt.picture_bytes(wire, bits, H, W) == wn.picture_bytes(wire, bits, H, W)
    rng = np.random.default_rng(11 + wire)
    c = wn.random_carrier(rng, wire, bits, H, W)
    want = wn.pack(c, wire, bits, H, W)
    base = torch.from_numpy(want.copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the input is made on the side stream right before the call and overwritten right after it: only stream order protects it
        t = (base.to(torch.int32) + 0).to(torch.uint8)
        carrier = wirefmt.unpack(t, wire, bits, H, W)
        t.fill_(FILL)
        u = carrier.clone()
        packed = wirefmt.pack(u, wire, bits, H, W)
        u.zero_()
    side.synchronize()
    assert carrier.numel() == c.size and packed.dtype == torch.uint8
    got = carrier.cpu().numpy() if bits == 8 else carrier.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, c)
    assert np.array_equal(packed.cpu().numpy(), want)


def test_the_wrappers_check_their_arguments():
    H, W = 4, 24
    good = torch.zeros(wn.picture_bytes(wn.V210, 10, H, W), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        wirefmt.unpack(good[:-1], wn.V210, 10, H, W)
    with pytest.raises(ValueError):
        wirefmt.unpack(good.cpu(), wn.V210, 10, H, W)
    with pytest.raises(ValueError):
        wirefmt.unpack(good.view(torch.int16), wn.V210, 10, H, W)
    with pytest.raises(ValueError):
        wirefmt.pack(torch.zeros(2 * H * W, dtype=torch.uint8, device="cuda"), wn.V210, 10, H, W)         # u16 samples wanted
    with pytest.raises(ValueError):
        wirefmt.pack(torch.zeros(2 * H * W - 1, dtype=torch.int16, device="cuda"), wn.V210, 10, H, W)
    with pytest.raises(_lib.DcvcError):
        wirefmt.picture_bytes(wn.V210, 8, H, W)
    with pytest.raises(_lib.DcvcError):
        wirefmt.carrier(5)


def test_refusals_with_device_pointers_leave_the_destination_untouched():
    H, W = 16, 24
    n = wn.picture_bytes(wn.UYVY, 8, H, W)
    src = Buf(n, 0, np.zeros(n, np.uint8))
    dst = Buf(2 * n)
    fns = [_lib.fn("dcvc_wire_unpack", ci, SIG), _lib.fn("dcvc_wire_pack", ci, SIG)]
    inside = vp(dst.t.data_ptr() + GUARD + n - 1)             # a source whose last byte is the destination's first
    bad = [(src.ptr(), 5, 8, H, W, dst.ptr()), (src.ptr(), wn.UYVY, 10, H, W, dst.ptr()), (src.ptr(), wn.V210, 8, H, W, dst.ptr()),
           (src.ptr(), wn.UYVY, 8, H - 1, W, dst.ptr()), (src.ptr(), wn.UYVY, 8, H, W + 1, dst.ptr()), (src.ptr(), wn.UYVY, 8, 0, W, dst.ptr()),
           (None, wn.UYVY, 8, H, W, dst.ptr()), (dst.ptr(), wn.UYVY, 8, H, W, dst.ptr()),
           (vp(dst.t.data_ptr() + GUARD - n + 1), wn.UYVY, 8, H, W, dst.ptr()), (inside, wn.UYVY, 8, H, W, vp(inside.value + n - 1))]
    for fn in fns:
        for a in bad:
            assert fn(*a, _st()) < 0, a
            assert "wire" in _lib.lib().dcvc_last_error().decode()
        assert fn(src.ptr(), wn.UYVY, 8, H, W, None, _st()) < 0
    torch.cuda.synchronize()
    assert np.all(dst.body() == FILL) and not src.body().any()
    # ranges that touch do not overlap: the destination right behind the source
    pair = Buf(2 * n, 0, np.concatenate([np.arange(n, dtype=np.uint32).astype(np.uint8), np.full(n, FILL, np.uint8)]))
    _lib.check(fns[0](pair.ptr(), wn.UYVY, 8, H, W, vp(pair.t.data_ptr() + GUARD + n), _st()))
    torch.cuda.synchronize()
    both = pair.body()
    assert np.array_equal(both[n:], wn.unpack(both[:n], wn.UYVY, 8, H, W))
