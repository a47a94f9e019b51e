"""dcvc_crop_stats and dcvc_window_planes on a real MI355X against the numpy restatement (tests/crop_np.py) with ==.

crop_stats: u8, u16 at 10 bits and u16 at 16 bits at 1x1, 2x2, 64x512 (one u8 tile exactly: 64 rows of 32 vectors of 16
samples), 65x513 (one past it both ways), 66x98, 130x1030 on a row stride above W, bases offset by one sample (the element
path), 4096x16 and 16x4096 (many workgroups adding into one word), limit 0 and 255, an all-zero and an all-max plane, and twice
in a row into words pre-filled with garbage: the second call overwrites.

window_planes: crops at every horizontal alignment class (ox 0..17 at u8, 0..9 at u16), pads by negative offsets, a window
hanging over all four sides, two planes on plane strides with distinct fills, 1x1 windows; sentinel samples in the row-stride
gap and behind the last row stay untouched."""
import numpy as np
import pytest
import torch

import crop_np as cnp
from dcvc_amd import crop

pytestmark = pytest.mark.gpu

KINDS = [("u8", np.uint8, 8), ("u10", np.uint16, 10), ("u16", np.uint16, 16)]
SIZES = [(1, 1), (2, 2), (64, 512), (65, 513), (66, 98), (4096, 16), (16, 4096)]
GARBAGE = 0x5A5A5A5A


def _dev(a):
    """numpy u8 / u16 -> CUDA tensor (16-bit samples as int16 storage, which every torch has)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()


def _host(t, dtype):
    if dtype == np.uint8:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _plane(H, W, dtype, bits, seed):
    """dark bars of random sizes around content, every sample within a few code values of the limit somewhere: counts of every
    size from 0 to the side"""
    rng = np.random.default_rng(seed)
    s = 1 << (bits - 8)
    y = rng.integers(0, 60 * s, (H, W))
    t, l = int(rng.integers(0, H // 3 + 1)), int(rng.integers(0, W // 3 + 1))
    y[:t] //= 8
    y[:, :l] //= 8
    y[H - H // 5:] = rng.integers(23 * s, 26 * s + 1, (H // 5, W))
    if bits == 16:
        y[::3] = 65535
    return np.clip(y, 0, (1 << bits) - 1).astype(dtype)


def _words(t):
    return t.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_crop_stats_equals_the_numpy_restatement(kind):
    _, dtype, bits = kind
    for H, W in SIZES:
        y = _plane(H, W, dtype, bits, seed=H * 7 + W)
        t = _dev(y)
        out = torch.empty(H + W, dtype=torch.int32, device="cuda")
        for limit in (24, 0, 255):
            want = cnp.crop_stats(y, limit, bits)
            out.fill_(GARBAGE)
            got = _words(crop.crop_stats(t, limit, bits, out=out))
            assert np.array_equal(got, want), (H, W, limit)
            # again into the words of the first run: overwritten, not added to
            assert np.array_equal(_words(crop.crop_stats(t, limit, bits, out=out)), want), (H, W, limit)
        fresh = crop.crop_stats(t, 24, bits)                       # a buffer of its own, int32
        assert fresh.dtype == torch.int32 and np.array_equal(_words(fresh), cnp.crop_stats(y, 24, bits))
        out64 = torch.full((H + W,), -1, dtype=torch.int64, device="cuda")
        assert np.array_equal(_words(crop.crop_stats(t, 24, bits, out=out64)), cnp.crop_stats(y, 24, bits))
        assert np.array_equal(_host(t, dtype), y)
        if (H, W) == (4096, 16):
            assert cnp.crop_stats(y, 0, bits)[H:].max() > 2048         # 64 workgroups add into every column word


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_crop_stats_on_a_row_stride_above_w_and_misaligned_bases(kind):
    _, dtype, bits = kind
    top = (1 << bits) - 1
    for H, W in [(130, 1030), (66, 98), (65, 513)]:
        y = _plane(H, W, dtype, bits, seed=H + W)
        want = cnp.crop_stats(y, 24, bits)
        for stride, off in ((W + 16 - W % 16 + 16, 0), (W + 5, 0), (W + 16 - W % 16 + 16, 1), (W + 1, 1)):
            # rows of `stride` samples, the plane `off` samples in, everything around it at the largest value: a read outside
            # [0, H) x [0, W) would count
            buf = np.full((H + 1, stride), top, dtype)
            buf[:H, off:off + W] = y
            got = _words(crop.crop_stats(_dev(buf)[:H, off:off + W], 24, bits))
            assert np.array_equal(got, want), (H, W, stride, off)


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_crop_stats_of_flat_planes(kind):
    _, dtype, bits = kind
    H, W = 65, 513
    zero, full = np.zeros((H, W), dtype), np.full((H, W), (1 << bits) - 1, dtype)
    for limit in (0, 24, 255):
        assert not _words(crop.crop_stats(_dev(zero), limit, bits)).any()
        got = _words(crop.crop_stats(_dev(full), limit, bits))
        # 255 << (bits - 8) is below the largest value above 8 bits, and equal to it (not above) at 8
        want = 0 if (bits == 8 and limit == 255) else 1
        assert (got[:H] == want * W).all() and (got[H:] == want * H).all(), limit
    # a sample AT the limit does not count, one above does
    at = np.full((H, W), 24 << (bits - 8), dtype)
    assert not _words(crop.crop_stats(_dev(at), 24, bits)).any()
    assert (_words(crop.crop_stats(_dev(at + 1), 24, bits))[:H] == W).all()


def _guarded(P, H, W, row_stride, plane_gap, dtype, sentinel):
    """[P] planes of H rows on a row stride, plane_gap samples between planes and behind the last, all sentinel"""
    plane = H * row_stride + plane_gap
    return np.full(P * plane, sentinel, dtype), plane


def _run_window(src, out_h, out_w, ox, oy, fills, dtype, src_pad=0, dst_pad=3, dst_off=0):
    """window_planes into a guarded destination -> asserts == the restatement and the guards untouched"""
    P, Hs, Ws = src.shape
    sentinel = 0xA5 if dtype == np.uint8 else 0xA5A5
    # the source on a row stride of its own
    sb, splane = _guarded(P, Hs, Ws + src_pad, Ws + src_pad, 16, dtype, sentinel)
    sv = sb.reshape(P, splane)[:, :Hs * (Ws + src_pad)].reshape(P, Hs, Ws + src_pad)
    sv[:, :, :Ws] = src
    st = _dev(sb).view(P, splane)[:, :Hs * (Ws + src_pad)].view(P, Hs, Ws + src_pad)[:, :, :Ws]
    rs = out_w + dst_pad
    db, dplane = _guarded(P, out_h, rs, rs, 16, dtype, sentinel)
    db = np.concatenate([np.full(dst_off, sentinel, dtype), db])
    dt_all = _dev(db)
    dt = dt_all[dst_off:].view(P, dplane)[:, :out_h * rs].view(P, out_h, rs)[:, :, :out_w]
    got_ret = crop.window_planes(st, out_h, out_w, ox, oy, fills, out=dt)
    assert got_ret is dt
    want = cnp.window_planes(src, out_h, out_w, ox, oy, fills)
    whole = _host(dt_all, dtype)[dst_off:].reshape(P, dplane)
    rows = whole[:, :out_h * rs].reshape(P, out_h, rs)
    assert np.array_equal(rows[:, :, :out_w], want), (src.shape, out_h, out_w, ox, oy)
    assert (rows[:, :, out_w:] == sentinel).all() and (whole[:, out_h * rs:] == sentinel).all(), "a guard sample was written"
    assert (_host(dt_all, dtype)[:dst_off] == sentinel).all()
    assert np.array_equal(_host(st, dtype), src)
    return want


def _src(P, H, W, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 250 if dtype == np.uint8 else 65000, (P, H, W)).astype(dtype)


@pytest.mark.parametrize("name,dtype,last_ox", [("u8", np.uint8, 17), ("u16", np.uint16, 9)])
def test_window_crops_at_every_alignment_class(name, dtype, last_ox):
    src = _src(1, 37, 96, dtype, 1)
    for ox in range(last_ox + 1):
        # vector-capable operands (row strides of whole vectors): the copy is 16-byte where ox's bytes allow
        _run_window(src, 20, 64, ox, 5, [7], dtype, src_pad=0, dst_pad=16 if dtype == np.uint8 else 8)
        # ragged operands: sample by sample
        _run_window(src, 21, 61, ox, 4, [7], dtype, src_pad=1, dst_pad=3)
    # a misaligned destination base
    _run_window(src, 20, 64, 16, 5, [7], dtype, dst_pad=16, dst_off=1)
    # the library's own output buffer
    got = crop.window_planes(_dev(src), 20, 64, 16, 5, [7])
    assert tuple(got.shape) == (1, 20, 64) and np.array_equal(_host(got, dtype), src[:, 5:25, 16:80])
    got = crop.window_planes(_dev(src[0]), 20, 64, 16, 5, 7)
    assert tuple(got.shape) == (20, 64) and np.array_equal(_host(got, dtype), src[0, 5:25, 16:80])


@pytest.mark.parametrize("name,dtype", [("u8", np.uint8), ("u16", np.uint16)])
def test_window_pads_and_hangs_over(name, dtype):
    src = _src(1, 20, 64, dtype, 2)
    for ox, oy in ((0, -6), (-16, 0), (-16, -6), (-5, -3), (-1, -1)):
        want = _run_window(src, 20 - 2 * oy, 64 - 2 * ox, ox, oy, [200], dtype, dst_pad=16 + 2 * ox % 16)
        assert np.array_equal(want[:, -oy:20 - oy, -ox:64 - ox], src)
    # pad(crop(x)) gives x's inside back between the bars
    big = _src(1, 48, 96, dtype, 3)
    inner = _run_window(big, 28, 96, 0, 10, [0], dtype, dst_pad=0)
    back = _run_window(inner, 48, 96, 0, -10, [16], dtype, dst_pad=0)
    assert np.array_equal(back[:, 10:38], big[:, 10:38]) and (back[:, :10] == 16).all() and (back[:, 38:] == 16).all()
    # over all four sides at once, aligned and not; and a window that misses the source altogether
    _run_window(src, 40, 128, -32, -9, [9], dtype, dst_pad=0)
    _run_window(src, 33, 99, -17, -5, [9], dtype)
    miss = _run_window(src, 8, 40, 70, 2, [9], dtype)
    assert (miss == 9).all()
    miss = _run_window(src, 8, 40, 2, -30, [9], dtype)
    assert (miss == 9).all()
    # a mixture: cropped on the left and the top, padded on the right and the bottom
    _run_window(src, 30, 80, 16, 5, [9], dtype, dst_pad=0)
    _run_window(src, 30, 80, 13, 5, [9], dtype)


@pytest.mark.parametrize("name,dtype", [("u8", np.uint8), ("u16", np.uint16)])
def test_window_of_two_planes_with_distinct_fills_and_of_one_sample(name, dtype):
    top = 255 if dtype == np.uint8 else 65535
    src = _src(2, 18, 48, dtype, 4)
    want = _run_window(src, 30, 80, -16, -6, [0, top], dtype, dst_pad=0)
    assert (want[0, :6] == 0).all() and (want[1, :6] == top).all()
    _run_window(src, 30, 81, -15, -6, [3, 4], dtype)
    _run_window(src, 10, 32, 16, 4, [3, 4], dtype, dst_pad=0)
    # more planes than one launch carries fill values for
    many = _src(19, 6, 20, dtype, 5)
    _run_window(many, 9, 24, -2, -1, list(range(19)), dtype)
    # 1 x 1 windows: a sample of the source, and the fill
    one = _run_window(src, 1, 1, 47, 17, [1, 2], dtype)
    assert one[0, 0, 0] == src[0, 17, 47] and one[1, 0, 0] == src[1, 17, 47]
    assert _run_window(src, 1, 1, 48, 17, [1, 2], dtype).ravel().tolist() == [1, 2]
    assert _run_window(src[:, :1, :1], 1, 1, 0, 0, [1, 2], dtype).ravel().tolist() == src[:, 0, 0].tolist()


def test_the_wrappers_argument_errors():
    t = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        crop.crop_stats(t.float(), 24, 8)
    with pytest.raises(ValueError):
        crop.crop_stats(t[None], 24, 8)
    with pytest.raises(ValueError):
        crop.crop_stats(t, 24, 8, out=torch.zeros(15, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        crop.window_planes(t, 4, 4, 0, 0, [1, 2])
    with pytest.raises(TypeError):
        crop.window_planes(t.half(), 4, 4, 0, 0, 0)
    from dcvc_amd._lib import DcvcError
    with pytest.raises(DcvcError, match="limit must be in 0..255"):
        crop.crop_stats(t, 256, 8)
    with pytest.raises(DcvcError, match="fill value 256"):
        crop.window_planes(t, 4, 4, 0, 0, 256)
