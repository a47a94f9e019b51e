"""dcvc_field_match and dcvc_weave_fields on a real MI355X against the numpy restatement (tests/ivtc_np.py) with ==: H in {2, 3,
4, 17, 33} x W in {1, 7, 31, 32, 33, 129, 257} and one 270 x 480 plane (more than one workgroup on both axes for u16: the tile
is 64 rows of 32 vectors), both parities, with and without prev, u8, u16 at 10 bits and u16 at 16 bits with rows alternating 0
and 65535 (the largest per-sample terms), padded strides and bases offset by one sample (the element path), cthresh 0, 9 and 255,
and twice in a row into a buffer pre-filled with garbage. weave_fields over the same sizes with 1 and 2 planes, guard samples
behind W and behind the last plane untouched."""
import numpy as np
import pytest
import torch

import ivtc_np as inp
from dcvc_amd import ivtc

pytestmark = pytest.mark.gpu

HS, WS = (2, 3, 4, 17, 33), (1, 7, 31, 32, 33, 129, 257)
SIZES = [(H, W) for H in HS for W in WS] + [(270, 480)]
KINDS = [("u8", np.uint8, 8), ("u10", np.uint16, 10), ("u16", np.uint16, 16)]
GARBAGE = -0x0123456789ABCDEF


def _dev(a):
    """numpy u8 / u16 -> CUDA tensor (16-bit samples as int16 storage, which every torch has)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()


def _host(t, dtype):
    if dtype == np.uint8:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _planes(H, W, dtype, bits, seed):
    """cur and prev: smooth enough that some samples are combed at cthresh 9 and some are not"""
    rng = np.random.default_rng(seed)
    m, s = (1 << bits) - 1, 1 << (bits - 8)
    base = rng.integers(0, 200 * s, (1, W)) + rng.integers(-14 * s, 14 * s + 1, (H, W))
    cur = np.clip(base, 0, m).astype(dtype)
    prev = np.clip(base + rng.integers(-14 * s, 14 * s + 1, (H, W)), 0, m).astype(dtype)
    return cur, prev


def _row_len(W, pad):
    """a row of W samples, pad more and a guard vector; a multiple of 16 samples for pad 16, so that the vector path meets a ragged row"""
    return (W + pad + 15) // 16 * 16 + 16 if pad == 16 else W + pad + 16


def _words(t):
    return [int(v) for v in t.cpu().tolist()]


_ref = {}


def _want(key, cur, prev, first, cthresh, bits):
    if key not in _ref:
        _ref[key] = inp.field_match(cur, prev, first, cthresh, bits)
    return _ref[key]


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_field_match_equals_the_numpy_restatement(kind):
    name, dtype, bits = kind
    out = torch.empty(8, dtype=torch.int64, device="cuda")
    some = 0
    for H, W in SIZES:
        cur, prev = _planes(H, W, dtype, bits, seed=H * 1000 + W)
        if bits == 16:
            cur[0::2], cur[1::2] = 0, 65535
            prev[0::2], prev[1::2] = 65535, 0
        t, p = _dev(cur), _dev(prev)
        for first in (0, 1):
            for cthresh in (0, 9, 255):
                for hist in (None, prev):
                    want = _want((name, H, W, first, cthresh, hist is not None), cur, hist, first, cthresh, bits)
                    out.fill_(GARBAGE)
                    got = _words(ivtc.field_match(t, None if hist is None else p, first, cthresh, bits, out=out))
                    assert got == want, (H, W, first, cthresh, hist is not None)
                    # again into the words of the first run: the same words
                    assert _words(ivtc.field_match(t, None if hist is None else p, first, cthresh, bits, out=out)) == want
                    some += want[2] > 0 and want[4] < want[2]
        assert _words(ivtc.field_match(t, p, 0, 9, bits)) == _want((name, H, W, 0, 9, True), cur, prev, 0, 9, bits)      # a buffer of its own
        assert np.array_equal(_host(t, dtype), cur) and np.array_equal(_host(p, dtype), prev)
    assert some > 10                                               # combed samples in more than one block
    if bits == 16:
        H, W = 270, 480
        q_rows = len([y for y in range(1, H - 1) if y % 2 == 1])
        assert _ref[(name, H, W, 0, 9, False)][0] == 2 * 65535 * q_rows * W          # every sample at the largest term
        assert _ref[(name, H, W, 0, 9, True)][6] == 65535 * (H // 2) * W


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
def test_field_match_on_padded_strides_and_misaligned_bases(kind):
    _, dtype, bits = kind
    for H, W in [(17, 33), (33, 129), (70, 300)]:
        cur, prev = _planes(H, W, dtype, bits, seed=H + W)
        want = inp.field_match(cur, prev, 1, 9, bits)
        for pad, off in ((16, 0), (5, 0), (16, 1), (0, 1)):
            # rows of W + pad samples from `off` samples into a buffer filled with the largest value
            cb = np.full((H, _row_len(W, pad)), (1 << bits) - 1, dtype)
            pb = cb.copy()
            cb[:, off:off + W], pb[:, off:off + W] = cur, prev
            ct, pt = _dev(cb), _dev(pb)
            got = _words(ivtc.field_match(ct[:, off:off + W], pt[:, off:off + W], 1, 9, bits))
            assert got == want, (H, W, pad, off)
            # an aligned cur with a misaligned prev takes the element path as well
            assert _words(ivtc.field_match(_dev(cur), pt[:, off:off + W], 1, 9, bits)) == want


def test_field_match_on_another_stream():
    cur, prev = _planes(64, 96, np.uint8, 8, seed=3)
    t, p = _dev(cur), _dev(prev)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = ivtc.field_match(t, p, 0, 9, 8)
    st.synchronize()
    assert _words(got) == inp.field_match(cur, prev, 0, 9, 8)


@pytest.mark.parametrize("kind", KINDS[:2], ids=[k[0] for k in KINDS[:2]])
@pytest.mark.parametrize("planes", [1, 2])
def test_weave_fields_equals_the_numpy_restatement(kind, planes):
    _, dtype, bits = kind
    rng = np.random.default_rng(7)
    guard = (1 << bits) - 1
    for H, W in SIZES + [(9, 1100)]:
        a = rng.integers(0, 1 << bits, (planes, H, W)).astype(dtype)
        b = rng.integers(0, 1 << bits, (planes, H, W)).astype(dtype)
        # the sources in rows of a multiple of 16 samples: with the padded destination below the vector path meets a ragged row
        wide = np.zeros((2, planes, H, _row_len(W, 16)), dtype)
        wide[0, :, :, :W], wide[1, :, :, :W] = a, b
        tw = _dev(wide)
        ta, tb = tw[0, :, :, :W], tw[1, :, :, :W]
        for first in (0, 1):
            want = np.stack([inp.weave_fields(a[p], b[p], first) for p in range(planes)])
            got = _host(ivtc.weave_fields(ta, tb, first), dtype)
            assert np.array_equal(got, want), (H, W, first)
            assert np.array_equal(got[:, first::2], a[:, first::2]) and np.array_equal(got[:, 1 - first::2], b[:, 1 - first::2])
            # rows of W + pad samples in a buffer of guard samples, a row of guards behind every plane, bases offset by `off`
            for pad, off in ((16, 0), (3, 1)):
                buf = _dev(np.full((planes, H + 1, _row_len(W, pad)), guard, dtype))
                view = buf[:, :H, off:off + W]
                ivtc.weave_fields(ta, tb, first, out=view)
                back = _host(buf, dtype)
                assert np.array_equal(back[:, :H, off:off + W], want), (H, W, first, pad, off)
                back[:, :H, off:off + W] = guard
                assert (back == guard).all(), (H, W, first, pad, off)
        if planes == 1:
            assert np.array_equal(_host(ivtc.weave_fields(ta[0], ta[0], 0), dtype), a[0])          # a as b: a copy
        assert np.array_equal(_host(ta, dtype), a) and np.array_equal(_host(tb, dtype), b)


def test_the_python_wrappers_refuse_what_the_entries_refuse():
    from dcvc_amd import _lib
    t = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.DcvcError, match="cthresh must be in 0..255"):
        ivtc.field_match(t, None, 0, 256, 8)
    with pytest.raises(_lib.DcvcError, match="first must be 0 or 1"):
        ivtc.weave_fields(t, t, 2)
    with pytest.raises(_lib.DcvcError, match="dst overlaps a"):
        ivtc.weave_fields(t, t, 0, out=t)
    with pytest.raises(TypeError):
        ivtc.field_match(t.float(), None, 0, 9, 8)
    with pytest.raises(ValueError):
        ivtc.field_match(t, t[:4], 0, 9, 8)
