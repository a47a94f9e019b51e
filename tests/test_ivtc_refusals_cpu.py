"""dcvc_field_match and dcvc_weave_fields refuse a bad argument before any device work (field_match_validate,
weave_fields_validate): every call below passes never-dereferenced device pointers on a box without a GPU, must
return < 0 and must name the kernel in dcvc_last_error."""
import ctypes

import pytest

vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
U8, F16, U16, F32 = 0, 1, 3, 4
CUR, PREV, DST, OUT = 0x100000, 0x200000, 0x300000, 0x400000          # never dereferenced; 1 MiB apart


def _match(cur=CUR, crs=64, prev=PREV, prs=64, dtype=U8, bit_depth=8, H=48, W=64, first=0, cthresh=9, out=OUT):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_field_match", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp])
    rc = f(vp(cur) if cur else None, crs, vp(prev) if prev else None, prs, dtype, bit_depth, H, W, first, cthresh, vp(out) if out else None, None)
    return rc, _lib.lib().dcvc_last_error().decode()


def _weave(a=CUR, ars=64, aps=64 * 48, b=PREV, brs=64, bps=64 * 48, dst=DST, drs=64, dps=64 * 48, dtype=U8, H=48, W=64, n_planes=1, first=0):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_weave_fields", ci, [vp, ci, cll, vp, ci, cll, vp, ci, cll, ci, ci, ci, ci, ci, vp])
    rc = f(vp(a) if a else None, ars, aps, vp(b) if b else None, brs, bps, vp(dst) if dst else None, drs, dps, dtype, H, W, n_planes, first, None)
    return rc, _lib.lib().dcvc_last_error().decode()


MATCH_REFUSED = [
    ("null cur", dict(cur=0), "null operand"),
    ("null out8", dict(out=0), "null operand"),
    ("fp16 samples", dict(dtype=F16), "sample type"),
    ("fp32 samples", dict(dtype=F32), "sample type"),
    ("sample type 2", dict(dtype=2), "sample type"),
    ("sample type -1", dict(dtype=-1), "sample type"),
    ("u8 at 10 bits", dict(bit_depth=10), "bit_depth must be 8 (u8) or 9..16 (u16), got 10"),
    ("u8 at 7 bits", dict(bit_depth=7), "got 7"),
    ("u16 at 8 bits", dict(dtype=U16, bit_depth=8), "got 8"),
    ("u16 at 17 bits", dict(dtype=U16, bit_depth=17), "got 17"),
    ("H = 1", dict(H=1), "H must be in 2..16384"),
    ("H = 0", dict(H=0), "H must be in 2..16384"),
    ("H = -1", dict(H=-1), "H must be in 2..16384"),
    ("H = 16385", dict(H=16385), "H must be in 2..16384"),
    ("W = 0", dict(W=0), "W in 1..16384"),
    ("W = 16385", dict(W=16385, crs=16385, prs=16385), "W in 1..16384"),
    ("first = 2", dict(first=2), "first must be 0 or 1, got 2"),
    ("first = -1", dict(first=-1), "first must be 0 or 1, got -1"),
    ("cthresh = -1", dict(cthresh=-1), "cthresh must be in 0..255, got -1"),
    ("cthresh = 256", dict(cthresh=256), "cthresh must be in 0..255, got 256"),
    ("cur row stride below W", dict(crs=63), "a row stride is below the width"),
    ("prev row stride below W", dict(prs=63), "a row stride is below the width"),
    ("u16 cur at an odd address", dict(dtype=U16, bit_depth=10, cur=CUR + 1), "16-bit planes must be 2-byte aligned"),
    ("u16 prev at an odd address", dict(dtype=U16, bit_depth=10, prev=PREV + 1), "16-bit planes must be 2-byte aligned"),
    ("out8 at 4 bytes", dict(out=OUT + 4), "out8 must be 8-byte aligned"),
    ("out8 at an odd address", dict(out=OUT + 1), "out8 must be 8-byte aligned"),
]


@pytest.mark.parametrize("why,kwargs,words", MATCH_REFUSED, ids=[r[0].replace(" ", "_") for r in MATCH_REFUSED])
def test_field_match_refuses_before_any_launch(why, kwargs, words):
    rc, err = _match(**kwargs)
    assert rc < 0, why
    assert err.startswith("field_match:") and words in err, err


def test_field_match_does_not_read_prevs_stride_without_prev():
    # a stride that is refused with prev passes without it: the call gets as far as the last check
    rc, err = _match(prev=0, prs=0, out=OUT + 4)
    assert rc < 0 and "out8 must be 8-byte aligned" in err, err


WEAVE_REFUSED = [
    ("null a", dict(a=0), "null operand"),
    ("null b", dict(b=0), "null operand"),
    ("null dst", dict(dst=0), "null operand"),
    ("fp16 samples", dict(dtype=F16), "sample type"),
    ("sample type 2", dict(dtype=2), "sample type"),
    ("sample type -1", dict(dtype=-1), "sample type"),
    ("H = 1", dict(H=1), "H must be in 2..16384"),
    ("H = 16385", dict(H=16385), "H must be in 2..16384"),
    ("W = 0", dict(W=0), "W in 1..16384"),
    ("W = 16385", dict(W=16385, ars=16385, brs=16385, drs=16385), "W in 1..16384"),
    ("n_planes = 0", dict(n_planes=0), "n_planes must be in 1..65535"),
    ("n_planes = 65536", dict(n_planes=65536), "n_planes must be in 1..65535"),
    ("first = 2", dict(first=2), "first must be 0 or 1, got 2"),
    ("first = -1", dict(first=-1), "first must be 0 or 1, got -1"),
    ("a row stride below W", dict(ars=63), "a row stride is below the width"),
    ("b row stride below W", dict(brs=63), "a row stride is below the width"),
    ("dst row stride below W", dict(drs=63), "a row stride is below the width"),
    ("a plane stride below the plane", dict(n_planes=2, aps=64 * 48 - 1), "a plane stride is below the plane"),
    ("b plane stride below the plane", dict(n_planes=2, bps=64 * 48 - 1), "a plane stride is below the plane"),
    ("dst plane stride below the plane", dict(n_planes=2, dps=64 * 48 - 1), "a plane stride is below the plane"),
    ("u16 a at an odd address", dict(dtype=U16, a=CUR + 1), "16-bit planes must be 2-byte aligned"),
    ("u16 b at an odd address", dict(dtype=U16, b=PREV + 1), "16-bit planes must be 2-byte aligned"),
    ("u16 dst at an odd address", dict(dtype=U16, dst=DST + 1), "16-bit planes must be 2-byte aligned"),
    ("dst is a", dict(dst=CUR), "dst overlaps a"),
    ("dst starts inside a", dict(dst=CUR + 64 * 48 - 1), "dst overlaps a"),
    ("dst ends inside a", dict(dst=CUR - 64 * 48 + 1), "dst overlaps a"),
    ("dst is b", dict(dst=PREV), "dst overlaps b"),
    ("dst starts inside b's second plane", dict(n_planes=2, dst=PREV + 2 * 64 * 48 - 1), "dst overlaps b"),
]


@pytest.mark.parametrize("why,kwargs,words", WEAVE_REFUSED, ids=[r[0].replace(" ", "_") for r in WEAVE_REFUSED])
def test_weave_fields_refuses_before_any_launch(why, kwargs, words):
    rc, err = _weave(**kwargs)
    assert rc < 0, why
    assert err.startswith("weave_fields:") and words in err, err


def test_weave_fields_does_not_read_plane_strides_for_one_plane_and_takes_a_as_b():
    rc, err = _weave(aps=0, bps=0, dps=0, b=CUR, dst=CUR)
    assert rc < 0 and "overlaps a" in err, err
