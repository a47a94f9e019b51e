"""dcvc_denoise_planes refuses a bad argument before any device work (denoise_validate): every call below passes
never-dereferenced device pointers on a box without a GPU, must return < 0 and must name the kernel in dcvc_last_error."""
import ctypes

import pytest

vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
U8, F16, U16, F32 = 0, 1, 3, 4
SRC, PREV, DST = 0x100000, 0x200000, 0x300000          # never dereferenced; 1 MiB apart


def _call(src=SRC, srs=64, sps=64 * 48, prev=PREV, prs=64, pps=64 * 48, dst=DST, drs=64, dps=64 * 48, dtype=U8, bit_depth=8, H=48, W=64,
          n_planes=1, spatial=8, temporal=8):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_denoise_planes", ci, [vp, ci, cll, vp, ci, cll, vp, ci, cll, ci, ci, ci, ci, ci, ci, ci, vp])
    rc = f(vp(src) if src else None, srs, sps, vp(prev) if prev else None, prs, pps, vp(dst) if dst else None, drs, dps, dtype, bit_depth,
           H, W, n_planes, spatial, temporal, None)
    return rc, _lib.lib().dcvc_last_error().decode()


REFUSED = [
    ("null src", dict(src=0)),
    ("null dst", dict(dst=0)),
    ("fp16 samples", dict(dtype=F16)),
    ("fp32 samples", dict(dtype=F32)),
    ("sample type 2", dict(dtype=2)),
    ("sample type -1", dict(dtype=-1)),
    ("u8 at 10 bits", dict(bit_depth=10)),
    ("u8 at 7 bits", dict(bit_depth=7)),
    ("u16 at 8 bits", dict(dtype=U16, bit_depth=8)),
    ("u16 at 17 bits", dict(dtype=U16, bit_depth=17)),
    ("H = 0", dict(H=0)),
    ("W = 0", dict(W=0)),
    ("H = -1", dict(H=-1)),
    ("H = 16385", dict(H=16385)),
    ("W = 16385", dict(W=16385, srs=16385, prs=16385, drs=16385)),
    ("n_planes = 0", dict(n_planes=0)),
    ("n_planes = 65536", dict(n_planes=65536)),
    ("spatial = -1", dict(spatial=-1)),
    ("spatial = 65", dict(spatial=65)),
    ("temporal = -1", dict(temporal=-1)),
    ("temporal = 65", dict(temporal=65)),
    ("src row stride below W", dict(srs=63)),
    ("prev row stride below W", dict(prs=63)),
    ("dst row stride below W", dict(drs=63)),
    ("src plane stride below the plane", dict(n_planes=2, sps=64 * 48 - 1)),
    ("prev plane stride below the plane", dict(n_planes=2, pps=64 * 48 - 1)),
    ("dst plane stride below the plane", dict(n_planes=2, dps=64 * 48 - 1)),
    ("dst is src", dict(dst=SRC)),
    ("dst starts inside src", dict(dst=SRC + 64 * 48 - 1)),
    ("dst ends inside src", dict(dst=SRC - 64 * 48 + 1)),
    ("dst is prev", dict(dst=PREV)),
    ("dst starts inside prev's second plane", dict(n_planes=2, dst=PREV + 2 * 64 * 48 - 1)),
    ("u16 src at an odd address", dict(dtype=U16, bit_depth=10, src=SRC + 1)),
]


@pytest.mark.parametrize("why,kwargs", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_refused_before_any_launch(why, kwargs):
    rc, err = _call(**kwargs)
    assert rc < 0, why
    assert err.startswith("denoise:"), err


def test_the_message_says_what_is_wrong():
    assert "got 65:8" in _call(spatial=65)[1]
    assert "1..16384" in _call(H=16385)[1]
    assert "overlaps prev" in _call(dst=PREV)[1] and "overlaps src" in _call(dst=SRC)[1]
    assert "got 10" in _call(bit_depth=10)[1]


def test_prev_strides_are_not_read_without_prev():
    # strides that are refused with prev pass without it: the call gets as far as the overlap check, which comes last
    rc, err = _call(prev=0, prs=0, pps=0, n_planes=2, dst=SRC)
    assert rc < 0 and "overlaps src" in err, err
