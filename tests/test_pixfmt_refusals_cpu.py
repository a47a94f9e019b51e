"""dcvc_pix_to_x, dcvc_x_to_pix and dcvc_pix_picture_samples refuse a bad argument before any device work: every call below
passes never-dereferenced pointers on a box without a GPU, must return < 0 and must name its entry point in dcvc_last_error
(the pattern of test_ops_refusals_cpu.py). The 8-bit YUV420 entries and the plain RGB entries, which forward to the same code,
refuse under their own names."""
import ctypes

import pytest

vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
P = vp(0x1000)          # never dereferenced
P2 = vp(0x2000)
P3 = vp(0x3000)
NULL = None

SIG = {
    "pix_to_x": (ci, [vp, ci, ci, ci, ci, vp, ci, vp, vp]),
    "x_to_pix": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp]),
    "pix_picture_samples": (cll, [ci, ci, ci]),
}


def _fn(name):
    from dcvc_amd import _lib
    return _lib.fn("dcvc_" + name, *SIG[name])


def _err():
    from dcvc_amd import _lib
    return _lib.lib().dcvc_last_error().decode()


def _to_x(src=P, fmt=0, bits=8, H=16, W=24, x=P2, ldx=3, planar=NULL):
    return (src, fmt, bits, H, W, x, ldx, planar, NULL)


def _to_pix(x=P, row=24, H=16, W=24, fmt=0, bits=8, dist=P2, out=P3):
    return (x, row, H, W, fmt, bits, dist, out, NULL)


REFUSED = [
    ("pix_to_x", _to_x(fmt=4), "unknown format"),
    ("pix_to_x", _to_x(fmt=-1), "negative format"),
    ("pix_to_x", _to_x(bits=0), "bit depth 0"),
    ("pix_to_x", _to_x(bits=7), "bit depth 7"),
    ("pix_to_x", _to_x(bits=17), "bit depth 17"),
    ("pix_to_x", _to_x(H=15), "odd height"),
    ("pix_to_x", _to_x(W=23), "odd width"),
    ("pix_to_x", _to_x(fmt=2, W=23), "odd 444 width"),
    ("pix_to_x", _to_x(H=0), "no rows"),
    ("pix_to_x", _to_x(W=-2), "negative width"),
    ("pix_to_x", _to_x(ldx=2), "ldx below 3"),
    ("pix_to_x", _to_x(src=NULL), "null source"),
    ("pix_to_x", _to_x(x=NULL, planar=NULL), "x and planar both null"),
    ("pix_to_x", _to_x(H=1 << 18, W=1 << 17), "beyond the 32-bit thread index"),
    ("x_to_pix", _to_pix(fmt=4), "unknown format"),
    ("x_to_pix", _to_pix(bits=0), "bit depth 0"),
    ("x_to_pix", _to_pix(bits=7), "bit depth 7"),
    ("x_to_pix", _to_pix(bits=17), "bit depth 17"),
    ("x_to_pix", _to_pix(H=15), "odd height"),
    ("x_to_pix", _to_pix(W=23, row=23), "odd width"),
    ("x_to_pix", _to_pix(H=-16), "negative height"),
    ("x_to_pix", _to_pix(W=0), "no columns"),
    ("x_to_pix", _to_pix(row=22), "row_pixels below W"),
    ("x_to_pix", _to_pix(x=NULL), "null x_hat"),
    ("x_to_pix", _to_pix(H=1 << 18, W=1 << 17, row=1 << 17, fmt=1), "beyond the 32-bit thread index"),
    ("pix_picture_samples", (4, 16, 24), "unknown format"),
    ("pix_picture_samples", (0, 15, 24), "odd height"),
    ("pix_picture_samples", (2, 16, 23), "odd 444 width"),
    ("pix_picture_samples", (1, 0, 24), "no rows"),
]


@pytest.mark.parametrize("name,args,why", REFUSED, ids=["%s-%s" % (r[0], r[2].replace(" ", "_")) for r in REFUSED])
def test_refused_before_any_launch(name, args, why):
    f = _fn(name)
    assert len(args) == len(SIG[name][1])
    assert f(*args) < 0, why
    assert _err().startswith(name + ":"), _err()


def test_the_refusal_says_what_is_wrong():
    assert _fn("pix_to_x")(*_to_x(H=1 << 18, W=1 << 17)) < 0 and "picture too large" in _err()
    assert _fn("pix_to_x")(*_to_x(x=NULL)) < 0 and "both null" in _err()
    assert _fn("x_to_pix")(*_to_pix(row=22)) < 0 and "shorter than the picture" in _err()


def test_both_outputs_null_returns_0_without_a_launch():
    # no device is present: a launch would fail
    assert _fn("x_to_pix")(*_to_pix(dist=NULL, out=NULL)) == 0


def test_picture_samples():
    f = _fn("pix_picture_samples")
    H, W = 1080, 1920
    assert f(0, H, W) == H * W * 3 // 2 and f(3, H, W) == H * W * 3 // 2
    assert f(1, H, W) == H * W * 2 and f(2, H, W) == H * W * 3
    assert f(0, 2, 2) == 6 and f(1, 2, 2) == 8 and f(2, 2, 2) == 12 and f(3, 2, 2) == 6
    assert f(2, 16384, 16384) == 3 * 16384 * 16384          # beyond 32 bits of samples


def test_every_entry_point_of_the_group_is_tried():
    assert {r[0] for r in REFUSED} == set(SIG)


ll = cll
FORWARDS = {
    "yuv420_to_x": [vp, vp, ci, ci, vp, ci, vp],
    "x_to_yuv420": [vp, ci, ci, ci, vp, vp, vp, vp, vp],
    "rgb_to_x": [vp, ll, ll, ll, ci, ci, vp, ci, vp, vp],
    "x_to_rgb": [vp, ci, ci, ci, vp, vp, vp],
}


def _yuv_to_x(y=P, uv=P2, H=16, W=24, x=P3, ldx=3):
    return (y, uv, H, W, x, ldx, NULL)


def _x_to_yuv(x=P, row=24, H=16, W=24, y16=P2, uv16=P2, y8=P3, uv8=P3):
    return (x, row, H, W, y16, uv16, y8, uv8, NULL)


FORWARDS_REFUSED = [
    ("yuv420_to_x", _yuv_to_x(H=15), "odd height"),
    ("yuv420_to_x", _yuv_to_x(W=23), "odd width"),
    ("yuv420_to_x", _yuv_to_x(H=0), "no rows"),
    ("yuv420_to_x", _yuv_to_x(ldx=2), "ldx below 3"),
    ("yuv420_to_x", _yuv_to_x(y=NULL), "null y"),
    ("yuv420_to_x", _yuv_to_x(uv=NULL), "null uv"),
    ("yuv420_to_x", _yuv_to_x(x=NULL), "null x"),
    ("yuv420_to_x", _yuv_to_x(H=1 << 18, W=1 << 17), "beyond the 32-bit thread index"),
    ("x_to_yuv420", _x_to_yuv(H=15), "odd height"),
    ("x_to_yuv420", _x_to_yuv(W=23, row=23), "odd width"),
    ("x_to_yuv420", _x_to_yuv(W=0), "no columns"),
    ("x_to_yuv420", _x_to_yuv(row=22), "row_pixels below W"),
    ("x_to_yuv420", _x_to_yuv(x=NULL), "null x_hat"),
    ("x_to_yuv420", _x_to_yuv(H=1 << 18, W=1 << 17, row=1 << 17), "beyond the 32-bit thread index"),
    ("rgb_to_x", (P, 72, 3, 1, 15, 24, P2, 3, NULL, NULL), "odd height"),
    ("rgb_to_x", (P, 72, 3, 1, 16, 24, P2, 2, NULL, NULL), "ldx below 3"),
    ("rgb_to_x", (NULL, 72, 3, 1, 16, 24, P2, 3, NULL, NULL), "null source"),
    ("rgb_to_x", (P, 71, 3, 1, 16, 24, P2, 3, NULL, NULL), "rows overlap"),
    ("rgb_to_x", (P, 72, 3, 0, 16, 24, P2, 3, NULL, NULL), "channel stride 0"),
    ("x_to_rgb", (P, 24, 16, 23, P2, P3, NULL), "odd width"),
    ("x_to_rgb", (P, 22, 16, 24, P2, P3, NULL), "row_pixels below W"),
    ("x_to_rgb", (NULL, 24, 16, 24, P2, P3, NULL), "null x_hat"),
]


@pytest.mark.parametrize("name,args,why", FORWARDS_REFUSED, ids=["%s-%s" % (r[0], r[2].replace(" ", "_")) for r in FORWARDS_REFUSED])
def test_forwarding_entries_refuse_under_their_own_names(name, args, why):
    from dcvc_amd import _lib
    assert len(args) == len(FORWARDS[name])
    assert _lib.fn("dcvc_" + name, ci, FORWARDS[name])(*args) < 0, why
    assert _err().startswith(name + ":"), _err()        # rgb_to_x: / x_to_rgb:, not the _cs entries'


def test_x_to_yuv420_with_no_output_returns_0_without_a_launch():
    from dcvc_amd import _lib
    assert _lib.fn("dcvc_x_to_yuv420", ci, FORWARDS["x_to_yuv420"])(*_x_to_yuv(y16=NULL, uv16=NULL, y8=NULL, uv8=NULL)) == 0
