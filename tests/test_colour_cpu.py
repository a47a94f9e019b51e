"""Colour matrices and ranges for RGB pictures without a GPU: the numpy restatement (tests/colour_np.py) of dcvc_rgb_to_x_cs /
dcvc_x_to_rgb_cs over all 2^24 colours - equal to rgb_np at bt709 / full, an exact round trip, within fp16 rounding of the
matrix in closed form, the nominal limited-range levels - and the argument checks of the two entry points, which refuse
before touching the device."""
import ctypes
import functools

import numpy as np
import pytest

import colour_np
import rgb_np

vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


@functools.lru_cache(maxsize=None)
def _cube():
    c = rgb_np.all_colours()
    c.setflags(write=False)
    return c


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


def test_bt709_full_is_the_reference_conversion_bit_for_bit():
    cube = _cube()
    x = colour_np.rgb_to_x(cube, "bt709", "full", 8)
    assert np.array_equal(_bits(x), _bits(rgb_np.rgb_to_x(cube, "recip")))
    # the inverse on the colours' own x and on x_hat that reaches the clamps and the special values
    rng = np.random.default_rng(5)
    x_hat = (rng.random((512, 512, 3)) * 1.5 - 0.75).astype(np.float16)
    x_hat[0, :6] = np.array([np.nan, np.inf, -np.inf, 0.5, -0.5, 0.0], dtype=np.float16)[:, None]
    for xh, H, W in ((x, 4096, 4096), (x_hat, 500, 510)):
        a16, a8 = colour_np.x_to_rgb(xh, H, W, "bt709", "full", 8)
        with np.errstate(invalid="ignore"):
            b16, b8 = rgb_np.x_to_rgb(xh, H, W, "recip")
        assert np.array_equal(_bits(a16), _bits(b16))
        ok = ~np.isnan(b16).transpose(1, 2, 0)              # rgb_np leaves the u8 of NaN to numpy; colour_np writes 0
        assert np.array_equal(a8[ok], b8[ok]) and (a8[~ok] == 0).all()
        assert bool((~ok).any()) == (xh is x_hat)


@pytest.mark.parametrize("matrix", ["bt601", "bt2020"])
@pytest.mark.parametrize("range_,depth", [("full", 8), ("limited", 8), ("limited", 10)])
def test_every_colour_round_trips_and_sits_on_the_closed_form(matrix, range_, depth):
    cube = _cube()
    x = colour_np.rgb_to_x(cube, matrix, range_, depth)
    _, back = colour_np.x_to_rgb(x, 4096, 4096, matrix, range_, depth)
    assert np.array_equal(back.transpose(2, 0, 1), cube)
    # 2^-11: twice the fp16 rounding (2^-12) of a value in [0.5, 1]; the fp32 steps add less than 2e-7
    got = x.astype(np.float64) + 0.5
    err = max(float(np.abs(got[..., k] - e).max()) for k, e in enumerate(colour_np.exact_ycc(cube, matrix, range_, depth)))
    print("max |x - exact| = %.6g" % err)
    assert err <= 2.0 ** -11
    if range_ == "limited":
        m, s = (1 << depth) - 1, 1 << (depth - 8)
        code = np.rint(got * m)
        assert (code[..., 0].min(), code[..., 0].max()) == (16 * s, 235 * s)
        for k in (1, 2):
            assert (code[..., k].min(), code[..., k].max()) == (16 * s, 240 * s)


@pytest.mark.parametrize("matrix", ["bt601", "bt709", "bt2020"])
def test_white_black_and_grey_in_limited_range_at_8_bits(matrix):
    for v, want in ((255, (235, 128, 128)), (0, (16, 128, 128)), (128, (126, 128, 128))):
        x = colour_np.rgb_to_x(np.full((3, 2, 2), v, np.uint8), matrix, "limited", 8)
        assert tuple(np.rint((x[0, 0].astype(np.float64) + 0.5) * 255).astype(int)) == want, (matrix, v)


@pytest.mark.parametrize("matrix", ["bt601", "bt2020"])
def test_every_colour_round_trips_at_depth_16(matrix):
    """the round trip alone: fp16 x cannot hold the code 60160 (235 * 256) exactly, so the levels are not asserted"""
    cube = _cube()
    _, back = colour_np.x_to_rgb(colour_np.rgb_to_x(cube, matrix, "limited", 16), 4096, 4096, matrix, "limited", 16)
    assert np.array_equal(back.transpose(2, 0, 1), cube)


def test_the_levels_are_one_double_division_each():
    lo, ry, mid, rc, iy, ic = colour_np.levels(10)
    assert (lo, ry, mid, rc) == tuple(np.float32(v) for v in (64 / 1023, 876 / 1023, 512 / 1023, 896 / 1023))
    assert (iy, ic) == (np.float32(1023 / 876), np.float32(1023 / 896))
    assert colour_np.levels(8)[0] == np.float32(16 / 255)


def _err():
    from dcvc_amd import _lib
    return _lib.lib().dcvc_last_error().decode()


def test_abi_refuses_bad_arguments():
    from dcvc_amd import _lib
    to_x = _lib.fn("dcvc_rgb_to_x_cs", ci, [vp, ll, ll, ll, ci, ci, vp, ci, vp, ci, ci, ci, vp])
    to_rgb = _lib.fn("dcvc_x_to_rgb_cs", ci, [vp, ci, ci, ci, vp, vp, ci, ci, ci, vp])
    p = vp(4096)     # never dereferenced: every call below is refused by the argument checks
    ok_x, ok_rgb = (p, 384, 3, 1, 64, 128, p, 3, None), (p, 128, 64, 128, p, p)
    bad_colour = [((-1, 0, 8), "matrix"), ((3, 0, 8), "matrix"), ((1, -1, 8), "range"), ((1, 2, 8), "range"),
                  ((1, 1, 7), "8..16"), ((1, 1, 17), "8..16"), ((0, 0, 7), "8..16"), ((2, 0, 17), "8..16")]
    for colour, msg in bad_colour:
        assert to_x(*ok_x, *colour, None) == -1, colour
        assert msg in _err() and "rgb_to_x_cs" in _err(), (colour, _err())
        assert to_rgb(*ok_rgb, *colour, None) == -1, colour
        assert msg in _err() and "x_to_rgb_cs" in _err(), (colour, _err())
    # what dcvc_rgb_to_x / dcvc_x_to_rgb refuse (test_rgb_cpu.py), through the new entry points with a valid colour
    bad_to_x = [((p, 384, 3, 1, 63, 128, p, 3, None), "even"),
                ((p, 384, 3, 1, 64, 127, p, 3, None), "even"),
                ((p, 384, 3, 1, 0, 128, p, 3, None), "even"),
                ((p, 384, 3, 1, 64, 128, None, 3, None), "neither"),
                ((None, 384, 3, 1, 64, 128, p, 3, None), "source"),
                ((p, 384, 3, 1, 64, 128, p, 2, None), ">= 3"),
                ((p, 383, 3, 1, 64, 128, p, 3, None), "too small"),
                ((p, 384, 2, 1, 64, 128, p, 3, None), "too small"),
                ((p, 128, 1, 128 * 63, 64, 128, p, 3, None), "too small"),
                ((p, 384, 3, 0, 64, 128, p, 3, None), "positive"),
                ((p, -384, 3, 1, 64, 128, p, 3, None), "positive"),
                ((p, 3 << 30, 3, 1, 1 << 30, 1 << 30, p, 3, None), "too large")]
    for args, msg in bad_to_x:
        assert to_x(*args, 0, 1, 10, None) == -1, args
        assert msg in _err(), (args, _err())
    bad_to_rgb = [((p, 128, 63, 128, p, p), "even"),
                  ((p, 127, 64, 128, p, p), "shorter"),
                  ((None, 128, 64, 128, p, p), "x_hat")]
    for args, msg in bad_to_rgb:
        assert to_rgb(*args, 2, 1, 10, None) == -1, args
        assert msg in _err(), (args, _err())


def test_python_wrappers_refuse_unknown_names():
    from dcvc_amd import rgb
    with pytest.raises(ValueError, match="unknown matrix"):
        rgb.rgb_to_x(None, matrix="bt470")
    with pytest.raises(ValueError, match="unknown range"):
        rgb.x_to_rgb(None, 2, 2, range="tv")
