"""The integer Lanczos-3 resampler without a GPU: the host table of dcvc_resample_taps against its two numpy
restatements with ==, the pinned rows, the row sums, the accumulator bound, what needs no device to be refused, the numpy
reference's own invariants, and the tool's refusals of --scale / --out-size, which run before a model is loaded."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import resample_np
from dcvc_amd import _lib, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")

# ratios 2:1, 1:2, 3:2, 2:3 and 1:1: every pre-rounding value w * 4096 / sum lies at least 1.3e-2 from a rounding boundary, so a
# last-bit difference between two libm's sin cannot flip a coefficient (1920 -> 854 has a margin of 4e-5 and is left out)
PAIRS = [(8, 4), (4, 8), (46, 23), (23, 46), (96, 64), (64, 96), (144, 96), (352, 176), (176, 352), (64, 64)]
ROW_8_4 = [15, 62, -139, -273, 555, 1828, 1828, 555, -273, -139, 62, 15]
ROW_4_8_EVEN = [30, -279, 1110, 3658, -546, 123]


@pytest.fixture(scope="module")
def tables():
    return {p: resample.native_taps(*p) for p in PAIRS}


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_native_table_equals_both_restatements(tables, pair):
    coef, first = tables[pair]
    assert coef.dtype == np.int16 and first.dtype == np.int32
    assert coef.shape == (pair[1], resample.ntaps(*pair)) == (pair[1], resample_np.ntaps(*pair))
    for name, (c, f) in (("resample.taps", resample.taps(*pair)), ("resample_np.taps", resample_np.taps(*pair))):
        assert c.dtype == np.int16 and np.array_equal(c, coef), name
        assert np.array_equal(f, first), name


def test_pinned_rows(tables):
    coef, first = tables[(8, 4)]
    assert coef.tolist() == [ROW_8_4] * 4 and first.tolist() == [-5, -3, -1, 1]
    coef, first = tables[(4, 8)]
    assert coef.tolist() == [ROW_4_8_EVEN, ROW_4_8_EVEN[::-1]] * 4
    assert first.tolist() == [-3, -2, -2, -1, -1, 0, 0, 1]
    coef, first = tables[(64, 64)]
    assert coef.shape == (64, 6) and coef.tolist() == [[0, 0, 4096, 0, 0, 0]] * 64
    assert first.tolist() == list(range(-2, 62))


def test_rows_sum_to_4096_and_fit_the_accumulator(tables):
    worst = 0
    for pair, (coef, _) in tables.items():
        c = coef.astype(np.int64)
        assert (c.sum(axis=1) == 4096).all(), pair
        worst = max(worst, int(np.abs(c).sum(axis=1).max()))
    assert worst * 65535 + 2048 < 2 ** 31, worst


def test_tap_counts():
    ntaps = resample._fn("dcvc_resample_ntaps")
    assert [ntaps(a, b) for a, b in ((8, 4), (4, 8), (64, 64), (96, 64), (64, 8), (8, 64), (16384, 2048))] == [12, 6, 6, 10, 48, 6, 48]


@pytest.mark.parametrize("n_in,n_out", [(0, 4), (4, 0), (-8, 4), (65, 8), (8, 65), (16385, 16385), (2, 16386)])
def test_lengths_and_ratios_outside_the_range_are_refused(n_in, n_out):
    assert resample._fn("dcvc_resample_ntaps")(n_in, n_out) == -1
    coef = np.zeros(48 * max(n_out, 1), np.int16)
    first = np.zeros(max(n_out, 1), np.int32)
    rc = resample._fn("dcvc_resample_taps")(n_in, n_out, coef.ctypes.data, first.ctypes.data)
    assert rc == -1 and "ratio in [1/8, 8]" in _lib.lib().dcvc_last_error().decode()
    assert not coef.any() and not first.any()
    # the plan refuses the same before it asks for device memory
    for dims in ((n_in, 64, n_out, 64), (64, n_in, 64, n_out)):
        plan = ctypes.c_void_p()
        assert resample._fn("dcvc_resample_plan_create")(*dims, ctypes.byref(plan)) == -1 and not plan
        assert "ratio in [1/8, 8]" in _lib.lib().dcvc_last_error().decode()
    with pytest.raises(ValueError):
        resample.native_taps(n_in, n_out)
    if 0 < max(n_in, n_out) <= 16384:
        for mod in (resample, resample_np):
            with pytest.raises(ValueError):
                mod.ntaps(n_in, n_out)


def test_null_operands_are_refused_without_a_device():
    first = np.zeros(4, np.int32)
    assert resample._fn("dcvc_resample_taps")(8, 4, None, first.ctypes.data) == -1
    assert "null" in _lib.lib().dcvc_last_error().decode()
    assert resample._fn("dcvc_resample_plan_create")(8, 8, 4, 4, None) == -1
    buf = np.zeros(64, np.uint8)
    rc = resample._fn("dcvc_resample_planes")(None, buf.ctypes.data, 0, 8, 64, buf.ctypes.data, 0, 8, 64, 1, 255, buf.ctypes.data, 64, None)
    assert rc == -1 and "null plan" in _lib.lib().dcvc_last_error().decode()
    assert resample._fn("dcvc_resample_workspace_bytes")(None, 1) == 0
    assert resample._fn("dcvc_resample_plan_free")(None) == 0


@pytest.mark.parametrize("shape,out", [((16, 24), (8, 12)), ((8, 12), (16, 24)), ((18, 30), (12, 20)), ((12, 20), (18, 30)),
                                       ((17, 23), (40, 9))])
@pytest.mark.parametrize("dtype,max_val,value", [(np.uint8, 255, 255), (np.uint8, 255, 0), (np.uint8, 255, 77),
                                                 (np.uint16, 1023, 1023), (np.uint16, 65535, 65535), (np.uint16, 65535, 12345)])
def test_a_constant_plane_stays_constant(shape, out, dtype, max_val, value):
    got = resample_np.resample_plane(np.full(shape, value, dtype), out[0], out[1], max_val)
    assert got.dtype == dtype and got.shape == out and (got == value).all()


@pytest.mark.parametrize("dtype,max_val", [(np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535)])
def test_the_identity_is_a_copy(dtype, max_val):
    a = np.random.default_rng(3).integers(0, max_val + 1, (37, 53)).astype(dtype)
    assert np.array_equal(resample_np.resample_plane(a, 37, 53, max_val), a)


def test_the_reference_clamps_both_ways():
    # a 0 / max checkerboard column pattern overshoots on both sides before the clamp
    a = np.zeros((8, 32), np.uint16)
    a[:, 16:] = 65535
    got = resample_np.resample_plane(a, 8, 64, 65535).astype(np.int64)
    assert got.min() == 0 and got.max() == 65535
    c, first = resample_np.taps(32, 64)
    raw = [(int((c[j].astype(np.int64) * a[0, np.clip(first[j] + np.arange(6), 0, 31)].astype(np.int64)).sum()) + 2048) >> 12
           for j in range(64)]
    assert min(raw) < 0 and max(raw) > 65535          # the unclamped filter does leave the range here


# ------------------------------------------------------------------------------------ the tool
def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.yuv"), "-W", "352", "-H", "288",
                 "-o", str(tmp_path / "o.bin")] + extra)


def _decode(tmp_path, extra):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path / "o.yuv")]
                + extra)


BAD_SIZES = ["", "176", "176x", "x144", "176x144x2", "177x144", "176x143", "0x144", "176x0", "-176x144", "176x-144", "176X144",
             "176 x144", "1e2x144", "176x144 "]


@pytest.mark.parametrize("value", BAD_SIZES)
def test_malformed_scale_is_refused(tmp_path, value):
    r = _encode(tmp_path, ["--scale", value])
    assert r.returncode == 2 and "--scale must be WxH" in r.stderr, r.stderr
    assert not (tmp_path / "o.bin").exists()


@pytest.mark.parametrize("value", BAD_SIZES)
def test_malformed_out_size_is_refused(tmp_path, value):
    r = _decode(tmp_path, ["--out-size", value])
    assert r.returncode == 2 and "--out-size must be WxH" in r.stderr, r.stderr
    assert not (tmp_path / "o.yuv").exists()


@pytest.mark.parametrize("value", ["42x288", "352x34", "2818x288", "352x2306", "32768x288"])
def test_scale_ratio_outside_the_range_is_refused(tmp_path, value):
    r = _encode(tmp_path, ["--scale", value])
    assert r.returncode == 2 and "ratio must lie in [1/8, 8]" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["44x36", "2816x2304"])
def test_scale_at_the_edge_of_the_range_passes_the_flag_checks(tmp_path, value):
    r = _encode(tmp_path, ["--scale", value])
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr


@pytest.mark.parametrize("src_type", ["rgb24", "png"])
def test_rgb_sources_are_refused(tmp_path, src_type):
    r = _encode(tmp_path, ["--scale", "176x144", "--src-type", src_type])
    assert r.returncode == 2 and "RGB sources are not resampled yet" in r.stderr, r.stderr
    r = _decode(tmp_path, ["--out-size", "176x144", "--src-type", src_type])
    assert r.returncode == 2 and "RGB sources are not resampled yet" in r.stderr, r.stderr


def test_scale_needs_the_source_size(tmp_path):
    r = _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.yuv"), "-o", str(tmp_path / "o.bin"),
              "--scale", "176x144"])
    assert r.returncode == 2 and "picture size must be positive and even" in r.stderr, r.stderr


def test_calc_ssim_floor_is_checked_at_the_output_size(tmp_path):
    r = _decode(tmp_path, ["--out-size", "352x160", "--calc-ssim", "1", "--ref", str(tmp_path / "missing.yuv")])
    assert r.returncode == 2 and "--calc-ssim needs both picture sides >= 176" in r.stderr and "--out-size" in r.stderr, r.stderr
