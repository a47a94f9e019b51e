"""What needs no device of the encoder-side quality path: the dcvc tool's refusals for --target-psnr and
--quality-log that the flags alone decide - each before a model is loaded (the weight files named here do not exist) with
status 2, its message naming the flag, and no output file - and the refusals of dcvc_dmcld_reconstruct /
dcvc_dmcht_reconstruct for a null handle or a null x_hat."""
import ctypes
import os
import subprocess

import pytest

from dcvc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")


def _encode(tmp_path, *extra):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    args = ["encode", "--intra", str(tmp_path / "missing.dcvw"), "--inter", str(tmp_path / "missing_p.dcvw"), "-i",
            str(tmp_path / "missing.yuv"), "-W", "64", "-H", "48", "-o", str(tmp_path / "o.bin"), "--quality-log", str(tmp_path / "q.json")]
    return subprocess.run([TOOL] + args + list(extra), capture_output=True, text=True, timeout=120)


def _refused(tmp_path, r, *says):
    assert r.returncode == 2, (r.returncode, r.stderr)
    for s in says:
        assert s in r.stderr, r.stderr
    assert "missing.dcvw" not in r.stderr and "missing_p.dcvw" not in r.stderr      # before a model is loaded
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "q.json").exists()


@pytest.mark.parametrize("value", ["nan", "inf", "-inf", "0", "-3", "", "38dB", "abc"])
def test_a_target_that_is_not_finite_or_not_positive_is_refused(tmp_path, value):
    _refused(tmp_path, _encode(tmp_path, "--target-psnr", value), "--target-psnr must be a positive number of dB")


def test_target_psnr_with_target_bpp_is_refused(tmp_path):
    _refused(tmp_path, _encode(tmp_path, "--target-psnr", "38", "--target-bpp", "0.1"), "--target-psnr cannot be combined with --target-bpp")


def test_target_psnr_with_qp_p_is_refused(tmp_path):
    _refused(tmp_path, _encode(tmp_path, "--target-psnr", "38", "--qp-p", "20"), "--target-psnr cannot be combined with --qp-p")


def test_target_psnr_with_a_batch_is_refused(tmp_path):
    _refused(tmp_path, _encode(tmp_path, "--target-psnr", "38", "--batch", "2", "--intra-period", "1"),
             "--target-psnr cannot be combined with --batch above 1")


def test_qp_min_above_qp_max_is_refused(tmp_path):
    _refused(tmp_path, _encode(tmp_path, "--target-psnr", "38", "--qp-min", "40", "--qp-max", "20"), "--qp-min 40 is above --qp-max 20")
    _refused(tmp_path, _encode(tmp_path, "--target-psnr", "38", "--qp-max", "64"), "--qp-max must be in 0..63")


def test_the_range_flags_still_need_a_target(tmp_path):
    """the refusal that was there: --qp-min / --qp-max without a rate or a quality target"""
    _refused(tmp_path, _encode(tmp_path, "--qp-min", "10"), "--qp-min needs --target-bpp")


def test_quality_log_needs_a_file_name(tmp_path):
    assert os.path.exists(TOOL)
    r = subprocess.run([TOOL, "encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.yuv"), "-W", "64", "-H", "48",
                        "-o", str(tmp_path / "o.bin"), "--quality-log", ""], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--quality-log needs a file name" in r.stderr and "missing.dcvw" not in r.stderr, r.stderr


@pytest.mark.parametrize("extra", [["--target-psnr", "38"], ["--target-psnr", "38.5", "--qp-min", "8", "--qp-max", "40", "--qp-i", "20"], []])
def test_good_flags_pass_the_checks(tmp_path, extra):
    """the model is next: the weight file that does not exist"""
    r = _encode(tmp_path, *extra)
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "q.json").exists()


# ---------------------------------------------------------------- the C ABI
_vp, _ci = ctypes.c_void_p, ctypes.c_int


@pytest.mark.parametrize("name", ["dcvc_dmcld_reconstruct", "dcvc_dmcht_reconstruct"])
def test_reconstruct_refuses_null_pointers(name):
    f = _lib.fn(name, _ci, [_vp, _vp, _vp])
    buf = ctypes.create_string_buffer(64)
    for handle, x_hat in ((None, ctypes.addressof(buf)), (None, None)):
        assert f(handle, x_hat, None) < 0
        msg = _lib.lib().dcvc_last_error().decode()
        assert name in msg and "null" in msg, msg
    assert buf.raw == b"\0" * 64                                       # nothing touched
