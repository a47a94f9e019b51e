"""The dcvc tool's refusals for the decoder-buffer flags that the flags alone decide: each before a model is
loaded (the weight files named here do not exist), with status 2, its message naming the flag, and no output file."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")


def _tool(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, *extra, inter=True):
    args = ["encode", "--intra", str(tmp_path / "missing.dcvw")] + (["--inter", str(tmp_path / "missing_p.dcvw")] if inter else [])
    return _tool(args + ["-i", str(tmp_path / "missing.yuv"), "-W", "64", "-H", "48", "-o", str(tmp_path / "o.bin")] + list(extra))


def _refused(tmp_path, r, *says):
    assert r.returncode == 2, (r.returncode, r.stderr)
    for s in says:
        assert s in r.stderr, r.stderr
    assert "missing.dcvw" not in r.stderr and "missing_p.dcvw" not in r.stderr      # before a model is loaded
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "v.json").exists()


PAIR = ["--vbv-maxrate", "0.05", "--vbv-bufsize", "4"]


def test_one_of_the_pair_without_the_other(tmp_path):
    _refused(tmp_path, _encode(tmp_path, "--vbv-maxrate", "0.05"), "--vbv-maxrate needs --vbv-bufsize")
    _refused(tmp_path, _encode(tmp_path, "--vbv-bufsize", "4"), "--vbv-bufsize needs --vbv-maxrate")


@pytest.mark.parametrize("value", ["nan", "inf", "-inf", "0", "-0.5"])
def test_values_the_model_refuses(tmp_path, value):
    _refused(tmp_path, _encode(tmp_path, "--vbv-maxrate", value, "--vbv-bufsize", "4"), "--vbv-maxrate " + value, "vbv: maxrate")
    _refused(tmp_path, _encode(tmp_path, "--vbv-maxrate", "0.05", "--vbv-bufsize", value), "--vbv-bufsize " + value, "vbv: bufsize")
    _refused(tmp_path, _encode(tmp_path, *PAIR, "--vbv-init", value), "--vbv-init " + value, "vbv: init")


def test_init_above_one_and_values_that_are_no_numbers(tmp_path):
    _refused(tmp_path, _encode(tmp_path, *PAIR, "--vbv-init", "1.5"), "--vbv-init 1.5", "(0, 1]")
    _refused(tmp_path, _encode(tmp_path, "--vbv-maxrate", "0.05bpp", "--vbv-bufsize", "4"), "--vbv-maxrate must be a number")
    _refused(tmp_path, _encode(tmp_path, "--vbv-maxrate", "0.05", "--vbv-bufsize", ""), "--vbv-bufsize must be a number")
    _refused(tmp_path, _encode(tmp_path, *PAIR, "--vbv-init", "half"), "--vbv-init must be a number")


def test_init_and_log_need_the_pair(tmp_path):
    _refused(tmp_path, _encode(tmp_path, "--vbv-init", "0.5"), "--vbv-init needs --vbv-maxrate and --vbv-bufsize")
    _refused(tmp_path, _encode(tmp_path, "--vbv-log", str(tmp_path / "v.json")), "--vbv-log needs --vbv-maxrate and --vbv-bufsize")


def test_a_batch_is_refused(tmp_path):
    _refused(tmp_path, _encode(tmp_path, *PAIR, "--batch", "2", inter=False), "--vbv-maxrate cannot be combined with --batch above 1", "one q_index")


def test_target_psnr_is_refused(tmp_path):
    _refused(tmp_path, _encode(tmp_path, *PAIR, "--target-psnr", "38"), "--vbv-maxrate cannot be combined with --target-psnr")


def test_a_log_named_dash_is_refused(tmp_path):
    _refused(tmp_path, _encode(tmp_path, *PAIR, "--vbv-log", "-"), "--vbv-log -: a log goes to a file of its own")
    _refused(tmp_path, _encode(tmp_path, *PAIR, "--vbv-log", ""), "--vbv-log needs a file name")


def test_qp_min_keeps_needing_a_target(tmp_path):
    _refused(tmp_path, _encode(tmp_path, *PAIR, "--qp-min", "10"), "--qp-min needs --target-bpp")


@pytest.mark.parametrize("flag,value", [("--vbv-maxrate", "0.05"), ("--vbv-bufsize", "4"), ("--vbv-init", "0.5"), ("--vbv-log", "v.json")])
def test_every_flag_is_refused_on_decode(tmp_path, flag, value):
    r = _tool(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path / "o.bin"), flag, value])
    _refused(tmp_path, r, flag + " is an encoder flag")


@pytest.mark.parametrize("extra", [[], ["--vbv-init", "1"], ["--vbv-init", "0.25", "--vbv-log", "v.json"], ["--target-bpp", "0.1", "--qp-min", "8"],
                                   ["--target-bpp", "0.1", "--rc-mode", "probe"], ["--scale", "32x32"]])
def test_good_flags_pass_the_checks(tmp_path, extra):
    """the model is next: the weight file that does not exist"""
    extra = [str(tmp_path / e) if e == "v.json" else e for e in extra]
    r = _encode(tmp_path, *PAIR, *extra)
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "v.json").exists()
