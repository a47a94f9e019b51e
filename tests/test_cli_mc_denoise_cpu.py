"""What dcvc encode --denoise-mc / --mv-log refuse with status 2 before a model is loaded, without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.yuv"), "-W", "352", "-H", "288",
                 "-o", str(tmp_path / "o.bin")] + extra)


def _decode(tmp_path, extra):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path / "o.yuv")]
                + extra)


def _refused(r, tmp_path, words):
    assert r.returncode == 2 and words in r.stderr, r.stderr
    assert "missing.dcvw" not in r.stderr, r.stderr          # before a model is loaded
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "o.yuv").exists() and not (tmp_path / "mv.json").exists()


@pytest.mark.parametrize("value", ["16", "-1", "7:", "a", "7:256", "", ":4", "7:4:2", "7.5", " 7", "1e1", "07", "7:-1", "7:x", "7: 4", "99"])
def test_malformed_and_out_of_range_values_are_refused(tmp_path, value):
    _refused(_encode(tmp_path, ["--denoise", "8", "--denoise-mc", value]), tmp_path,
             "--denoise-mc must be R or R:LAMBDA with integers in 0..15 and 0..255")


def test_the_flags_need_denoise(tmp_path):
    _refused(_encode(tmp_path, ["--denoise-mc", "7"]), tmp_path, "--denoise-mc needs --denoise")
    _refused(_encode(tmp_path, ["--mv-log", str(tmp_path / "mv.json")]), tmp_path, "--mv-log needs --denoise")
    _refused(_encode(tmp_path, ["--denoise-mc", "7", "--mv-log", str(tmp_path / "mv.json")]), tmp_path, "needs --denoise")


def test_the_log_needs_the_search_and_a_file_name(tmp_path):
    _refused(_encode(tmp_path, ["--denoise", "8", "--mv-log", str(tmp_path / "mv.json")]), tmp_path, "--mv-log needs --denoise-mc")
    _refused(_encode(tmp_path, ["--denoise", "8", "--denoise-mc", "7", "--mv-log", "-"]), tmp_path, "--mv-log needs a file name")


def test_the_flags_are_encoder_flags(tmp_path):
    _refused(_decode(tmp_path, ["--denoise-mc", "7"]), tmp_path, "--denoise-mc is an encoder flag")
    _refused(_decode(tmp_path, ["--mv-log", str(tmp_path / "mv.json")]), tmp_path, "--mv-log is an encoder flag")


def test_the_source_types_denoise_refuses_stay_refused(tmp_path):
    _refused(_encode(tmp_path, ["--denoise", "8", "--denoise-mc", "7", "--src-type", "nv12"]), tmp_path, "sources are not filtered yet")


@pytest.mark.parametrize("extra", [["--denoise-mc", "7"], ["--denoise-mc", "0"], ["--denoise-mc", "15:255"], ["--denoise-mc", "7:0"],
                                   ["--denoise-mc", "3:12", "--mv-log", "mv.json"], ["--denoise-mc", "7", "--src-type", "yuv422", "--bit-depth", "10"]])
def test_good_flags_pass_the_flag_checks(tmp_path, extra):
    extra = [str(tmp_path / e) if e == "mv.json" else e for e in extra]
    r = _encode(tmp_path, ["--denoise", "8:8"] + extra)
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "mv.json").exists()
