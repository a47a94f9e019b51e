"""What dcvc decode --interpolate / --interp-log / --interp-ref and dcvc encode --frame-step refuse with status 2
before a model is loaded, without a GPU."""
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
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "o.yuv").exists() and not (tmp_path / "ip.json").exists()


@pytest.mark.parametrize("value", ["1", "0", "9", "-2", "", "a", "2:", ":7", "2:16", "2:7:256", "2:7:4:256", "2:7:4:8:1", "2.5", " 2", "02",
                                   "2:07", "2:-1", "2:x", "2: 7", "1e1", "2::4", "99"])
def test_malformed_and_out_of_range_values_are_refused(tmp_path, value):
    _refused(_decode(tmp_path, ["--interpolate", value]), tmp_path,
             "--interpolate must be N[:R[:LAMBDA[:LIMIT]]] with integers in 2..8, 0..15, 0..255 and 0..255")


def test_the_companions_need_the_flag_and_each_other(tmp_path):
    log, ref = str(tmp_path / "ip.json"), str(tmp_path / "ref.yuv")
    _refused(_decode(tmp_path, ["--interp-log", log]), tmp_path, "--interp-log needs --interpolate")
    _refused(_decode(tmp_path, ["--interp-ref", ref]), tmp_path, "--interp-ref needs --interpolate")
    _refused(_decode(tmp_path, ["--interpolate", "2", "--interp-ref", ref]), tmp_path, "--interp-ref needs --interp-log")
    _refused(_decode(tmp_path, ["--interpolate", "2", "--interp-log", "-"]), tmp_path, "--interp-log needs a file name")
    _refused(_decode(tmp_path, ["--interpolate", "2", "--interp-log", log, "--interp-ref", "-"]), tmp_path, "--interp-ref needs a file name")


@pytest.mark.parametrize("flag", [["--interpolate", "2"], ["--interp-log", "ip.json"], ["--interp-ref", "ref.yuv"]])
def test_the_flags_are_decoder_flags(tmp_path, flag):
    _refused(_encode(tmp_path, flag), tmp_path, flag[0] + " is a decoder flag")


@pytest.mark.parametrize("src_type", ["rgb24", "rgb48", "png", "png16", "nv12", "p010", "nv21", "nv16", "p210", "uyvy", "yuy2", "y210", "v210"])
def test_other_picture_types_are_refused(tmp_path, src_type):
    r = _decode(tmp_path, ["--interpolate", "2", "--src-type", src_type])
    assert r.returncode == 2 and "missing.dcvw" not in r.stderr, r.stderr
    assert "--interpolate is for planar YUV pictures" in r.stderr, r.stderr
    assert not (tmp_path / "o.yuv").exists()


def test_the_manifest_check_is_refused(tmp_path):
    _refused(_decode(tmp_path, ["--interpolate", "2", "--verify-hash", str(tmp_path / "m.txt")]), tmp_path, "not with --interpolate")


@pytest.mark.parametrize("value", ["1", "0", "9", "-2", "", "a", "2:1", "2.5", "1e1"])
def test_a_bad_frame_step_is_refused(tmp_path, value):
    _refused(_encode(tmp_path, ["--frame-step", value]), tmp_path, "--frame-step must be in 2..8")


def test_the_frame_step_is_refused_where_it_cannot_work(tmp_path):
    _refused(_decode(tmp_path, ["--frame-step", "2"]), tmp_path, "--frame-step is an encoder flag")
    _refused(_encode(tmp_path, ["--frame-step", "2", "--deinterlace", "frame"]), tmp_path, "--frame-step and --deinterlace")
    _refused(_encode(tmp_path, ["--frame-step", "2", "--ivtc", "film"]), tmp_path, "--frame-step and --ivtc")


@pytest.mark.parametrize("extra", [["--interpolate", "2"], ["--interpolate", "8"], ["--interpolate", "3:15"], ["--interpolate", "2:0:255"],
                                   ["--interpolate", "2:7:4:0"], ["--interpolate", "4:7:4:255", "--interp-log", "ip.json"],
                                   ["--interpolate", "2", "--interp-log", "ip.json", "--interp-ref", "ref.yuv"],
                                   ["--interpolate", "2", "--src-type", "yuv422", "--bit-depth", "10"], ["--interpolate", "2", "--src-type", "yuv444"]])
def test_good_decoder_flags_pass_the_flag_checks(tmp_path, extra):
    extra = [str(tmp_path / e) if e in ("ip.json", "ref.yuv") else e for e in extra]
    r = _decode(tmp_path, extra)
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "ip.json").exists()


@pytest.mark.parametrize("value", ["2", "3", "8"])
def test_a_good_frame_step_passes_the_flag_checks(tmp_path, value):
    r = _encode(tmp_path, ["--frame-step", value])
    assert r.returncode == 2 and "--frame-step" not in r.stderr, r.stderr
