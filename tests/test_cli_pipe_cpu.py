"""The dcvc tool's refusals around pipes that the flags alone decide: each happens before a model is loaded or
the device is touched - the weight files named here do not exist, and no GPU is needed - with status 2 and a message that
names the flag."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)


def _encode(tmp_path, extra, i=None, o=None):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", i or str(tmp_path / "missing.yuv"),
                 "-o", o or str(tmp_path / "o.bin"), "-W", "64", "-H", "48"] + extra)


def _decode(tmp_path, extra, i=None):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", i or str(tmp_path / "missing.bin")] + extra)


def _refused(r, *says):
    assert r.returncode == 2, (r.returncode, r.stderr)
    for s in says:
        assert s in r.stderr, r.stderr
    assert "missing.dcvw" not in r.stderr              # refused before a model is loaded
    assert r.stdout == ""


@pytest.fixture
def fifo(tmp_path):
    p = tmp_path / "pipe"
    os.mkfifo(p)
    return str(p)


@pytest.mark.parametrize("png", ["png", "png16"])
def test_png_directories_are_no_pipes(tmp_path, fifo, png):
    t = ["--src-type", png]
    for name in ("-", fifo):
        _refused(_encode(tmp_path, t, i=name), "-i " + name, "--src-type " + png, "directory")
        _refused(_encode(tmp_path, t, o=name), "-o " + name, "--src-type " + png, "directory")
        _refused(_decode(tmp_path, t + ["--ref", name]), "--ref " + name, "--src-type " + png, "directory")
        _refused(_decode(tmp_path, t + ["-o", name]), "-o " + name, "--src-type " + png, "directory")
    # decode -i is the stream, not a directory: stdin serves, and the model is next
    r = _decode(tmp_path, t + ["-o", str(tmp_path / "rec")], i="-")
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr


def test_stdin_cannot_carry_the_stream_and_the_reference(tmp_path):
    _refused(_decode(tmp_path, ["--ref", "-"], i="-"), "-i -", "--ref -")


@pytest.mark.parametrize("flag", ["--json", "--hash-log"])
def test_decode_logs_named_dash_are_refused(tmp_path, flag):
    _refused(_decode(tmp_path, ["-o", "-", "--ref", str(tmp_path / "in.yuv"), flag, "-"]), flag + " -", "standard output")
    _refused(_decode(tmp_path, ["--ref", str(tmp_path / "in.yuv"), flag, "-"]), flag + " -")


@pytest.mark.parametrize("flag,extra", [("--rc-log", ["--target-bpp", "0.5"]),
                                        ("--scene-log", ["--scene-cut", "5", "--inter", "missing_p.dcvw"]),
                                        ("--quality-log", []), ("--hash-log", []), ("--latency-log", [])])
def test_encode_logs_named_dash_are_refused(tmp_path, flag, extra):
    _refused(_encode(tmp_path, extra + [flag, "-"], o="-"), flag + " -", "standard output")
    _refused(_encode(tmp_path, extra + [flag, "-"]), flag + " -")


@pytest.mark.parametrize("value", ["yuv", "Y4M", "", "png"])
def test_format_values(tmp_path, value):
    _refused(_encode(tmp_path, ["--in-format", value]), "--in-format must be raw or y4m")
    _refused(_decode(tmp_path, ["--in-format", value, "--ref", "-"]), "--in-format must be raw or y4m")
    _refused(_decode(tmp_path, ["--out-format", value, "-o", "-"]), "--out-format must be raw or y4m")


def test_the_good_values_pass_the_flag_checks(tmp_path):
    for extra in (["--in-format", "raw"], ["--src-type", "v210", "--in-format", "raw", "--read-ahead", "0"], ["--read-ahead", "8", "--flush-units", "1"],
                  ["--latency-log", str(tmp_path / "lat.json")]):
        r = _encode(tmp_path, extra, o="-")
        assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    for extra in (["--out-format", "y4m", "-o", "-"], ["--out-format", "raw", "-o", "-", "--in-format", "y4m", "--ref", str(tmp_path / "r")]):
        r = _decode(tmp_path, extra, i="-")
        assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "lat.json").exists()


WIRE = ["nv21", "nv16", "p210", "uyvy", "yuy2", "y210", "v210"]


@pytest.mark.parametrize("t", WIRE + ["nv12", "p010", "rgb24", "rgb48"])
def test_y4m_format_with_a_type_y4m_cannot_hold(tmp_path, t):
    # in the words of the refusals for names ending in .y4m
    says = "Y4M has no tag for --src-type " + t if t in WIRE else \
        "Y4M has no tag for interleaved chroma (--src-type %s)" % t if t in ("nv12", "p010") else \
        "a Y4M file holds YUV pictures, not --src-type " + t
    _refused(_encode(tmp_path, ["--src-type", t, "--in-format", "y4m"], i="-"), "--in-format y4m", says)
    _refused(_decode(tmp_path, ["--src-type", t, "--in-format", "y4m", "--ref", "-"]), "--in-format y4m", says)
    _refused(_decode(tmp_path, ["--src-type", t, "--out-format", "y4m", "-o", "-"]), "--out-format y4m", says)


@pytest.mark.parametrize("value", ["-1", "9", "two", "", "2.5"])
def test_read_ahead_range(tmp_path, value):
    _refused(_encode(tmp_path, ["--read-ahead", value]), "--read-ahead must be in 0..8")


@pytest.mark.parametrize("flag,value", [("--read-ahead", "2"), ("--flush-units", "1"), ("--latency-log", "lat.json")])
def test_encoder_flags_on_decode(tmp_path, flag, value):
    _refused(_decode(tmp_path, [flag, value]), flag, "encoder flag")


def test_out_format_on_encode_and_flush_units_values(tmp_path):
    _refused(_encode(tmp_path, ["--out-format", "raw"]), "--out-format is a decoder flag")
    _refused(_encode(tmp_path, ["--flush-units", "2"]), "--flush-units must be in 0..1")
