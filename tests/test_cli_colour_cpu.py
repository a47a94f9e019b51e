"""The dcvc tool's refusals for --matrix / --range / --yuv-depth: each is decided by the flags alone, before a model is loaded
or the device is touched - the weight files named here do not exist, and no GPU is needed - and no output file is created."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
YUV_TYPES = ["yuv420", "yuv422", "yuv444", "nv12", "p010"]


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.rgb"), "-o", str(tmp_path / "o.bin"),
                 "-W", "128", "-H", "96"] + extra)


def _decode(tmp_path, extra):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path / "o.rgb")]
                + extra)


def _both(tmp_path, extra):
    yield "encode", _encode(tmp_path, extra)
    yield "decode", _decode(tmp_path, extra)


def _no_output(tmp_path):
    return not (tmp_path / "o.bin").exists() and not (tmp_path / "o.rgb").exists()


@pytest.mark.parametrize("src_type", ["rgb24", "png"])
def test_unknown_names_are_refused(tmp_path, src_type):
    for name in ("bt470", "709", "BT601", ""):
        for mode, r in _both(tmp_path, ["--src-type", src_type, "--matrix", name]):
            assert r.returncode == 2 and "unknown --matrix " + name in r.stderr and "bt601, bt709 or bt2020" in r.stderr, (mode, r.stderr)
    for name in ("tv", "pc", "Limited", ""):
        for mode, r in _both(tmp_path, ["--src-type", src_type, "--range", name]):
            assert r.returncode == 2 and "unknown --range " + name in r.stderr and "full or limited" in r.stderr, (mode, r.stderr)
    assert _no_output(tmp_path)


def test_yuv_depth_is_checked_and_needs_limited_range(tmp_path):
    for bad in ("7", "17", "0", "-8", "ten", "10.5", ""):
        for mode, r in _both(tmp_path, ["--src-type", "rgb24", "--range", "limited", "--yuv-depth", bad]):
            assert r.returncode == 2 and "--yuv-depth must be in 8..16, got " + bad in r.stderr, (mode, bad, r.stderr)
    for extra in ([], ["--range", "full"], ["--matrix", "bt2020"]):
        for mode, r in _both(tmp_path, ["--src-type", "png", "--yuv-depth", "10"] + extra):
            assert r.returncode == 2 and "--yuv-depth needs --range limited" in r.stderr, (mode, extra, r.stderr)
    assert _no_output(tmp_path)


@pytest.mark.parametrize("src_type", YUV_TYPES + [None])
def test_the_flags_are_refused_for_yuv_sources(tmp_path, src_type):
    st = ["--src-type", src_type] if src_type else []            # no --src-type: yuv420
    for flags in (["--matrix", "bt601"], ["--range", "limited"], ["--matrix", "bt709", "--range", "full"],
                  ["--range", "limited", "--yuv-depth", "10"]):
        for mode, r in _both(tmp_path, st + flags):
            assert r.returncode == 2 and "are for --src-type rgb24 and png" in r.stderr, (mode, flags, r.stderr)
            assert (src_type or "yuv420") + " pictures are not converted" in r.stderr, (mode, flags, r.stderr)
    assert _no_output(tmp_path)


def test_a_y4m_source_with_the_flags_is_refused(tmp_path):
    """the type of a Y4M file is a YUV type whatever --src-type says: either the flags or the disagreement is refused"""
    with open(tmp_path / "in.y4m", "wb") as f:
        f.write(b"YUV4MPEG2 W128 H96 F30:1 Ip C420\nFRAME\n" + bytes(128 * 96 * 3 // 2))
    r = _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "o.bin"),
              "--matrix", "bt601"])
    assert r.returncode == 2 and "yuv420 pictures are not converted" in r.stderr, r.stderr
    r = _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "o.bin"),
              "--matrix", "bt601", "--src-type", "rgb24"])
    assert r.returncode == 2 and "not --src-type rgb24" in r.stderr, r.stderr
    assert _no_output(tmp_path)


@pytest.mark.parametrize("flags", [["--matrix", "bt601"], ["--range", "limited"], ["--matrix", "bt2020", "--range", "limited", "--yuv-depth", "10"],
                                   ["--matrix", "bt709", "--range", "full"], ["--range", "limited", "--yuv-depth", "16"]],
                         ids=lambda f: "_".join(f).replace("-", ""))
def test_valid_flags_pass_the_flag_checks(tmp_path, flags):
    # the model is next (encode --src-type png looks at its first picture before the model: decode alone)
    runs = list(_both(tmp_path, ["--src-type", "rgb24"] + flags)) + [("decode png", _decode(tmp_path, ["--src-type", "png"] + flags))]
    for mode, r in runs:
        assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, (mode, r.stderr)
    assert _no_output(tmp_path)
