"""The dcvc tool's refusals for the other chroma formats and Y4M that the flags (and a Y4M header) alone decide: each happens
before a model is loaded or the device is touched - the weight files named here do not exist, and no GPU is needed - and no
output file is created."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
NEW_TYPES = ["yuv422", "yuv444", "nv12", "p010"]


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra, src="missing.yuv", size=("-W", "352", "-H", "288")):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / src), "-o", str(tmp_path / "o.bin")]
                + list(size) + extra)


def _decode(tmp_path, extra, out="o.yuv"):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path / out)]
                + extra)


def _y4m(path, head, frames=1, frame_bytes=0):
    with open(path, "wb") as f:
        f.write(head)
        for _ in range(frames):
            f.write(b"FRAME\n" + bytes(frame_bytes))


@pytest.mark.parametrize("src_type", NEW_TYPES)
def test_scale_and_out_size_are_refused_for_the_new_types(tmp_path, src_type):
    r = _encode(tmp_path, ["--scale", "176x144", "--src-type", src_type])
    assert r.returncode == 2 and src_type + " sources are not resampled yet" in r.stderr, r.stderr
    r = _decode(tmp_path, ["--out-size", "176x144", "--src-type", src_type])
    assert r.returncode == 2 and src_type + " sources are not resampled yet" in r.stderr, r.stderr
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "o.yuv").exists()


@pytest.mark.parametrize("src_type", ["nv12", "p010"])
def test_y4m_output_of_interleaved_chroma_is_refused(tmp_path, src_type):
    r = _decode(tmp_path, ["--src-type", src_type], out="rec.y4m")
    assert r.returncode == 2 and "Y4M has no tag for interleaved chroma" in r.stderr, r.stderr
    assert not (tmp_path / "rec.y4m").exists()


def test_y4m_output_of_rgb_and_a_bad_rate_are_refused(tmp_path):
    r = _decode(tmp_path, ["--src-type", "rgb24"], out="rec.y4m")
    assert r.returncode == 2 and "a Y4M file holds YUV pictures" in r.stderr, r.stderr
    for bad in ("25", "25:", ":1", "0:1", "25:0", "a:b", "25:1:1", "-25:1"):
        r = _decode(tmp_path, ["--fps", bad], out="rec.y4m")
        assert r.returncode == 2 and "--fps must be N:D" in r.stderr, (bad, r.stderr)
    r = _decode(tmp_path, ["--fps", "25:1"])
    assert r.returncode == 2 and "--fps is the rate in the header of -o *.y4m" in r.stderr, r.stderr
    assert not (tmp_path / "rec.y4m").exists() and not (tmp_path / "o.yuv").exists()


def test_p010_is_nv12_at_10_bits(tmp_path):
    r = _encode(tmp_path, ["--src-type", "p010", "--bit-depth", "12"])
    assert r.returncode == 2 and "p010 is nv12 at 10 bits" in r.stderr, r.stderr
    r = _encode(tmp_path, ["--src-type", "p010", "--bit-depth", "10"])           # passes the flag checks: the model is next
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    for t in NEW_TYPES:
        r = _encode(tmp_path, ["--src-type", t, "--bit-depth", "17"])
        assert r.returncode == 2 and "--bit-depth must be 8 or 9..16" in r.stderr, r.stderr
    r = _encode(tmp_path, ["--src-type", "yuv411"])
    assert r.returncode == 2 and "unknown --src-type yuv411" in r.stderr, r.stderr


DISAGREE = [
    (["-W", "352", "-H", "288"], "not the -W x -H given"),
    (["-H", "98"], "not the -W x -H given"),
    (["--src-type", "yuv420"], "not --src-type yuv420"),
    (["--src-type", "yuv422"], "not --src-type yuv422"),
    (["--src-type", "nv12"], "not --src-type nv12"),
    (["--src-type", "p010"], "not --src-type p010"),
    (["--src-type", "rgb24"], "not --src-type rgb24"),
    (["--bit-depth", "8"], "not the --bit-depth given"),
    (["--src-type", "yuv444", "--bit-depth", "12"], "not the --bit-depth given"),
]


@pytest.mark.parametrize("flags,why", DISAGREE, ids=["_".join(f[0]).replace("-", "") for f in DISAGREE])
def test_a_y4m_header_that_disagrees_with_the_flags_is_refused(tmp_path, flags, why):
    _y4m(tmp_path / "in.y4m", b"YUV4MPEG2 W128 H96 F30:1 Ip C444p10\n", 1, 128 * 96 * 3 * 2)
    r = _encode(tmp_path, flags, src="in.y4m", size=())
    assert r.returncode == 2 and why in r.stderr and "128x96 yuv444 pictures of 10 bits" in r.stderr, r.stderr
    assert not (tmp_path / "o.bin").exists()


def test_a_y4m_header_that_agrees_passes_the_flag_checks(tmp_path):
    _y4m(tmp_path / "in.y4m", b"YUV4MPEG2 W128 H96 F30:1 Ip C444p10\n", 1, 128 * 96 * 3 * 2)
    for flags in ([], ["-W", "128", "-H", "96", "--src-type", "yuv444", "--bit-depth", "10"]):
        r = _encode(tmp_path, flags, src="in.y4m", size=())
        assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    r = _encode(tmp_path, ["--scale", "64x48"], src="in.y4m", size=())           # the type comes from the header
    assert r.returncode == 2 and "yuv444 sources are not resampled yet" in r.stderr, r.stderr


def test_a_y4m_name_without_the_magic_and_refused_headers(tmp_path):
    (tmp_path / "raw.y4m").write_bytes(bytes(4096))
    r = _encode(tmp_path, [], src="raw.y4m")
    assert r.returncode == 2 and "is no Y4M file" in r.stderr and "no YUV4MPEG2 magic" in r.stderr, r.stderr
    for head, names in ((b"YUV4MPEG2 W128 H96 It C420\n", "It"), (b"YUV4MPEG2 W128 H96 Cmono\n", "Cmono"),
                        (b"YUV4MPEG2 W127 H96\n", "W127"), (b"YUV4MPEG2 W128\n", "no H field")):
        _y4m(tmp_path / "bad.y4m", head)
        r = _encode(tmp_path, [], src="bad.y4m", size=())
        assert r.returncode == 2 and "is no Y4M file" in r.stderr and names in r.stderr, r.stderr
    assert not (tmp_path / "o.bin").exists()
