"""What dcvc encode --deinterlace / --field-order / --deinterlace-out refuse before a model is loaded, without a
GPU: every refusal ends with status 2 and its message, and no model file has been opened by then."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra, source="missing.yuv", size=("-W", "352", "-H", "288")):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / source), "-o", str(tmp_path / "o.bin")]
                + list(size) + extra)


def _decode(tmp_path, extra):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path / "o.yuv")]
                + extra)


def _refused(r, tmp_path, words):
    assert r.returncode == 2 and words in r.stderr, r.stderr
    assert "missing.dcvw" not in r.stderr, r.stderr          # before a model is loaded
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "o.yuv").exists() and not (tmp_path / "di.yuv").exists()


@pytest.mark.parametrize("value", ["", "weave", "frame:", "frame:65", "field:-1", "field:a", ":10", "10", "frame:1:2", "frame:1.5", "Frame",
                                   "field: 8", "frame:100"])
def test_malformed_values_are_refused(tmp_path, value):
    _refused(_encode(tmp_path, ["--deinterlace", value]), tmp_path, "--deinterlace must be frame or field, or either with :T, T an integer in 0..64")


@pytest.mark.parametrize("value", ["", "top", "TFF", "tff "])
def test_a_malformed_field_order_is_refused(tmp_path, value):
    _refused(_encode(tmp_path, ["--deinterlace", "frame", "--field-order", value]), tmp_path, "--field-order must be tff or bff")


def test_the_companions_need_deinterlace(tmp_path):
    _refused(_encode(tmp_path, ["--field-order", "bff"]), tmp_path, "--field-order needs --deinterlace")
    _refused(_encode(tmp_path, ["--deinterlace-out", str(tmp_path / "di.yuv")]), tmp_path, "--deinterlace-out needs --deinterlace")
    _refused(_encode(tmp_path, ["--deinterlace", "field", "--deinterlace-out", "-"]), tmp_path, "--deinterlace-out needs a file name")


@pytest.mark.parametrize("src_type", ["nv12", "p010", "nv21", "rgb24", "png", "rgb48", "png16"])
def test_interleaved_and_rgb_sources_are_refused(tmp_path, src_type):
    _refused(_encode(tmp_path, ["--deinterlace", "frame", "--src-type", src_type]), tmp_path, "sources are not deinterlaced yet")


def test_the_flags_are_encoder_flags(tmp_path):
    _refused(_decode(tmp_path, ["--deinterlace", "frame"]), tmp_path, "--deinterlace is an encoder flag")
    _refused(_decode(tmp_path, ["--field-order", "tff"]), tmp_path, "--field-order is an encoder flag")
    _refused(_decode(tmp_path, ["--deinterlace-out", str(tmp_path / "di.yuv")]), tmp_path, "--deinterlace-out is an encoder flag")


def _y4m(tmp_path, field, name="in.y4m"):
    (tmp_path / name).write_bytes(("YUV4MPEG2 W32 H16 F25:1 %s C420jpeg\n" % field).encode() + (b"FRAME\n" + bytes(32 * 16 * 3 // 2)) * 2)
    return name


def test_a_field_order_that_disagrees_with_the_file_is_refused(tmp_path):
    r = _encode(tmp_path, ["--deinterlace", "frame", "--field-order", "tff"], source=_y4m(tmp_path, "Ib"), size=())
    _refused(r, tmp_path, "is bottom field first (Ib), not --field-order tff")
    r = _encode(tmp_path, ["--deinterlace", "field:4", "--field-order", "bff"], source=_y4m(tmp_path, "It"), size=())
    _refused(r, tmp_path, "is top field first (It), not --field-order bff")
    _refused(_encode(tmp_path, ["--deinterlace", "frame"], source=_y4m(tmp_path, "Im"), size=()), tmp_path, "interlaced material is not supported")


@pytest.mark.parametrize("field", ["It", "Ib"])
def test_without_the_flag_an_interlaced_file_is_refused_as_ever(tmp_path, field):
    r = _encode(tmp_path, [], source=_y4m(tmp_path, field), size=())
    _refused(r, tmp_path, "is no Y4M file: y4m_parse_header: field %s: interlaced material is not supported" % field)


def test_planes_of_one_row_are_refused(tmp_path):
    _refused(_encode(tmp_path, ["--deinterlace", "frame"], size=("-W", "32", "-H", "2")), tmp_path, "--deinterlace needs planes of at least 2 rows")


@pytest.mark.parametrize("extra,source", [
    (["--deinterlace", "frame"], None), (["--deinterlace", "field:0"], None), (["--deinterlace", "field:64", "--field-order", "bff"], None),
    (["--deinterlace", "frame", "--src-type", "yuv444", "--bit-depth", "12"], None), (["--deinterlace", "field", "--src-type", "v210"], None),
    (["--deinterlace", "frame:6", "--src-type", "uyvy", "--deinterlace-out", "di.yuv"], None),
    (["--deinterlace", "frame", "--field-order", "bff"], "Ib"), (["--deinterlace", "field"], "It"), (["--deinterlace", "field", "--field-order", "bff"], "Ip"),
])
def test_good_flags_pass_the_flag_checks(tmp_path, extra, source):
    extra = [str(tmp_path / e) if e == "di.yuv" else e for e in extra]
    r = _encode(tmp_path, extra) if source is None else _encode(tmp_path, extra, source=_y4m(tmp_path, source), size=())
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "di.yuv").exists()
