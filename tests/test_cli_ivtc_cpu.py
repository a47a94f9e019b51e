"""What dcvc encode --ivtc / --ivtc-out / --ivtc-log refuse before a model is loaded, without a GPU: every refusal
ends with status 2 and its message, and no model file has been opened by then."""
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
    for name in ("o.bin", "o.yuv", "iv.yuv", "iv.json"):
        assert not (tmp_path / name).exists()


@pytest.mark.parametrize("value", ["", "frame", "field", "Film", "film:", "film:256", "film:-1", "match:a", ":9", "9", "film:9:513", "film:9:80:65",
                                   "film:9:80:10:1", "match:9:", "match:9::10", "film: 9", "film:1.5", "film:1000", "match:9:80:", "ivtc"])
def test_malformed_values_are_refused(tmp_path, value):
    _refused(_encode(tmp_path, ["--ivtc", value]), tmp_path,
             "--ivtc must be film or match, or either with :CTHRESH[:MI[:T]], integers in 0..255, 0..512 and 0..64")


@pytest.mark.parametrize("value", ["", "top", "TFF", "tff "])
def test_a_malformed_field_order_is_refused(tmp_path, value):
    _refused(_encode(tmp_path, ["--ivtc", "film", "--field-order", value]), tmp_path, "--field-order must be tff or bff")


def test_the_companions_need_ivtc(tmp_path):
    _refused(_encode(tmp_path, ["--ivtc-out", str(tmp_path / "iv.yuv")]), tmp_path, "--ivtc-out needs --ivtc")
    _refused(_encode(tmp_path, ["--ivtc-log", str(tmp_path / "iv.json")]), tmp_path, "--ivtc-log needs --ivtc")
    _refused(_encode(tmp_path, ["--ivtc", "film", "--ivtc-out", "-"]), tmp_path, "--ivtc-out needs a file name")
    _refused(_encode(tmp_path, ["--ivtc", "film", "--ivtc-out", ""]), tmp_path, "--ivtc-out needs a file name")
    _refused(_encode(tmp_path, ["--ivtc", "match", "--ivtc-log", "-"]), tmp_path, "--ivtc-log needs a file name")
    _refused(_encode(tmp_path, ["--ivtc", "match", "--ivtc-log", ""]), tmp_path, "--ivtc-log needs a file name")
    # the sentence of DESIGN.md 27, extended
    _refused(_encode(tmp_path, ["--field-order", "bff"]), tmp_path, "--field-order needs --deinterlace or --ivtc")


@pytest.mark.parametrize("mode", ["frame", "field:4"])
def test_ivtc_and_deinterlace_exclude_each_other(tmp_path, mode):
    _refused(_encode(tmp_path, ["--ivtc", "film", "--deinterlace", mode]), tmp_path, "--ivtc and --deinterlace exclude each other")
    _refused(_encode(tmp_path, ["--deinterlace", mode, "--ivtc", "match:9"]), tmp_path, "--ivtc and --deinterlace exclude each other")


@pytest.mark.parametrize("src_type", ["nv12", "p010", "nv21", "rgb24", "png", "rgb48", "png16"])
def test_interleaved_and_rgb_sources_are_refused(tmp_path, src_type):
    _refused(_encode(tmp_path, ["--ivtc", "film", "--src-type", src_type]), tmp_path, "sources are not deinterlaced yet")


def test_the_flags_are_encoder_flags(tmp_path):
    _refused(_decode(tmp_path, ["--ivtc", "film"]), tmp_path, "--ivtc is an encoder flag")
    _refused(_decode(tmp_path, ["--ivtc-out", str(tmp_path / "iv.yuv")]), tmp_path, "--ivtc-out is an encoder flag")
    _refused(_decode(tmp_path, ["--ivtc-log", str(tmp_path / "iv.json")]), tmp_path, "--ivtc-log is an encoder flag")


def _y4m(tmp_path, field, name="in.y4m"):
    (tmp_path / name).write_bytes(("YUV4MPEG2 W32 H16 F30000:1001 %s C420jpeg\n" % field).encode() + (b"FRAME\n" + bytes(32 * 16 * 3 // 2)) * 2)
    return name


def test_a_field_order_that_disagrees_with_the_file_is_refused(tmp_path):
    r = _encode(tmp_path, ["--ivtc", "film", "--field-order", "tff"], source=_y4m(tmp_path, "Ib"), size=())
    _refused(r, tmp_path, "is bottom field first (Ib), not --field-order tff")
    r = _encode(tmp_path, ["--ivtc", "match:9:80", "--field-order", "bff"], source=_y4m(tmp_path, "It"), size=())
    _refused(r, tmp_path, "is top field first (It), not --field-order bff")
    _refused(_encode(tmp_path, ["--ivtc", "film"], source=_y4m(tmp_path, "Im"), size=()), tmp_path, "interlaced material is not supported")


def test_planes_of_one_row_are_refused(tmp_path):
    _refused(_encode(tmp_path, ["--ivtc", "film"], size=("-W", "32", "-H", "2")), tmp_path, "--ivtc needs planes of at least 2 rows")


@pytest.mark.parametrize("extra,source", [
    (["--ivtc", "film"], None), (["--ivtc", "match"], None), (["--ivtc", "film:0"], None), (["--ivtc", "match:255:512:64", "--field-order", "bff"], None),
    (["--ivtc", "film:9:80"], None), (["--ivtc", "film", "--src-type", "yuv444", "--bit-depth", "12"], None),
    (["--ivtc", "match", "--src-type", "v210"], None), (["--ivtc", "film:9:80:6", "--src-type", "uyvy", "--ivtc-out", "iv.yuv", "--ivtc-log", "iv.json"], None),
    (["--ivtc", "film", "--field-order", "bff"], "Ib"), (["--ivtc", "match"], "It"), (["--ivtc", "film", "--field-order", "bff"], "Ip"),
])
def test_good_flags_pass_the_flag_checks(tmp_path, extra, source):
    extra = [str(tmp_path / e) if e in ("iv.yuv", "iv.json") else e for e in extra]
    r = _encode(tmp_path, extra) if source is None else _encode(tmp_path, extra, source=_y4m(tmp_path, source), size=())
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "iv.yuv").exists() and not (tmp_path / "iv.json").exists()
