"""What dcvc encode --crop / --crop-log / --crop-out / --crop-fill and dcvc decode --uncrop / --pad / --pad-fill refuse before a
model is loaded, without a GPU: every refusal ends with status 2 and its message, and no model file has been
opened by then."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
FORM = "--crop must be auto, auto:LIMIT[:FRAC[:MINBAR[:N]]] with integers in 0..255, 0..255, 0..4096 and 1..256, or WxH+X+Y"
OUTPUTS = ("o.bin", "o.yuv", "c.yuv", "c.json", "h.txt")


def _run(args, stdin=None):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120, stdin=stdin)


def _encode(tmp_path, extra, source="missing.yuv", size=("-W", "352", "-H", "288"), stdin=None):
    src = source if source == "-" else str(tmp_path / source)
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", src, "-o", str(tmp_path / "o.bin")] + list(size) + extra, stdin)


def _decode(tmp_path, extra, out=True):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin")]
                + (["-o", str(tmp_path / "o.yuv")] if out else []) + extra)


def _refused(r, tmp_path, words):
    assert r.returncode == 2 and words in r.stderr, r.stderr
    assert "missing.dcvw" not in r.stderr, r.stderr          # before a model is loaded
    for name in OUTPUTS:
        assert not (tmp_path / name).exists()


@pytest.mark.parametrize("value", ["", "Auto", "auto:", "auto:256", "auto:-1", "auto:24:256", "auto:24:4:4097", "auto:24:4:8:0", "auto:24:4:8:257",
                                   "auto:24:4:8:16:1", "auto:a", "auto::4", "autox", "auto 24", "auto:1.5", "auto:024", "320x240", "320x240+0",
                                   "320x240+0+", "x240+0+0", "320x+0+0", "320x240-8+0", "+0+0", "320:240+0+0", "320x240+a+0", "20000x240+0+0",
                                   "320x240+0+0+0", "manual"])
def test_malformed_values_are_refused(tmp_path, value):
    _refused(_encode(tmp_path, ["--crop", value]), tmp_path, FORM)


def test_the_companions_need_crop(tmp_path):
    _refused(_encode(tmp_path, ["--crop-out", str(tmp_path / "c.yuv")]), tmp_path, "--crop-out needs --crop")
    _refused(_encode(tmp_path, ["--crop-log", str(tmp_path / "c.json")]), tmp_path, "--crop-log needs --crop")
    _refused(_encode(tmp_path, ["--crop-fill", "16:128:128"]), tmp_path, "--crop-fill needs --crop")
    for mode in ("auto", "352x240+0+24"):
        _refused(_encode(tmp_path, ["--crop", mode, "--crop-out", "-"]), tmp_path, "--crop-out needs a file name")
        _refused(_encode(tmp_path, ["--crop", mode, "--crop-out", ""]), tmp_path, "--crop-out needs a file name")
        _refused(_encode(tmp_path, ["--crop", mode, "--crop-log", "-"]), tmp_path, "--crop-log needs a file name")
        _refused(_encode(tmp_path, ["--crop", mode, "--crop-log", ""]), tmp_path, "--crop-log needs a file name")
    for fill in ("", "16", "16:128", "16:128:128:0", "16:128:x", "16:128:65536", "-1:0:0"):
        _refused(_encode(tmp_path, ["--crop", "352x240+0+24", "--crop-fill", fill]), tmp_path, "--crop-fill must be Y:U:V")
    _refused(_encode(tmp_path, ["--crop", "352x240+0+24", "--crop-fill", "16:128:256"]), tmp_path, "--crop-fill: 256 is no sample of 8 bits")


@pytest.mark.parametrize("src_type", ["nv12", "p010", "nv21", "rgb24", "png", "rgb48", "png16"])
def test_interleaved_and_rgb_sources_are_refused(tmp_path, src_type):
    _refused(_encode(tmp_path, ["--crop", "auto", "--src-type", src_type]), tmp_path, "sources are not cropped yet")
    _refused(_encode(tmp_path, ["--crop", "320x240+0+0", "--src-type", src_type]), tmp_path, "sources are not cropped yet")


def test_auto_needs_a_seekable_source(tmp_path):
    words = "--crop auto needs a seekable source; give --crop WxH+X+Y"
    _refused(_encode(tmp_path, ["--crop", "auto"], source="-", stdin=subprocess.DEVNULL), tmp_path, words)
    fifo = tmp_path / "in.fifo"
    os.mkfifo(fifo)
    _refused(_encode(tmp_path, ["--crop", "auto:24:4"], source="in.fifo"), tmp_path, words)


@pytest.mark.parametrize("window,extra,words", [
    ("352x288+0+2", [], "does not lie inside the 352x288 picture"),
    ("354x288+0+0", [], "does not lie inside the 352x288 picture"),
    ("352x240+2+24", [], "does not lie inside the 352x288 picture"),
    ("0x240+0+24", [], "the window's sides must be positive"),
    ("352x0+0+24", [], "the window's sides must be positive"),
    ("351x240+0+24", [], "offsets and sides must be multiples of 2 (horizontal) and 2 (vertical)"),
    ("350x240+1+24", [], "offsets and sides must be multiples of 2 (horizontal) and 2 (vertical)"),
    ("352x239+0+24", [], "offsets and sides must be multiples of 2 (horizontal) and 2 (vertical)"),
    ("352x240+0+23", [], "offsets and sides must be multiples of 2 (horizontal) and 2 (vertical)"),
    ("351x240+0+24", ["--src-type", "yuv444"], "offsets and sides must be multiples of 2 (horizontal) and 2 (vertical)"),
    ("352x239+0+24", ["--src-type", "yuv422"], "offsets and sides must be multiples of 2 (horizontal) and 2 (vertical)"),
    # field rows: a window that is fine for progressive material breaks the alignment under --deinterlace and --ivtc
    ("352x240+0+22", ["--deinterlace", "frame"], "multiples of 2 (horizontal) and 4 (vertical) for this source (field rows"),
    ("352x238+0+24", ["--deinterlace", "field:4"], "multiples of 2 (horizontal) and 4 (vertical) for this source (field rows"),
    ("352x240+0+22", ["--ivtc", "film"], "multiples of 2 (horizontal) and 4 (vertical) for this source (field rows"),
    ("352x240+0+22", ["--ivtc", "match", "--src-type", "uyvy"], "multiples of 2 (horizontal) and 4 (vertical) for this source (field rows"),
])
def test_a_manual_window_that_does_not_fit_is_refused(tmp_path, window, extra, words):
    _refused(_encode(tmp_path, ["--crop", window] + extra), tmp_path, words)


def _y4m(tmp_path, name="in.y4m"):
    (tmp_path / name).write_bytes(b"YUV4MPEG2 W32 H16 F25:1 Ip C420jpeg\n" + (b"FRAME\n" + bytes(32 * 16 * 3 // 2)) * 2)
    return name


def test_a_manual_window_against_a_y4m_header(tmp_path):
    _refused(_encode(tmp_path, ["--crop", "32x12+0+6"], source=_y4m(tmp_path), size=()), tmp_path, "does not lie inside the 32x16 picture")
    _refused(_encode(tmp_path, ["--crop", "32x10+0+3"], source=_y4m(tmp_path), size=()), tmp_path, "offsets and sides must be multiples")


def test_the_flags_belong_to_one_side(tmp_path):
    _refused(_decode(tmp_path, ["--crop", "auto"]), tmp_path, "--crop is an encoder flag")
    _refused(_decode(tmp_path, ["--crop-out", str(tmp_path / "c.yuv")]), tmp_path, "--crop-out is an encoder flag")
    _refused(_decode(tmp_path, ["--crop-log", str(tmp_path / "c.json")]), tmp_path, "--crop-log is an encoder flag")
    _refused(_decode(tmp_path, ["--crop-fill", "16:128:128"]), tmp_path, "--crop-fill is an encoder flag")
    _refused(_encode(tmp_path, ["--uncrop", str(tmp_path / "c.json")]), tmp_path, "--uncrop is a decoder flag")
    _refused(_encode(tmp_path, ["--pad", "352x288+0+24"]), tmp_path, "--pad is a decoder flag")
    _refused(_encode(tmp_path, ["--pad-fill", "16:128:128"]), tmp_path, "--pad-fill is a decoder flag")


@pytest.mark.parametrize("extra", [
    ["--crop", "352x240+0+24"], ["--crop", "320x288+16+0"], ["--crop", "352x288+0+0"], ["--crop", "2x2+350+286"],
    ["--crop", "352x240+0+24", "--crop-fill", "0:0:255", "--crop-out", "c.yuv", "--crop-log", "c.json"],
    ["--crop", "352x240+0+24", "--src-type", "yuv444", "--bit-depth", "12", "--crop-fill", "64:2048:4095"],
    ["--crop", "352x240+0+24", "--src-type", "yuv422"], ["--crop", "352x240+0+24", "--src-type", "v210"],
    ["--crop", "352x240+0+24", "--deinterlace", "frame"], ["--crop", "348x240+4+24", "--ivtc", "film", "--src-type", "uyvy"],
])
def test_good_manual_flags_pass_the_flag_checks(tmp_path, extra):
    extra = [str(tmp_path / e) if e in ("c.yuv", "c.json") else e for e in extra]
    r = _encode(tmp_path, extra)
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "c.yuv").exists()


# ---------------------------------------------------------------- decode
def _log(tmp_path, **over):
    d = {"mode": "auto", "limit": 24, "frac": 4, "min_bar": 8, "source_width": 96, "source_height": 64, "src_type": "yuv420",
         "chroma_format": "yuv420", "bit_depth": 8,
         "probes": [{"idx": 0, "voted": False, "top": None, "bottom": None, "left": None, "right": None},
                    {"idx": 1, "voted": True, "top": 12, "bottom": 51, "left": 0, "right": 95}],
         "votes": 1, "window": {"x": 0, "y": 12, "width": 96, "height": 40}, "fill": [16, 128, 128]}
    d.update(over)
    d = {k: v for k, v in d.items() if v is not None}
    p = tmp_path / "crop.json"
    p.write_text(json.dumps(d))
    return str(p)


def test_decode_flag_refusals(tmp_path):
    log = _log(tmp_path)
    _refused(_decode(tmp_path, ["--uncrop", log, "--pad", "96x64+0+12"]), tmp_path, "--uncrop and --pad: exactly one of them may be given")
    _refused(_decode(tmp_path, ["--pad-fill", "16:128:128"]), tmp_path, "--pad-fill needs --uncrop or --pad")
    _refused(_decode(tmp_path, ["--uncrop", log], out=False), tmp_path, "--uncrop changes what -o writes and the hashes cover")
    _refused(_decode(tmp_path, ["--pad", "96x64+0+12"], out=False), tmp_path, "--pad changes what -o writes and the hashes cover")
    for value in ("", "96x64", "96x64+0", "96+64+0+0", "96x64+0+a", "96x64+0+-2", "0x64+0+0", "96x1+0+0", "20000x64+0+0"):
        _refused(_decode(tmp_path, ["--pad", value]), tmp_path, "--pad must be SWxSH+X+Y")
    for fill in ("", "16", "16:128", "16:128:128:0", "a:b:c", "16:128:65536"):
        _refused(_decode(tmp_path, ["--pad", "96x64+0+12", "--pad-fill", fill]), tmp_path, "--pad-fill must be Y:U:V")
    for src_type in ("nv12", "p010", "nv21", "uyvy", "v210", "rgb24", "png", "rgb48"):
        _refused(_decode(tmp_path, ["--pad", "96x64+0+12", "--src-type", src_type]), tmp_path, "pictures are not padded yet")
        _refused(_decode(tmp_path, ["--uncrop", log, "--src-type", src_type]), tmp_path, "pictures are not padded yet")
    _refused(_decode(tmp_path, ["--uncrop", str(tmp_path / "nothing.json")]), tmp_path, "--uncrop: cannot open")


@pytest.mark.parametrize("over,words", [
    (dict(source_width=None), '"source_width" must be an integer in 2..16384'),
    (dict(source_height=1), '"source_height" must be an integer in 2..16384'),
    (dict(bit_depth=7), '"bit_depth" must be an integer in 8..16'),
    (dict(chroma_format="nv12"), '"chroma_format" must be yuv420, yuv422 or yuv444'),
    (dict(chroma_format=None), '"chroma_format" must be yuv420, yuv422 or yuv444'),
    (dict(window=None), '"window" must be an object'),
    (dict(window=[0, 12, 96, 40]), '"window" must be an object'),
    (dict(window={"x": 0, "y": 12, "width": 96}), '"height" must be an integer'),
    (dict(window={"x": 0, "y": 30, "width": 96, "height": 40}), "the window does not lie inside the source"),
    (dict(window={"x": 2, "y": 12, "width": 96, "height": 40}), "the window does not lie inside the source"),
    (dict(fill=[16, 128]), '"fill" must be a list of 3'),
    (dict(fill=[16, 128, 70000]), '"fill" holds integers in 0..65535'),
    (dict(fill=None), '"fill" must be a list of 3'),
])
def test_a_malformed_crop_log_is_refused(tmp_path, over, words):
    _refused(_decode(tmp_path, ["--uncrop", _log(tmp_path, **over)]), tmp_path, "is no crop log: " + words)


def test_text_that_is_no_json_is_refused(tmp_path):
    p = tmp_path / "crop.json"
    for text in ("", "[1, 2]", '{"source_width": 96', '{"source_width": 96} x', '{"source_width": nil}'):
        p.write_text(text)
        _refused(_decode(tmp_path, ["--uncrop", str(p)]), tmp_path, "is no crop log")


def test_a_log_of_another_depth_or_chroma_format_is_refused(tmp_path):
    _refused(_decode(tmp_path, ["--uncrop", _log(tmp_path, bit_depth=10)]), tmp_path,
             "--uncrop: the log describes yuv420 pictures of 10 bits, this run's are yuv420 of 8 bits")
    _refused(_decode(tmp_path, ["--uncrop", _log(tmp_path), "--bit-depth", "10"]), tmp_path,
             "--uncrop: the log describes yuv420 pictures of 8 bits, this run's are yuv420 of 10 bits")
    _refused(_decode(tmp_path, ["--uncrop", _log(tmp_path, chroma_format="yuv422")]), tmp_path,
             "--uncrop: the log describes yuv422 pictures of 8 bits, this run's are yuv420 of 8 bits")
    _refused(_decode(tmp_path, ["--uncrop", _log(tmp_path), "--src-type", "yuv444"]), tmp_path,
             "--uncrop: the log describes yuv420 pictures of 8 bits, this run's are yuv444 of 8 bits")


@pytest.mark.parametrize("extra", [["--uncrop", "LOG"], ["--pad", "96x64+0+12"], ["--pad", "96x64+0+12", "--pad-fill", "0:0:0"],
                                   ["--uncrop", "LOG", "--pad-fill", "235:128:128"], ["--uncrop", "LOG", "--hash-log", "h.txt"]])
def test_good_decoder_flags_pass_the_flag_checks(tmp_path, extra):
    extra = [_log(tmp_path) if e == "LOG" else str(tmp_path / e) if e == "h.txt" else e for e in extra]
    r = _decode(tmp_path, extra)
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
