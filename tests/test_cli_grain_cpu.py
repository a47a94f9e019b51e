"""What dcvc refuses of the film-grain flags before a model is loaded, without a GPU: encode --grain-log and its
options, decode --film-grain / --grain-strength. Every refusal ends with status 2 and its message, and no model file has been
opened by then."""
import copy
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.yuv"), "-o", str(tmp_path / "o.bin"),
                 "-W", "352", "-H", "288"] + extra)


def _decode(tmp_path, extra, out=True):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin")]
                + (["-o", str(tmp_path / "o.yuv")] if out else []) + extra)


def _refused(r, tmp_path, words):
    assert r.returncode == 2 and words in r.stderr, r.stderr
    assert "missing.dcvw" not in r.stderr, r.stderr          # before a model is loaded
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "o.yuv").exists() and not (tmp_path / "g.json").exists()


def _accepted(r):
    """the flags pass: the run gets as far as the model file, which does not exist"""
    assert r.returncode != 0 and "missing.dcvw" in r.stderr, r.stderr


GOOD = {
    "version": 1, "bit_depth": 8, "chroma_format": "yuv420", "width": 352, "height": 288, "denoise": [8, 8],
    "records": [
        {"first": 0, "pictures": 2, "seed": 1, "size": 12, "y": [16] * 9, "u": [8] * 9, "v": [8] * 9, "words": [[1000] * 16] * 3},
        {"first": 2, "pictures": 3, "seed": 2, "size": 12, "y": [0] * 9, "u": [255] * 9, "v": [8] * 9, "words": [[0] * 16] * 3},
    ],
}


def _file(tmp_path, doc, name="grain.json"):
    (tmp_path / name).write_text(doc if isinstance(doc, str) else json.dumps(doc))
    return str(tmp_path / name)


# ------------------------------------------------------------------------------------ encode
def test_grain_log_needs_denoise_and_a_file_name(tmp_path):
    log = str(tmp_path / "g.json")
    _refused(_encode(tmp_path, ["--grain-log", log]), tmp_path, "--grain-log needs --denoise")
    _refused(_encode(tmp_path, ["--denoise", "8", "--grain-log", "-"]), tmp_path, "--grain-log needs a file name")
    _refused(_encode(tmp_path, ["--denoise", "8", "--grain-log", ""]), tmp_path, "--grain-log needs a file name")
    _accepted(_encode(tmp_path, ["--denoise", "8", "--grain-log", log]))
    _accepted(_encode(tmp_path, ["--denoise", "8:4", "--grain-log", log, "--grain-size", "37", "--grain-window", "0", "--grain-gain", "400",
                                 "--grain-flat", "255", "--grain-seed", "4294967295"]))


@pytest.mark.parametrize("flag", ["grain-size", "grain-window", "grain-gain", "grain-flat", "grain-seed"])
def test_the_options_need_grain_log(tmp_path, flag):
    _refused(_encode(tmp_path, ["--denoise", "8", "--" + flag, "1"]), tmp_path, "--%s needs --grain-log" % flag)


@pytest.mark.parametrize("flag,value", [("grain-size", "38"), ("grain-size", "-1"), ("grain-size", "a"), ("grain-size", ""), ("grain-size", "1.5"),
                                        ("grain-window", "-1"), ("grain-window", "x"), ("grain-gain", "0"), ("grain-gain", "401"),
                                        ("grain-flat", "256"), ("grain-flat", "-1"), ("grain-seed", "4294967296"), ("grain-seed", "-1"),
                                        ("grain-size", "012")])
def test_malformed_options_are_refused(tmp_path, flag, value):
    r = _encode(tmp_path, ["--denoise", "8", "--grain-log", str(tmp_path / "g.json"), "--" + flag, value])
    _refused(r, tmp_path, "--%s must be an integer in" % flag)


def test_the_source_types_are_denoises(tmp_path):
    r = _encode(tmp_path, ["--denoise", "8", "--grain-log", str(tmp_path / "g.json"), "--src-type", "nv12"])
    _refused(r, tmp_path, "nv12 sources are not filtered yet")


@pytest.mark.parametrize("flag,value", [("film-grain", "x.json"), ("grain-strength", "16")])
def test_the_decoder_flags_are_refused_on_encode(tmp_path, flag, value):
    _refused(_encode(tmp_path, ["--denoise", "8", "--" + flag, value]), tmp_path, "--%s is a decoder flag" % flag)


# ------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("flag", ["grain-log", "grain-size", "grain-window", "grain-gain", "grain-flat", "grain-seed"])
def test_the_encoder_flags_are_refused_on_decode(tmp_path, flag):
    _refused(_decode(tmp_path, ["--" + flag, "1"]), tmp_path, "--%s is an encoder flag" % flag)


def test_exactly_one_of_the_two_flags(tmp_path):
    r = _decode(tmp_path, ["--film-grain", _file(tmp_path, GOOD), "--grain-strength", "16"])
    _refused(r, tmp_path, "exactly one of them")


@pytest.mark.parametrize("flag,value", [("film-grain", None), ("grain-strength", "16")])
def test_the_flag_needs_an_output_or_a_hash(tmp_path, flag, value):
    value = value or _file(tmp_path, GOOD)
    _refused(_decode(tmp_path, ["--" + flag, value], out=False), tmp_path, "it needs -o, --hash-log or --verify-hash")
    _accepted(_decode(tmp_path, ["--" + flag, value]))
    _accepted(_decode(tmp_path, ["--" + flag, value, "--hash-log", str(tmp_path / "h.txt")], out=False))


@pytest.mark.parametrize("value", ["", "256", "-1", "a", "16:", ":16", "16:256", "16:8:38", "16:8:12:1", "16.5", "16:8:", "016", "16 "])
def test_a_malformed_strength_is_refused(tmp_path, value):
    _refused(_decode(tmp_path, ["--grain-strength", value]), tmp_path, "--grain-strength must be Y, Y:C or Y:C:SIZE")


@pytest.mark.parametrize("value", ["0", "255", "16:8", "16:8:0", "255:255:37"])
def test_a_strength_is_accepted(tmp_path, value):
    _accepted(_decode(tmp_path, ["--grain-strength", value]))
    _accepted(_decode(tmp_path, ["--grain-strength", value, "--src-type", "yuv444", "--bit-depth", "12"]))


@pytest.mark.parametrize("src_type", ["nv12", "p010", "nv21", "nv16", "p210", "uyvy", "yuy2", "y210", "v210", "rgb24", "png", "rgb48", "png16"])
def test_other_picture_types_are_refused(tmp_path, src_type):
    _refused(_decode(tmp_path, ["--grain-strength", "16", "--src-type", src_type]), tmp_path, src_type + " pictures are not grained yet")
    _refused(_decode(tmp_path, ["--film-grain", _file(tmp_path, GOOD), "--src-type", src_type]), tmp_path, src_type + " pictures are not grained yet")


def test_a_file_of_another_depth_or_chroma_format_is_refused(tmp_path):
    f = _file(tmp_path, GOOD)
    _accepted(_decode(tmp_path, ["--film-grain", f]))
    _refused(_decode(tmp_path, ["--film-grain", f, "--bit-depth", "10"]), tmp_path, "the file describes yuv420 pictures of 8 bits, this run's are yuv420 of 10")
    _refused(_decode(tmp_path, ["--film-grain", f, "--src-type", "yuv422"]), tmp_path, "this run's are yuv422 of 8 bits")
    doc = dict(GOOD, bit_depth=10, chroma_format="yuv444")
    _accepted(_decode(tmp_path, ["--film-grain", _file(tmp_path, doc), "--bit-depth", "10", "--src-type", "yuv444"]))
    _refused(_decode(tmp_path, ["--film-grain", _file(tmp_path, doc)]), tmp_path, "the file describes yuv444 pictures of 10 bits")


def _edit(path, value):
    doc = copy.deepcopy(GOOD)
    at = doc
    for k in path[:-1]:
        at = at[k]
    if value is None:
        del at[path[-1]]
    else:
        at[path[-1]] = value
    return doc


MALFORMED = [
    ("no file", None),
    ("empty", ""),
    ("no json", "grain"),
    ("a list", "[1, 2]"),
    ("text behind the value", json.dumps(GOOD) + " x"),
    ("cut short", json.dumps(GOOD)[:-20]),
    ("a float", json.dumps(GOOD).replace('"seed": 1', '"seed": 1.5')),
    ("a negative number", json.dumps(GOOD).replace('"seed": 1', '"seed": -1')),
    ("true", json.dumps(GOOD).replace('"seed": 1', '"seed": true')),
    ("version 2", _edit(["version"], 2)),
    ("no version", _edit(["version"], None)),
    ("bit_depth 7", _edit(["bit_depth"], 7)),
    ("bit_depth 17", _edit(["bit_depth"], 17)),
    ("bit_depth as a string", _edit(["bit_depth"], "8")),
    ("chroma_format nv12", _edit(["chroma_format"], "nv12")),
    ("no chroma_format", _edit(["chroma_format"], None)),
    ("width 0", _edit(["width"], 0)),
    ("height 16385", _edit(["height"], 16385)),
    ("denoise of one value", _edit(["denoise"], [8])),
    ("denoise 65", _edit(["denoise"], [65, 8])),
    ("no records", _edit(["records"], None)),
    ("empty records", _edit(["records"], [])),
    ("records as an object", _edit(["records"], {})),
    ("a record that is a number", _edit(["records", 0], 5)),
    ("the first record starts at 1", _edit(["records", 0, "first"], 1)),
    ("a gap between records", _edit(["records", 1, "first"], 3)),
    ("pictures 0", _edit(["records", 0, "pictures"], 0)),
    ("seed 2^32", _edit(["records", 0, "seed"], 1 << 32)),
    ("size 38", _edit(["records", 0, "size"], 38)),
    ("no size", _edit(["records", 0, "size"], None)),
    ("y of eight", _edit(["records", 0, "y"], [16] * 8)),
    ("u holds 256", _edit(["records", 0, "u"], [8] * 8 + [256])),
    ("v holds a string", _edit(["records", 0, "v"], [8] * 8 + ["8"])),
    ("no v", _edit(["records", 1, "v"], None)),
    ("words of two planes", _edit(["records", 0, "words"], [[0] * 16] * 2)),
    ("words of 15", _edit(["records", 0, "words"], [[0] * 16, [0] * 15, [0] * 16])),
    ("a word of 2^63", _edit(["records", 0, "words"], [[0] * 15 + [1 << 63]] * 3)),
]


@pytest.mark.parametrize("why,doc", MALFORMED, ids=[m[0].replace(" ", "_") for m in MALFORMED])
def test_a_malformed_file_is_refused(tmp_path, why, doc):
    path = str(tmp_path / "none.json") if doc is None else _file(tmp_path, doc)
    r = _decode(tmp_path, ["--film-grain", path])
    _refused(r, tmp_path, "cannot open" if doc is None else "is no grain file")


def test_the_message_names_the_key(tmp_path):
    for path, value, words in ((["records", 0, "size"], 38, '"size" must be an integer in 0..37'), (["version"], 2, "version 2"),
                               (["records", 1, "first"], 3, "record 1 must start at picture 2"), (["records", 0, "y"], [1], '"y" must be a list of 9')):
        r = _decode(tmp_path, ["--film-grain", _file(tmp_path, _edit(path, value))])
        _refused(r, tmp_path, words)
