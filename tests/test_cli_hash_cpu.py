"""The dcvc tool's refusals for --hash-log / --verify-hash that the flags (and the manifest file) alone decide (DESIGN.md
19): each happens before a model is loaded or the device is touched - the weight files named here do not exist, and no GPU is
needed - with status 2, and no output file is created."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
GOOD = "# dcvc-hash 1 crc32 yuv420 8 64 48\n0 00000000 00000000 00000000 00000000\nsequence 00000000 4608\n"


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.yuv"), "-o", str(tmp_path / "o.bin"),
                 "-W", "64", "-H", "48"] + extra)


def _decode(tmp_path, extra):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin")] + extra)


def test_encode_hash_log_with_an_inter_model_is_refused(tmp_path):
    log = tmp_path / "h.txt"
    r = _encode(tmp_path, ["--inter", str(tmp_path / "missing_p.dcvw"), "--hash-log", str(log)])
    assert r.returncode == 2 and "--hash-log on encode is for all-intra runs" in r.stderr, r.stderr
    assert "the inter encoders reconstruct no pictures" in r.stderr
    r = _encode(tmp_path, ["--inter", str(tmp_path / "missing_p.dcvw"), "--intra-period", "8", "--hash-log", str(log)])
    assert r.returncode == 2 and "--hash-log on encode is for all-intra runs" in r.stderr, r.stderr
    # all-intra runs pass the flag checks: the model is next
    for extra in ([], ["--inter", str(tmp_path / "missing_p.dcvw"), "--intra-period", "1"], ["--batch", "3"]):
        r = _encode(tmp_path, extra + ["--hash-log", str(log)])
        assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not log.exists() and not (tmp_path / "o.bin").exists()


def test_verify_hash_on_encode_is_refused(tmp_path):
    (tmp_path / "h.txt").write_text(GOOD)
    r = _encode(tmp_path, ["--verify-hash", str(tmp_path / "h.txt")])
    assert r.returncode == 2 and "--verify-hash is a decoder flag" in r.stderr, r.stderr
    assert not (tmp_path / "o.bin").exists()


def test_verify_hash_on_a_missing_file_is_refused(tmp_path):
    r = _decode(tmp_path, ["--verify-hash", str(tmp_path / "nothing.txt")])
    assert r.returncode == 2 and "--verify-hash: cannot open" in r.stderr and "nothing.txt" in r.stderr, r.stderr


def test_a_well_formed_manifest_passes_the_flag_checks(tmp_path):
    (tmp_path / "h.txt").write_text(GOOD)
    r = _decode(tmp_path, ["--verify-hash", str(tmp_path / "h.txt"), "--hash-log", str(tmp_path / "out.txt")])
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "out.txt").exists()


MALFORMED = [
    ("empty", "", "not terminated"),
    ("no newline at the end", GOOD[:-1], "not terminated"),
    ("no header", GOOD.split("\n", 1)[1], "header"),
    ("another magic", GOOD.replace("dcvc-hash", "dcvc-hush"), "header"),
    ("version 2", GOOD.replace("dcvc-hash 1", "dcvc-hash 2"), "version 2"),
    ("another algorithm", GOOD.replace("crc32", "md5"), "algorithm md5"),
    ("unknown source type", GOOD.replace("yuv420", "yuv411"), "unknown source type yuv411"),
    ("a size that is no number", GOOD.replace(" 64 48", " 64 4x"), "bad numbers"),
    ("upper-case hex", GOOD.replace("0 00000000 00000000", "0 00000000 0000000A"), "8 lowercase hex digits"),
    ("seven hex digits", GOOD.replace("0 00000000 ", "0 0000000 "), "picture 0"),
    ("a plane missing", GOOD.replace("0 00000000 00000000 ", "0 00000000 "), "picture 0"),
    ("a picture index out of order", GOOD.replace("\n0 ", "\n1 "), "picture 0"),
    ("no sequence line", GOOD.rsplit("sequence", 1)[0], "no sequence line"),
    ("a byte count that is no number", GOOD.replace("4608", "46o8"), "sequence"),
    ("binary", "\x00\x01\x02\n", "header"),
]


@pytest.mark.parametrize("why,text,says", MALFORMED, ids=[m[0].replace(" ", "_") for m in MALFORMED])
def test_verify_hash_on_a_malformed_file_is_refused(tmp_path, why, text, says):
    (tmp_path / "h.txt").write_bytes(text.encode("latin-1"))
    r = _decode(tmp_path, ["--verify-hash", str(tmp_path / "h.txt")])
    assert r.returncode == 2 and "is no hash manifest" in r.stderr and says in r.stderr, r.stderr
    assert "missing.dcvw" not in r.stderr              # refused before a model is loaded
