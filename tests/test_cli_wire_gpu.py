"""dcvc encode / decode with the wire formats (--src-type nv21 | nv16 | p210 | uyvy | yuy2 | y210 | v210) on a real
MI355X against the SAME clip in the carrier's layout coded with the carrier's type: a wire picture is unpacked into the buffer
where the carrier type's upload lands and packed behind dcvc_x_to_pix, so the stream, the log and the quality search are the
carrier run's byte for byte, -o is tests/wire_np.py's pack of the carrier run's -o, and the hashes cover the packed bytes.
352x288, 3 pictures, seeded synthetic weights and pictures as test_cli_pixfmt_gpu.py builds them."""
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import wire_np as wn
from codec_util import dmc_ld_model, dmci_model
from dcvc_amd import export_weights, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 288, 352, 3
SIZE = ["-W", str(W), "-H", str(H)]
# --src-type: (wire, depth, the carrier's --src-type flags, flags of the wire type itself)
TYPES = {
    "uyvy": (wn.UYVY, 8, ["--src-type", "yuv422"], []),
    "v210": (wn.V210, 10, ["--src-type", "yuv422", "--bit-depth", "10"], []),
    "nv21": (wn.NV21, 8, ["--src-type", "nv12"], []),
    "yuy2": (wn.YUY2, 8, ["--src-type", "yuv422"], []),
    "y210": (wn.YUY2, 10, ["--src-type", "yuv422", "--bit-depth", "10"], []),
    "nv16": (wn.NV16, 8, ["--src-type", "yuv422"], []),
    "p210": (wn.NV16, 10, ["--src-type", "yuv422", "--bit-depth", "10"], []),
    "yuy2-16": (wn.YUY2, 16, ["--src-type", "yuv422", "--bit-depth", "16"], ["--bit-depth", "16"]),
}


def _run(args, check=True):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, check=check, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("wire_models")
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "p.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    return ["--intra", str(d / "i.dcvw")], ["--inter", str(d / "p.dcvw")]


_clips = {}


def _carrier_clip(wire, bits):
    """N flat carrier pictures: the synthetic 8-bit 4:2:0 sequence with its chroma rows repeated for 4:2:2, plus noise, scaled
    to `bits` with low-order noise; computed once per (carrier, depth)"""
    key = (wn.carrier(wire), bits)
    if key not in _clips:
        rng = np.random.default_rng(17 + bits)
        s = 1 << (bits - 8)
        pics = []
        for i in range(N):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=5)
            if wire != wn.NV21:
                uv = np.repeat(uv, 2, axis=1)
            uv = np.clip(uv.astype(np.int32) + rng.integers(-3, 4, uv.shape), 0, 255)
            y, uv = ((p.astype(np.uint32) * s + rng.integers(0, s, p.shape)).astype(wn.dtype(bits)) for p in (y, uv))
            c = np.stack([uv[0], uv[1]], axis=-1) if wire == wn.NV21 else uv                 # NV12: interleaved pairs
            pics.append(np.concatenate([y.ravel(), c.ravel()]))
        _clips[key] = pics
    return _clips[key]


def _write_clips(tmp_path, name):
    """the clip in the carrier's layout and in the wire layout -> (carrier flags, wire flags)"""
    wire, bits, carrier_flags, extra = TYPES[name]
    pics = _carrier_clip(wire, bits)
    le = "<u2" if bits > 8 else np.uint8
    (tmp_path / "carrier.yuv").write_bytes(b"".join(p.astype(le).tobytes() for p in pics))
    (tmp_path / "wire.yuv").write_bytes(b"".join(wn.pack(p, wire, bits, H, W).tobytes() for p in pics))
    return carrier_flags, ["--src-type", name.split("-")[0]] + extra


def _numbers(path):
    log = json.loads(path.read_text())
    log.pop("test_time")
    return log


@pytest.mark.parametrize("name", ["uyvy", "v210", "nv21"])
def test_round_trip_equals_the_carrier_types(tmp_path, models, name):
    wire, bits = TYPES[name][:2]
    carrier_flags, wire_flags = _write_clips(tmp_path, name)
    args = models[0] + models[1]
    p = lambda f: str(tmp_path / f)
    for kind, flags in (("carrier", carrier_flags), ("wire", wire_flags)):
        _run(["encode"] + args + flags + ["--qp-i", "30", "--qp-p", "36", "-i", p(kind + ".yuv")] + SIZE + ["-o", p(kind + ".bin")])
        _run(["decode"] + args + flags + ["-i", p(kind + ".bin"), "-o", p(kind + ".rec"), "--ref", p(kind + ".yuv"), "--json", p(kind + ".json"),
                                          "--calc-ssim", "1", "--verbose-json", "1", "--hash-log", p(kind + ".hash")])
    assert (tmp_path / "wire.bin").read_bytes() == (tmp_path / "carrier.bin").read_bytes(), "the streams differ"
    rec = np.frombuffer((tmp_path / "carrier.rec").read_bytes(), "<u2" if bits > 8 else np.uint8).reshape(N, -1)
    want = b"".join(wn.pack(r, wire, bits, H, W).tobytes() for r in rec)
    got = (tmp_path / "wire.rec").read_bytes()
    assert len(got) == N * wn.picture_bytes(wire, bits, H, W) and got == want, "-o is not the packed carrier picture"
    log = _numbers(tmp_path / "wire.json")
    assert log == _numbers(tmp_path / "carrier.json") and len(log["frame_msssim"]) == N and log["p_frame_num"] == N - 1
    # the manifest: the type's own name, one segment for the packed formats and two for nv21, the sequence CRC of the -o file
    lines = (tmp_path / "wire.hash").read_text().splitlines()
    assert lines[0] == "# dcvc-hash 1 crc32 %s %d %d %d" % (name, bits, W, H)
    assert lines[-1] == "sequence %08x %d" % (zlib.crc32(got), len(got))
    fb = len(got) // N
    for i, line in enumerate(lines[1:-1]):
        pic = got[i * fb:(i + 1) * fb]
        segs = [pic[:H * W], pic[H * W:]] if name == "nv21" else [pic]
        assert line.split() == [str(i), "%08x" % zlib.crc32(pic)] + ["%08x" % zlib.crc32(s) for s in segs]
    r = _run(["decode"] + args + wire_flags + ["-i", p("wire.bin"), "--verify-hash", p("wire.hash")])
    assert "verified %d pictures" % N in r.stdout
    # one byte of the first picture's CRC changed: status 3
    text = (tmp_path / "wire.hash").read_text()
    at = text.index("\n0 ") + 3
    (tmp_path / "bad.hash").write_text(text[:at] + ("0" if text[at] != "0" else "1") + text[at + 1:])
    r = _run(["decode"] + args + wire_flags + ["-i", p("wire.bin"), "--verify-hash", p("bad.hash")], check=False)
    assert r.returncode == 3 and "picture 0" in r.stderr, r.stderr
    # a manifest of the carrier type is another type's: refused before a picture is decoded
    r = _run(["decode"] + args + wire_flags + ["-i", p("wire.bin"), "--verify-hash", p("carrier.hash")], check=False)
    assert r.returncode == 2 and "--verify-hash" in r.stderr, r.stderr


@pytest.mark.parametrize("name", ["yuy2", "y210", "nv16", "p210", "yuy2-16"])
def test_all_intra_streams_equal_the_carrier_types(tmp_path, models, name):
    carrier_flags, wire_flags = _write_clips(tmp_path, name)
    for kind, flags in (("carrier", carrier_flags), ("wire", wire_flags)):
        _run(["encode"] + models[0] + flags + ["--qp-i", "30", "-n", "1", "-i", str(tmp_path / (kind + ".yuv"))] + SIZE +
             ["-o", str(tmp_path / (kind + ".bin"))])
    assert (tmp_path / "wire.bin").read_bytes() == (tmp_path / "carrier.bin").read_bytes()


def test_encode_hash_log_equals_decode_hash_log(tmp_path, models):
    _, wire_flags = _write_clips(tmp_path, "v210")
    p = lambda f: str(tmp_path / f)
    _run(["encode"] + models[0] + wire_flags + ["--qp-i", "30", "-n", "2", "-i", p("wire.yuv")] + SIZE + ["-o", p("w.bin"), "--hash-log", p("enc.hash")])
    _run(["decode"] + models[0] + wire_flags + ["-i", p("w.bin"), "--hash-log", p("dec.hash")])
    assert (tmp_path / "enc.hash").read_bytes() == (tmp_path / "dec.hash").read_bytes()
    assert (tmp_path / "enc.hash").read_text().startswith("# dcvc-hash 1 crc32 v210 10 %d %d\n0 " % (W, H))


def test_target_psnr_equals_the_yuv422_run(tmp_path, models):
    carrier_flags, wire_flags = _write_clips(tmp_path, "uyvy")
    args = models[0] + models[1]
    for kind, flags in (("carrier", carrier_flags), ("wire", wire_flags)):
        _run(["encode"] + args + flags + ["--qp-i", "32", "--target-psnr", "30", "-i", str(tmp_path / (kind + ".yuv"))] + SIZE +
             ["-o", str(tmp_path / (kind + ".bin")), "--quality-log", str(tmp_path / (kind + ".q.json"))])
    wire_log, carrier_log = (json.loads((tmp_path / (k + ".q.json")).read_text()) for k in ("wire", "carrier"))
    assert [u["qp"] for u in wire_log["units"]] == [u["qp"] for u in carrier_log["units"]] and len(wire_log["units"]) == N
    assert wire_log == carrier_log
    assert (tmp_path / "wire.bin").read_bytes() == (tmp_path / "carrier.bin").read_bytes()


def test_a_file_that_ends_inside_a_picture(tmp_path, models):
    """as the raw YUV types: the pictures that are whole are coded"""
    _, wire_flags = _write_clips(tmp_path, "v210")
    data = (tmp_path / "wire.yuv").read_bytes()
    fb = wn.picture_bytes(wn.V210, 10, H, W)
    (tmp_path / "short.yuv").write_bytes(data[:2 * fb - 1])
    r = _run(["encode"] + models[0] + wire_flags + ["--qp-i", "30", "-i", str(tmp_path / "short.yuv")] + SIZE + ["-o", str(tmp_path / "s.bin")])
    assert "encoded 1 pictures" in r.stdout, r.stdout
