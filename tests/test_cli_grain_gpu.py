"""dcvc decode --film-grain / --grain-strength and dcvc encode --denoise --grain-log on a real MI355X, against the
numpy restatement (tests/grain_np.py) around the tool's own plain paths: what a grained decode writes is the restatement applied
to what the plain decode writes, byte for byte - all-intra, LD, HT-S with a ragged chunk, 8 and 10 bits, yuv422, Y4M output,
behind --out-size, to stdout - its JSON log is the plain run's, its --hash-log holds the CRCs of the grained bytes, and
--grain-strength 0 writes the plain file; the records of --grain-log are the restatement's (denoise_np, then the measurement,
then the fit) for one window and for windows of two pictures, the stream is the --denoise run's, and the log decodes. Seeded
synthetic weights; the clip is 352x288, five pictures of the synthetic sequence plus seeded noise of sigma 3."""
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import denoise_np
import grain_np as gnp
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, picture_hash as ph, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 288, 352, 5
h, w = 144, 176
SIZE = ["-W", str(W), "-H", str(H)]
QP = ["--qp-i", "30", "--qp-p", "36"]


def _run(args, check=True):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    r = subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, timeout=600)
    assert not check or r.returncode == 0, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("grain_models")
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "ld.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "hts.dcvw"), "hts", dmc_ht_model("hts", skip_thres=0.15), 0.15)
    intra = ["--intra", str(d / "i.dcvw")]
    return {"intra": intra, "ld": intra + ["--inter", str(d / "ld.dcvw")], "hts": intra + ["--inter", str(d / "hts.dcvw")]}


_clips = {}


def _clip(bits, fmt="420"):
    """N noisy pictures (y, u, v); made once per (depth, chroma format)"""
    if (bits, fmt) not in _clips:
        rng = np.random.default_rng(29 + bits)
        s = 1 << (bits - 8)
        dtype = np.uint8 if bits == 8 else np.uint16
        pics = []
        for i in range(N):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=9)
            if fmt == "422":
                uv = np.repeat(uv, 2, axis=1)
            pics.append(tuple(np.clip(np.rint(p.astype(np.float64) * s + rng.normal(0, 3 * s, p.shape)), 0, (1 << bits) - 1).astype(dtype)
                              for p in (y, uv[0], uv[1])))
        _clips[(bits, fmt)] = pics
    return _clips[(bits, fmt)]


def _bytes(pics):
    return b"".join(p.astype("<u2" if p.dtype == np.uint16 else np.uint8).tobytes() for pic in pics for p in pic)


def _pictures(data, H_, W_, bits, fmt="420"):
    """a raw file -> pictures (y, u, v)"""
    dt = np.dtype("<u2") if bits > 8 else np.dtype(np.uint8)
    hc, wc = (H_, W_ // 2) if fmt == "422" else (H_ // 2, W_ // 2)
    a = np.frombuffer(data, dt)
    per = H_ * W_ + 2 * hc * wc
    assert a.size % per == 0
    out = []
    for i in range(a.size // per):
        p = a[i * per:(i + 1) * per]
        out.append((p[:H_ * W_].reshape(H_, W_), p[H_ * W_:H_ * W_ + hc * wc].reshape(hc, wc), p[H_ * W_ + hc * wc:].reshape(hc, wc)))
    return out


def _flags(bits, fmt):
    return (["--bit-depth", str(bits)] if bits > 8 else []) + (["--src-type", "yuv422"] if fmt == "422" else [])


_tpl = {}


def _template(seed, p, size):
    if (seed, p, size) not in _tpl:
        _tpl[(seed, p, size)] = gnp.template(seed, p, size)
    return _tpl[(seed, p, size)]


def _grained(pics, doc, bits):
    """the restatement of the decoder's stage: every picture through the record that holds its index (the last one past the end)"""
    out = []
    for i, (y, u, v) in enumerate(pics):
        r = [rec for rec in doc["records"] if rec["first"] <= i][-1]
        sx, sy = int(u.shape[1] != y.shape[1]), int(u.shape[0] != y.shape[0])
        t = [_template(r["seed"], p, r["size"]) for p in range(3)]
        out.append((gnp.apply_plane(y, y, t[0], r["y"], r["seed"], i, 0, bits, 0, 0),
                    gnp.apply_plane(u, y, t[1], r["u"], r["seed"], i, 1, bits, sx, sy),
                    gnp.apply_plane(v, y, t[2], r["v"], r["seed"], i, 2, bits, sx, sy)))
    return out


def _doc(bits, fmt="420", width=W, height=H):
    """a grain file of two records that ends before the clip does: tables that rise and fall with the luma, chroma tables of their own"""
    return {"version": 1, "bit_depth": bits, "chroma_format": "yuv" + fmt, "width": width, "height": height, "denoise": [8, 8],
            "records": [{"first": 0, "pictures": 1, "seed": 7, "size": 12, "y": [8, 16, 24, 32, 40, 48, 56, 64, 72], "u": [20] * 9,
                         "v": [0, 10, 20, 30, 40, 30, 20, 10, 0], "words": [[0] * 16] * 3},
                        {"first": 1, "pictures": 2, "seed": 4000000000, "size": 30, "y": [90, 60, 30, 20, 10, 20, 30, 60, 255], "u": [0] * 9,
                         "v": [33] * 9, "words": [[5] * 16] * 3}]}


def _manifest_of(data, src_type, depth, w_, h_):
    lens = ph.plane_bytes(src_type, depth, w_, h_)
    fb = sum(lens)
    pictures = []
    for at in range(0, len(data), fb):
        pic, planes, o = data[at:at + fb], [], 0
        for n in lens:
            planes.append(zlib.crc32(pic[o:o + n]))
            o += n
        pictures.append((zlib.crc32(pic), planes))
    return ph.format_manifest(ph.Manifest(src_type, depth, w_, h_, pictures, zlib.crc32(data), len(data)))


def _log(path):
    log = json.loads(path.read_text())
    log.pop("test_time")
    return log


CASES = [("intra", 8, "420"), ("ld", 10, "420"), ("hts", 8, "420"), ("ld", 8, "422")]


@pytest.mark.parametrize("model,bits,fmt", CASES, ids=["%s-%d-%s" % c for c in CASES])
def test_a_grained_decode_writes_the_restatement_on_the_plain_decode(tmp_path, models, model, bits, fmt):
    # hts: 1 I picture, then a chunk of 4 pictures and 4 repeats of the last one, which --ref ends in front of
    (tmp_path / "in.yuv").write_bytes(_bytes(_clip(bits, fmt)))
    kind = _flags(bits, fmt)
    _run(["encode"] + models[model] + kind + QP + SIZE + ["-i", tmp_path / "in.yuv", "-o", tmp_path / "s.bin"])
    dec = ["decode"] + models[model] + kind + ["-i", tmp_path / "s.bin", "--ref", tmp_path / "in.yuv"]
    _run(dec + ["-o", tmp_path / "plain.yuv", "--json", tmp_path / "plain.json"])
    doc = _doc(bits, fmt)
    (tmp_path / "g.json").write_text(json.dumps(doc))
    _run(dec + ["--film-grain", tmp_path / "g.json", "-o", tmp_path / "g.yuv", "--json", tmp_path / "g.json.log", "--hash-log", tmp_path / "g.txt"])
    plain = (tmp_path / "plain.yuv").read_bytes()
    pics = _pictures(plain, H, W, bits, fmt)
    assert len(pics) == N
    want = _bytes(_grained(pics, doc, bits))
    got = (tmp_path / "g.yuv").read_bytes()
    assert got != plain and len(got) == len(plain)
    assert got == want
    assert _log(tmp_path / "g.json.log") == _log(tmp_path / "plain.json")             # the metrics read the ungrained pictures
    assert (tmp_path / "g.txt").read_text() == _manifest_of(want, "yuv" + fmt, bits, W, H)
    # the hashes alone, without -o, and checked against the manifest just written
    r = _run(dec + ["--film-grain", tmp_path / "g.json", "--verify-hash", tmp_path / "g.txt"])
    assert "verified %d pictures" % N in r.stdout.decode()


@pytest.fixture(scope="module")
def ld8(tmp_path_factory, models):
    """an 8-bit LD stream of the clip, the decoder's call for it and its plain output, shared by the two tests below"""
    d = tmp_path_factory.mktemp("grain_ld8")
    (d / "in.yuv").write_bytes(_bytes(_clip(8)))
    _run(["encode"] + models["ld"] + QP + SIZE + ["-i", d / "in.yuv", "-o", d / "s.bin"])
    dec = ["decode"] + models["ld"] + ["-i", d / "s.bin"]
    _run(dec + ["-o", d / "plain.yuv"])
    plain = (d / "plain.yuv").read_bytes()
    return dec, plain, _pictures(plain, H, W, 8)


def test_y4m_output_and_stdout(tmp_path, ld8):
    dec, plain, pics = ld8
    _run(dec + ["-o", tmp_path / "plain.y4m"])
    doc = _doc(8)
    (tmp_path / "g.json").write_text(json.dumps(doc))
    want = _grained(pics, doc, 8)
    # Y4M: the plain file's header, then FRAME and a grained picture each
    _run(dec + ["--film-grain", tmp_path / "g.json", "-o", tmp_path / "g.y4m"])
    y4m = (tmp_path / "plain.y4m").read_bytes()
    header = y4m[:y4m.index(b"\n") + 1]
    assert (tmp_path / "g.y4m").read_bytes() == header + b"".join(b"FRAME\n" + _bytes([p]) for p in want)
    # -o -: the pictures on stdout, the messages on stderr
    r = _run(dec + ["--film-grain", tmp_path / "g.json", "-o", "-"])
    assert r.stdout == _bytes(want) and b"decoded %d pictures" % N in r.stderr


def test_a_constant_strength_and_a_file_of_another_size(tmp_path, ld8):
    dec, plain, pics = ld8
    # --grain-strength: constant tables, seed 1; 0 writes the plain file
    _run(dec + ["--grain-strength", "0", "-o", tmp_path / "zero.yuv"])
    assert (tmp_path / "zero.yuv").read_bytes() == plain
    _run(dec + ["--grain-strength", "24:9:20", "-o", tmp_path / "c.yuv"])
    const = {"records": [{"first": 0, "pictures": 1, "seed": 1, "size": 20, "y": [24] * 9, "u": [9] * 9, "v": [9] * 9}]}
    assert (tmp_path / "c.yuv").read_bytes() == _bytes(_grained(pics, const, 8))
    _run(dec + ["--grain-strength", "24", "-o", tmp_path / "d.yuv"])
    const = {"records": [{"first": 0, "pictures": 1, "seed": 1, "size": 12, "y": [24] * 9, "u": [24] * 9, "v": [24] * 9}]}
    assert (tmp_path / "d.yuv").read_bytes() == _bytes(_grained(pics, const, 8))
    # a file of another size is refused once the stream's size is known
    (tmp_path / "other.json").write_text(json.dumps(_doc(8, width=W, height=H + 2)))
    r = _run(dec + ["--film-grain", tmp_path / "other.json", "-o", tmp_path / "no.yuv"], check=False)
    assert r.returncode == 2 and b"the file describes 352x290 pictures, the stream holds 352x288" in r.stderr, r.stderr


@pytest.mark.parametrize("bits", [8, 10])
def test_behind_out_size_the_resampled_picture_is_grained_and_the_ungrained_one_measured(tmp_path, models, bits):
    (tmp_path / "in.yuv").write_bytes(_bytes(_clip(bits)))
    kind = _flags(bits, "420")
    _run(["encode"] + models["ld"] + kind + QP + SIZE + ["-i", tmp_path / "in.yuv", "--scale", "%dx%d" % (w, h), "-o", tmp_path / "s.bin"])
    dec = ["decode"] + models["ld"] + kind + ["-i", tmp_path / "s.bin", "--out-size", "%dx%d" % (W, H), "--ref", tmp_path / "in.yuv"]
    _run(dec + ["-o", tmp_path / "plain.yuv", "--json", tmp_path / "plain.json"])
    doc = _doc(bits, width=w, height=h)              # the coded size: with --out-size the file's size is not compared
    (tmp_path / "g.json").write_text(json.dumps(doc))
    _run(dec + ["--film-grain", tmp_path / "g.json", "-o", tmp_path / "g.yuv", "--json", tmp_path / "g.log", "--hash-log", tmp_path / "g.txt"])
    plain = (tmp_path / "plain.yuv").read_bytes()
    want = _bytes(_grained(_pictures(plain, H, W, bits), doc, bits))
    assert (tmp_path / "g.yuv").read_bytes() == want and want != plain
    assert _log(tmp_path / "g.log") == _log(tmp_path / "plain.json")
    assert (tmp_path / "g.txt").read_text() == _manifest_of(want, "yuv420", bits, W, H)


_filtered = {}


def _records(pics, bits, window, size=12, gain=100, flat=4, seed=1):
    """the restatement of --grain-log: the clip through denoise_np at 8:8, every picture measured, a record a window"""
    if (bits, len(pics)) not in _filtered:
        _filtered[(bits, len(pics))] = denoise_np.denoise_clip(pics, 8, 8, bits)
    filtered = _filtered[(bits, len(pics))]
    words = []
    for (sy_, su, sv), (dy, du, dv) in zip(pics, filtered):
        words.append([gnp.stats_plane(sy_, dy, dy, bits, 0, 0, flat), gnp.stats_plane(su, du, dy, bits, 1, 1, flat),
                      gnp.stats_plane(sv, dv, dy, bits, 1, 1, flat)])
    records, first = [], 0
    while first < len(pics):
        n = len(pics) - first if window == 0 else min(window, len(pics) - first)
        total = [[sum(wd[p][k] for wd in words[first:first + n]) for k in range(16)] for p in range(3)]
        lut = gnp.fit(total, bits, gain, 256)
        records.append({"first": first, "pictures": n, "seed": seed + len(records), "size": size, "y": lut[0], "u": lut[1], "v": lut[2],
                        "words": total})
        first += n
    return records


@pytest.mark.parametrize("model,bits,window", [("ld", 8, 0), ("ld", 10, 2), ("hts", 8, 2)], ids=["ld-8-whole", "ld-10-by2", "hts-8-by2"])
def test_grain_log_holds_the_restatements_records_and_changes_no_stream(tmp_path, models, model, bits, window):
    pics = _clip(bits)
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    kind = _flags(bits, "420")
    enc = ["encode"] + models[model] + kind + QP + SIZE + ["-i", tmp_path / "in.yuv", "--denoise", "8"]
    _run(enc + ["-o", tmp_path / "dn.bin"])
    extra = ["--grain-window", window] if window else []
    r = _run(enc + ["--grain-log", tmp_path / "g.json", "-o", tmp_path / "gl.bin"] + extra)
    assert (tmp_path / "gl.bin").read_bytes() == (tmp_path / "dn.bin").read_bytes()        # the stream does not change
    records = _records(pics, bits, window)
    assert len(records) == (1 if window == 0 else 3)
    assert b"grain: %d record" % len(records) in r.stdout and b"over %d pictures" % N in r.stdout      # padding pictures are not measured
    doc = json.loads((tmp_path / "g.json").read_text())
    assert doc == {"version": 1, "bit_depth": bits, "chroma_format": "yuv420", "width": W, "height": H, "denoise": [8, 8], "records": records}
    assert any(v > 0 for rec in records for v in rec["y"])                                  # noise of sigma 3 was found
    # the round trip: the log is a grain file
    dec = ["decode"] + models[model] + kind + ["-i", tmp_path / "gl.bin", "-n", N]
    _run(dec + ["-o", tmp_path / "plain.yuv"])
    _run(dec + ["--film-grain", tmp_path / "g.json", "-o", tmp_path / "g.yuv"])
    plain = (tmp_path / "plain.yuv").read_bytes()
    assert (tmp_path / "g.yuv").read_bytes() == _bytes(_grained(_pictures(plain, H, W, bits), doc, bits)) != plain


def test_the_options_reach_the_records(tmp_path, models):
    pics = _clip(8)[:2]
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    _run(["encode"] + models["intra"] + QP + SIZE + ["-i", tmp_path / "in.yuv", "--denoise", "8", "--grain-log", tmp_path / "g.json", "--grain-size",
                                                     "30", "--grain-gain", "150", "--grain-flat", "9", "--grain-seed", "4294967295", "--grain-window",
                                                     "1", "-o", tmp_path / "s.bin"])
    doc = json.loads((tmp_path / "g.json").read_text())
    want = _records(pics, 8, 1, size=30, gain=150, flat=9, seed=4294967295)
    want[1]["seed"] = 0                              # the seed is a u32: it wraps
    assert doc["records"] == want
