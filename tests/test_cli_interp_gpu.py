"""dcvc decode --interpolate / --interp-log / --interp-ref and dcvc encode --frame-step on a real MI355X, against the
numpy restatement (tests/interp_np.py) around the tool's own plain paths: what an interpolating decode writes is the restatement
applied to what the plain decode writes - N = 2 and 3, all-intra, LD, HT-S with a ragged chunk, 10-bit yuv422, behind --out-size,
as Y4M at N times the rate, to stdout, with --pad (the bars untouched) and with grain (at output-order indexes); --hash-log holds
the CRCs of the written pictures, --json is the plain run's, --interp-log holds the restatement's counts and, with --interp-ref,
numpy's PSNRs; a stream of one picture writes one picture; --frame-step 2 writes the stream of the pre-decimated clip. Seeded
synthetic weights; the clip is 352x288, pictures of the synthetic sequence (a pan of 4 samples along x and 2 along y a picture)."""
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import grain_np as gnp
import interp_np
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, picture_hash as ph, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 288, 352, 3
SIZE = ["-W", str(W), "-H", str(H)]
QP = ["--qp-i", "30", "--qp-p", "36"]


def _run(args, check=True, data=None):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    r = subprocess.run([TOOL] + [str(a) for a in args], input=data, capture_output=True, timeout=600)
    assert not check or r.returncode == 0, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("interp_models")
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "ld.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "hts.dcvw"), "hts", dmc_ht_model("hts", skip_thres=0.15), 0.15)
    intra = ["--intra", str(d / "i.dcvw")]
    return {"intra": intra, "ld": intra + ["--inter", str(d / "ld.dcvw")], "hts": intra + ["--inter", str(d / "hts.dcvw")]}


_clips = {}


def _clip(bits, fmt="420", n=N):
    if (bits, fmt, n) not in _clips:
        s = 1 << (bits - 8)
        dtype = np.uint8 if bits == 8 else np.uint16
        pics = []
        for i in range(n):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=9)      # index i: a pan of (4 i, 2 i)
            if fmt == "422":
                uv = np.repeat(uv, 2, axis=1)
            pics.append(tuple((p.astype(np.int64) * s).astype(dtype) for p in (y, uv[0], uv[1])))
        _clips[(bits, fmt, n)] = pics
    return _clips[(bits, fmt, n)]


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


def _sub(fmt):
    return (1, 0) if fmt == "422" else (1, 1)


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


CASES = [("intra", 8, "420", 2), ("intra", 8, "420", 3), ("ld", 8, "420", 2), ("hts", 8, "420", 3), ("ld", 10, "422", 2)]


@pytest.mark.parametrize("model,bits,fmt,n", CASES, ids=["%s-%d-%s-x%d" % c for c in CASES])
def test_an_interpolating_decode_writes_the_restatement_on_the_plain_decode(tmp_path, models, model, bits, fmt, n):
    # hts: 1 I picture, then a chunk of 2 pictures and 6 repeats of the last one, which --ref ends in front of
    (tmp_path / "in.yuv").write_bytes(_bytes(_clip(bits, fmt)))
    kind = _flags(bits, fmt)
    _run(["encode"] + models[model] + kind + QP + SIZE + ["-i", tmp_path / "in.yuv", "-o", tmp_path / "s.bin"])
    dec = ["decode"] + models[model] + kind + ["-i", tmp_path / "s.bin", "--ref", tmp_path / "in.yuv"]
    _run(dec + ["-o", tmp_path / "plain.yuv", "--json", tmp_path / "plain.json"])
    r = _run(dec + ["--interpolate", n, "-o", tmp_path / "ip.yuv", "--json", tmp_path / "ip.json.log", "--hash-log", tmp_path / "ip.txt",
                    "--interp-log", tmp_path / "ip.json"])
    plain = (tmp_path / "plain.yuv").read_bytes()
    pics = _pictures(plain, H, W, bits, fmt)
    assert len(pics) == N
    sx, sy = _sub(fmt)
    want_pics, want_log = interp_np.interpolate_clip(pics, bits, n, sx=sx, sy=sy)
    assert len(want_pics) == n * (N - 1) + 1
    want = _bytes(want_pics)
    got = (tmp_path / "ip.yuv").read_bytes()
    assert len(got) == len(want)
    assert got == want
    assert _log(tmp_path / "ip.json.log") == _log(tmp_path / "plain.json")            # the metrics are those of the decoded pictures
    assert (tmp_path / "ip.txt").read_text() == _manifest_of(want, "yuv" + fmt, bits, W, H)
    log = json.loads((tmp_path / "ip.json").read_text())
    assert (log["n"], log["range"], log["lambda"], log["limit"], log["block"], log["width"], log["height"]) == (n, 7, 4, 8, 16, W, H)
    print(model, bits, fmt, n, want_log)
    assert log["pictures"] == want_log
    rep = sum(e["repeated"] for e in want_log)
    assert ("interpolate x%d (%d in-between pictures, %d repeated)" % (n, (n - 1) * (N - 1), rep)) in r.stdout.decode()


@pytest.fixture(scope="module")
def ld8(tmp_path_factory, models):
    """an 8-bit LD stream of the clip, the decoder's call for it, its plain output and the restatement's pictures at N = 2"""
    d = tmp_path_factory.mktemp("interp_ld8")
    (d / "in.yuv").write_bytes(_bytes(_clip(8)))
    _run(["encode"] + models["ld"] + QP + SIZE + ["-i", d / "in.yuv", "-o", d / "s.bin"])
    dec = ["decode"] + models["ld"] + ["-i", d / "s.bin"]
    _run(dec + ["-o", d / "plain.yuv"])
    pics = _pictures((d / "plain.yuv").read_bytes(), H, W, 8)
    return dec, pics, interp_np.interpolate_clip(pics, 8, 2)[0], d


def test_the_parameters_reach_the_kernels(tmp_path, ld8):
    dec, pics, _, _ = ld8
    _run(dec + ["--interpolate", "2:3:0:2", "-o", tmp_path / "a.yuv", "--interp-log", tmp_path / "a.json"])
    want, log = interp_np.interpolate_clip(pics, 8, 2, R=3, lam=0, limit=2)
    assert (tmp_path / "a.yuv").read_bytes() == _bytes(want)
    got = json.loads((tmp_path / "a.json").read_text())
    assert (got["range"], got["lambda"], got["limit"]) == (3, 0, 2) and got["pictures"] == log


def test_y4m_output_at_n_times_the_rate_and_stdout(tmp_path, ld8):
    dec, pics, want, _ = ld8
    _run(dec + ["-o", tmp_path / "plain.y4m", "--fps", "30000:1001"])
    _run(dec + ["--interpolate", 2, "-o", tmp_path / "ip.y4m", "--fps", "30000:1001"])
    y4m = (tmp_path / "plain.y4m").read_bytes()
    header = y4m[:y4m.index(b"\n") + 1]
    assert b" F30000:1001 " in header
    assert (tmp_path / "ip.y4m").read_bytes() == header.replace(b" F30000:1001 ", b" F60000:1001 ") + b"".join(b"FRAME\n" + _bytes([p]) for p in want)
    _run(dec + ["--interpolate", 3, "-o", tmp_path / "ip3.y4m"])                      # no --fps, no --ref: 25:1
    assert b" F75:1 " in (tmp_path / "ip3.y4m").read_bytes()[:80]
    # -o -: the pictures on stdout, the messages on stderr
    r = _run(dec + ["--interpolate", 2, "-o", "-"])
    assert r.stdout == _bytes(want) and b"interpolate x2" in r.stderr


def test_behind_out_size(tmp_path, ld8):
    dec, _, _, _ = ld8
    _run(dec + ["--out-size", "176x144", "-o", tmp_path / "small.yuv"])
    small = _pictures((tmp_path / "small.yuv").read_bytes(), 144, 176, 8)
    _run(dec + ["--out-size", "176x144", "--interpolate", 2, "-o", tmp_path / "ip.yuv", "--interp-log", tmp_path / "ip.json"])
    want, log = interp_np.interpolate_clip(small, 8, 2)
    assert (tmp_path / "ip.yuv").read_bytes() == _bytes(want)
    got = json.loads((tmp_path / "ip.json").read_text())
    assert (got["width"], got["height"]) == (176, 144) and got["pictures"] == log


def test_the_bars_of_pad_come_out_untouched(tmp_path, ld8):
    dec, _, want, _ = ld8
    pad = ["--pad", "%dx%d+16+8" % (W + 48, H + 24), "--pad-fill", "30:100:200"]
    _run(dec + pad + ["-o", tmp_path / "plain.yuv"])
    padded = _pictures((tmp_path / "plain.yuv").read_bytes(), H + 24, W + 48, 8)
    _run(dec + pad + ["--interpolate", 2, "-o", tmp_path / "ip.yuv"])
    got = _pictures((tmp_path / "ip.yuv").read_bytes(), H + 24, W + 48, 8)
    assert len(got) == len(want)
    for g, w_ in zip(got, want):
        for p, (gp, wp) in enumerate(zip(g, w_)):
            s = 1 if p == 0 else 2
            exp = padded[0][p].copy()
            exp[8 // s:8 // s + wp.shape[0], 16 // s:16 // s + wp.shape[1]] = wp
            assert np.array_equal(gp, exp)


def test_grain_takes_output_order_indexes(tmp_path, ld8):
    dec, _, want, _ = ld8
    _run(dec + ["--interpolate", 2, "--grain-strength", "24", "-o", tmp_path / "g.yuv", "--hash-log", tmp_path / "g.txt"])
    t = [gnp.template(1, p, 12) for p in range(3)]
    grained = [(gnp.apply_plane(y, y, t[0], [24] * 9, 1, i, 0, 8, 0, 0), gnp.apply_plane(u, y, t[1], [24] * 9, 1, i, 1, 8, 1, 1),
                gnp.apply_plane(v, y, t[2], [24] * 9, 1, i, 2, 8, 1, 1)) for i, (y, u, v) in enumerate(want)]
    assert (tmp_path / "g.yuv").read_bytes() == _bytes(grained)
    assert (tmp_path / "g.txt").read_text() == _manifest_of(_bytes(grained), "yuv420", 8, W, H)


def _psnr(src, rec, peak):
    """metrics.py calc_psnr of integer samples: the sum of squares is an exact integer, so only log10 can differ"""
    se = int(((src.astype(np.int64) - rec.astype(np.int64)) ** 2).sum())
    mse = se / src.size
    p = 10 * np.log10(peak * peak / mse) if mse > 1e-10 else 999.9
    return float(min(p, 99.9))


@pytest.mark.parametrize("y4m", [False, True], ids=["raw", "y4m"])
def test_the_in_between_pictures_are_measured_against_a_clip_at_the_output_rate(tmp_path, ld8, y4m):
    dec, _, want, _ = ld8
    ref = _clip(8, n=2 * N - 1)                      # the synthetic sequence at twice the rate has no counterpart: any clip of that length does
    if y4m:
        (tmp_path / "ref.y4m").write_bytes(b"YUV4MPEG2 W%d H%d F50:1 Ip A1:1 C420jpeg\n" % (W, H) + b"".join(b"FRAME\n" + _bytes([p]) for p in ref))
    else:
        (tmp_path / "ref.yuv").write_bytes(_bytes(ref))
    name = tmp_path / ("ref.y4m" if y4m else "ref.yuv")
    _run(dec + ["--interpolate", 2, "--interp-log", tmp_path / "ip.json", "--interp-ref", name])
    got = json.loads((tmp_path / "ip.json").read_text())["pictures"]
    assert [e["out_idx"] for e in got] == [1, 3]
    for e in got:
        for p, key in enumerate(("psnr_y", "psnr_u", "psnr_v")):
            assert e[key] == pytest.approx(_psnr(ref[e["out_idx"]][p], want[e["out_idx"]][p], 255.0), rel=1e-12, abs=0), (e, key)
    # a clip that ends before the output does is refused
    (tmp_path / "short.yuv").write_bytes(_bytes(ref[:2]))
    r = _run(dec + ["--interpolate", 2, "--interp-log", tmp_path / "no.json", "--interp-ref", tmp_path / "short.yuv"], check=False)
    assert r.returncode == 2 and b"is shorter than the output" in r.stderr


def test_a_stream_of_one_picture_writes_one_picture(tmp_path, models):
    (tmp_path / "in.yuv").write_bytes(_bytes(_clip(8)[:1]))
    _run(["encode"] + models["intra"] + QP + SIZE + ["-i", tmp_path / "in.yuv", "-o", tmp_path / "s.bin"])
    dec = ["decode"] + models["intra"] + ["-i", tmp_path / "s.bin"]
    _run(dec + ["-o", tmp_path / "plain.yuv"])
    r = _run(dec + ["--interpolate", 4, "-o", tmp_path / "ip.yuv", "--interp-log", tmp_path / "ip.json"])
    assert (tmp_path / "ip.yuv").read_bytes() == (tmp_path / "plain.yuv").read_bytes()
    assert json.loads((tmp_path / "ip.json").read_text())["pictures"] == []
    assert b"interpolate x4 (0 in-between pictures, 0 repeated)" in r.stdout


@pytest.mark.parametrize("inter", ["intra", "ld"])
def test_frame_step_writes_the_stream_of_the_decimated_clip(tmp_path, models, inter):
    clip = _clip(8, n=5)
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(clip[::2]))
    enc = ["encode"] + models[inter] + QP + SIZE
    _run(enc + ["-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    want = (tmp_path / "pre.bin").read_bytes()
    _run(enc + ["-i", tmp_path / "in.yuv", "--frame-step", 2, "-o", tmp_path / "a.bin"])
    assert len(want) > 100 and (tmp_path / "a.bin").read_bytes() == want
    # from stdin, where the dropped pictures are read too; and -n counts coded pictures
    _run(enc + ["-i", "-", "--frame-step", 2, "-o", tmp_path / "b.bin"], data=_bytes(clip))
    assert (tmp_path / "b.bin").read_bytes() == want
    _run(enc + ["-i", tmp_path / "pre.yuv", "-n", 2, "-o", tmp_path / "pre2.bin"])
    _run(enc + ["-i", tmp_path / "in.yuv", "--frame-step", 2, "-n", 2, "-o", tmp_path / "a2.bin"])
    assert (tmp_path / "a2.bin").read_bytes() == (tmp_path / "pre2.bin").read_bytes()
    # a step of 3 over 5 pictures keeps pictures 0 and 3; a Y4M source is decimated as a raw one
    (tmp_path / "pre3.yuv").write_bytes(_bytes(clip[::3]))
    (tmp_path / "in.y4m").write_bytes(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n" % (W, H) + b"".join(b"FRAME\n" + _bytes([p]) for p in clip))
    _run(enc + ["-i", tmp_path / "pre3.yuv", "-o", tmp_path / "pre3.bin"])
    _run(["encode"] + models[inter] + QP + ["-i", tmp_path / "in.y4m", "--frame-step", 3, "-o", tmp_path / "a3.bin"])
    assert (tmp_path / "a3.bin").read_bytes() == (tmp_path / "pre3.bin").read_bytes()
