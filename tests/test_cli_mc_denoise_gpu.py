"""dcvc encode --denoise S:T --denoise-mc R[:LAMBDA] / --mv-log on a real MI355X, against the numpy restatement
(tests/motion_np.py around tests/denoise_np.py) and the tool's own unfiltered paths: on a panning clip the stream of a
--denoise 8 --denoise-mc 7 run is the stream of a run without the flags on the clip pre-filtered in numpy - all-intra, LD, HT-S
with a ragged chunk, 10-bit yuv422, uyvy on its planar carrier, behind --scale, from stdin with --read-ahead 2 - --denoise-out
holds the numpy pictures, a static clip and --denoise 8:0 give the files of --denoise alone, --mv-log holds the numpy vectors'
sums and --grain-log still writes its records. Seeded synthetic weights; the clip is 352x288, three pictures of the synthetic
sequence (a pan of 4 samples along x and 2 along y a picture) plus seeded noise of sigma 3."""
import json
import os
import subprocess

import numpy as np
import pytest

import denoise_np
import grain_np as gnp
import motion_np
import resample_np
import wire_np as wn
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 288, 352, 3
h, w = 144, 176
SIZE = ["-W", str(W), "-H", str(H)]
QP = ["--qp-i", "30", "--qp-p", "36"]
R, LAM = 7, 4
MC = ["--denoise", "8", "--denoise-mc", str(R)]


def _run(args, check=True, data=None):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    r = subprocess.run([TOOL] + [str(a) for a in args], input=data, capture_output=True, timeout=600)
    assert not check or r.returncode == 0, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("mc_denoise_models")
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "ld.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "hts.dcvw"), "hts", dmc_ht_model("hts", skip_thres=0.15), 0.15)
    intra = ["--intra", str(d / "i.dcvw")]
    return {"intra": intra, "ld": intra + ["--inter", str(d / "ld.dcvw")], "hts": intra + ["--inter", str(d / "hts.dcvw")]}


_clips = {}


def _noisy(bits, fmt, static):
    rng = np.random.default_rng(57 + bits)
    s = 1 << (bits - 8)
    dtype = np.uint8 if bits == 8 else np.uint16
    pics = []
    for i in range(N):
        y, uv = synthetic.synthetic_frame_yuv420(H, W, index=0 if static else i, seed=9)      # index i: a pan of (4 i, 2 i)
        if fmt == "422":
            uv = np.repeat(uv, 2, axis=1)
        planes = []
        for p in (y, uv[0], uv[1]):
            v = p.astype(np.float64) * s + rng.normal(0, 3 * s, p.shape)
            planes.append(np.clip(np.rint(v), 0, (1 << bits) - 1).astype(dtype))
        pics.append(tuple(planes))
    return pics


def _sub(fmt):
    return (1, 0) if fmt == "422" else (1, 1)


def _clip(bits, fmt="420", static=False):
    """(the noisy clip, the clip filtered at 8:8 with compensation at range 7, lambda 4, the vectors): computed once"""
    key = (bits, fmt, static)
    if key not in _clips:
        pics = _noisy(bits, fmt, static)
        sx, sy = _sub(fmt)
        filtered, mvs = motion_np.mc_denoise_clip(pics, 8, 8, bits, R, LAM, sx, sy)
        if not static:
            plain = denoise_np.denoise_clip(pics, 8, 8, bits)
            assert not np.array_equal(filtered[N - 1][0], plain[N - 1][0])          # the compensation changes the clip
            assert all(tuple(np.median(m[0].reshape(-1, 2), axis=0)) == (4, 2) for m in mvs[1:])      # and finds the pan
        _clips[key] = (pics, filtered, mvs)
    return _clips[key]


def _bytes(pics):
    return b"".join(p.astype("<u2" if p.dtype == np.uint16 else np.uint8).tobytes() for pic in pics for p in pic)


def _depth(bits):
    return ["--bit-depth", str(bits)] if bits > 8 else []


def _summary(mvs):
    moved = sum(int(m[0].any(axis=-1).sum()) for m in mvs if m is not None)
    blocks = sum(m[0].shape[0] * m[0].shape[1] for m in mvs if m is not None)
    return "denoise: spatial 8, temporal 8, %d pictures filtered, mc range %d lambda %d (%d of %d blocks moved)" % (N, R, LAM, moved, blocks)


def _both(tmp_path, model, bits, extra=(), fmt="420"):
    """the --denoise 8 --denoise-mc 7 run on the noisy clip and the plain run on the pre-filtered one -> the two streams"""
    pics, filtered, mvs = _clip(bits, fmt)
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    kind = ["--src-type", "yuv422"] if fmt == "422" else []
    args = ["encode"] + model + _depth(bits) + kind + QP + SIZE
    r = _run(args + ["-i", tmp_path / "in.yuv", "-o", tmp_path / "mc.bin"] + MC + list(extra))
    assert _summary(mvs) in r.stdout.decode(), r.stdout
    _run(args + ["-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    return (tmp_path / "mc.bin").read_bytes(), (tmp_path / "pre.bin").read_bytes()


@pytest.mark.parametrize("inter", ["intra", "ld"])
def test_the_stream_is_that_of_the_prefiltered_clip(tmp_path, models, inter):
    got, want = _both(tmp_path, models[inter], 8, extra=["--denoise-out", tmp_path / "dn.yuv"])
    assert len(want) > 100 and got == want
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(_clip(8)[1])              # --denoise-out holds the numpy pictures


def test_a_ragged_hts_chunk(tmp_path, models):
    # 1 I picture, then a chunk of 2 pictures and 6 repeats of the last one: the repeats are neither searched nor filtered again
    got, want = _both(tmp_path, models["hts"], 8, extra=["--denoise-out", tmp_path / "dn.yuv"])
    assert len(want) > 100 and got == want
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(_clip(8)[1])


def test_10_bit_yuv422(tmp_path, models):
    got, want = _both(tmp_path, models["ld"], 10, extra=["--denoise-out", tmp_path / "dn.yuv"], fmt="422")
    assert len(want) > 100 and got == want
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(_clip(10, "422")[1])


def test_uyvy_is_filtered_on_its_planar_carrier(tmp_path, models):
    pics, filtered, _ = _clip(8, "422")
    carrier = [np.concatenate([p.ravel() for p in pic]) for pic in pics]
    (tmp_path / "wire.yuv").write_bytes(b"".join(wn.pack(c, wn.UYVY, 8, H, W).tobytes() for c in carrier))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + models["ld"] + QP + SIZE
    _run(args + ["-i", tmp_path / "wire.yuv", "--src-type", "uyvy", "--denoise-out", tmp_path / "dn.yuv", "-o", tmp_path / "mc.bin"] + MC)
    _run(args + ["-i", tmp_path / "pre.yuv", "--src-type", "yuv422", "-o", tmp_path / "pre.bin"])
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(filtered)
    assert (tmp_path / "mc.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_behind_scale_the_scaled_clip_is_searched_and_filtered(tmp_path, models):
    pics, _, _ = _clip(8)
    small = [(resample_np.resample_plane(y, h, w, 255), resample_np.resample_plane(u, h // 2, w // 2, 255),
              resample_np.resample_plane(v, h // 2, w // 2, 255)) for y, u, v in pics]
    filtered, mvs = motion_np.mc_denoise_clip(small, 8, 8, 8, R, LAM)
    assert mvs[1][0].shape == (9, 11, 2) and mvs[1][0].any()
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + models["ld"] + QP
    _run(args + SIZE + ["-i", tmp_path / "in.yuv", "--scale", "%dx%d" % (w, h), "--denoise-out", tmp_path / "dn.yuv", "-o",
                        tmp_path / "mc.bin"] + MC)
    _run(args + ["-W", w, "-H", h, "-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(filtered)
    assert (tmp_path / "mc.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_from_stdin_with_read_ahead(tmp_path, models):
    pics, filtered, _ = _clip(8)
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + models["ld"] + QP + SIZE
    _run(args + ["-i", "-", "--read-ahead", "2", "-o", tmp_path / "mc.bin"] + MC, data=_bytes(pics))
    _run(args + ["-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    assert (tmp_path / "mc.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_a_static_clip_gives_the_file_of_denoise_alone(tmp_path, models):
    pics, filtered, mvs = _clip(8, static=True)
    assert all(not m[0].any() for m in mvs[1:])
    assert all(np.array_equal(a, b) for f, p in zip(filtered, denoise_np.denoise_clip(pics, 8, 8, 8)) for a, b in zip(f, p))
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    args = ["encode"] + models["ld"] + QP + SIZE + ["-i", tmp_path / "in.yuv"]
    _run(args + ["--denoise", "8", "-o", tmp_path / "dn.bin"])
    r = _run(args + MC + ["-o", tmp_path / "mc.bin"])
    assert "(0 of %d blocks moved)" % (2 * 18 * 22) in r.stdout.decode(), r.stdout
    assert (tmp_path / "mc.bin").read_bytes() == (tmp_path / "dn.bin").read_bytes()


def test_without_a_temporal_stage_the_flag_changes_nothing(tmp_path, models):
    pics, _, _ = _clip(8)
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    args = ["encode"] + models["ld"] + QP + SIZE + ["-i", tmp_path / "in.yuv", "--denoise", "8:0"]
    _run(args + ["--denoise-out", tmp_path / "a.yuv", "-o", tmp_path / "a.bin"])
    r = _run(args + ["--denoise-mc", "7", "--denoise-out", tmp_path / "b.yuv", "--mv-log", tmp_path / "mv.json", "-o", tmp_path / "b.bin"])
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes()
    assert (tmp_path / "a.yuv").read_bytes() == (tmp_path / "b.yuv").read_bytes()
    assert "(0 of 0 blocks moved)" in r.stdout.decode()
    assert json.loads((tmp_path / "mv.json").read_text())["pictures"] == []        # nothing was searched


@pytest.mark.parametrize("bits,fmt", [(8, "420"), (10, "422")])
def test_the_mv_log_holds_the_numpy_vectors_sums(tmp_path, models, bits, fmt):
    pics, filtered, mvs = _clip(bits, fmt)
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    kind = ["--src-type", "yuv422"] if fmt == "422" else []
    args = ["encode"] + models["intra"] + _depth(bits) + kind + QP + SIZE + ["-i", tmp_path / "in.yuv"]
    _run(args + MC + ["-o", tmp_path / "plain.bin"])
    _run(args + ["--denoise", "8", "--denoise-mc", "%d:%d" % (R, LAM), "--mv-log", tmp_path / "mv.json", "-o", tmp_path / "log.bin"])
    assert (tmp_path / "log.bin").read_bytes() == (tmp_path / "plain.bin").read_bytes()      # the log changes no stream
    want = []
    for i, m in enumerate(mvs):
        if m is None:
            continue
        mv, sad = m[0].astype(np.int64), m[1].astype(np.int64)
        want.append({"idx": i, "blocks": mv.shape[0] * mv.shape[1], "nonzero": int(mv.any(axis=-1).sum()),
                     "sum_abs_dx": int(np.abs(mv[..., 0]).sum()), "sum_abs_dy": int(np.abs(mv[..., 1]).sum()),
                     "max_abs": int(np.abs(mv).max()), "sum_sad": int(sad.sum())})
    assert len(want) == N - 1 and want[0]["nonzero"] > 0
    doc = json.loads((tmp_path / "mv.json").read_text())
    assert doc == {"range": R, "lambda": LAM, "block": 16, "width": W, "height": H, "pictures": want}


def test_another_range_and_lambda_reach_the_search(tmp_path, models):
    pics, _, _ = _clip(8)
    filtered, mvs = motion_np.mc_denoise_clip(pics[:2], 8, 8, 8, 1, 40)               # range 1: the pan of (4, 2) is out of reach
    (tmp_path / "in.yuv").write_bytes(_bytes(pics[:2]))
    _run(["encode"] + models["intra"] + QP + SIZE + ["-i", tmp_path / "in.yuv", "--denoise", "8", "--denoise-mc", "1:40", "--denoise-out",
                                                     tmp_path / "dn.yuv", "--mv-log", tmp_path / "mv.json", "-o", tmp_path / "o.bin"])
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(filtered)
    doc = json.loads((tmp_path / "mv.json").read_text())
    assert doc["range"] == 1 and doc["lambda"] == 40 and doc["pictures"][0]["max_abs"] == int(np.abs(mvs[1][0]).max()) <= 3
    assert doc["pictures"][0]["sum_sad"] == int(mvs[1][1].astype(np.int64).sum())


def test_the_grain_log_still_writes_its_records(tmp_path, models):
    """--grain-log measures what the filter removed: with the flag on, what the compensated filter removed"""
    pics, filtered, _ = _clip(8)
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    enc = ["encode"] + models["ld"] + QP + SIZE + ["-i", tmp_path / "in.yuv"] + MC
    _run(enc + ["-o", tmp_path / "mc.bin"])
    _run(enc + ["--grain-log", tmp_path / "g.json", "-o", tmp_path / "gl.bin"])
    assert (tmp_path / "gl.bin").read_bytes() == (tmp_path / "mc.bin").read_bytes()
    words = [[gnp.stats_plane(s[0], d[0], d[0], 8, 0, 0, 4), gnp.stats_plane(s[1], d[1], d[0], 8, 1, 1, 4),
              gnp.stats_plane(s[2], d[2], d[0], 8, 1, 1, 4)] for s, d in zip(pics, filtered)]
    total = [[sum(wd[p][k] for wd in words) for k in range(16)] for p in range(3)]
    doc = json.loads((tmp_path / "g.json").read_text())
    assert doc["denoise"] == [8, 8] and len(doc["records"]) == 1
    assert doc["records"][0]["pictures"] == N and doc["records"][0]["words"] == total
