"""dcvc encode --denoise / --denoise-out on a real MI355X, against the numpy restatement of the filter
(tests/denoise_np.py) around the tool's own unfiltered paths: the stream of a --denoise run is the stream of a run without the
flag on the clip pre-filtered in numpy - all-intra, LD and HT-S with a ragged chunk, 8-bit and 10-bit yuv420, uyvy (filtered on
its planar 4:2:2 carrier), behind --scale, from stdin with --read-ahead - --denoise 0 changes nothing, --denoise-out holds the
pre-filtered pictures and --quality-log measures against them. Seeded synthetic weights; the clip is 352x288, three pictures of
the synthetic sequence plus seeded noise of sigma 3."""
import json
import os
import subprocess

import numpy as np
import pytest

import denoise_np
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


def _run(args, check=True, data=None):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    r = subprocess.run([TOOL] + args, input=data, capture_output=True, timeout=600)
    assert not check or r.returncode == 0, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("denoise_models")
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "ld.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "hts.dcvw"), "hts", dmc_ht_model("hts", skip_thres=0.15), 0.15)
    intra = ["--intra", str(d / "i.dcvw")]
    return {"intra": intra, "ld": intra + ["--inter", str(d / "ld.dcvw")], "hts": intra + ["--inter", str(d / "hts.dcvw")]}


_clips = {}


def _clip(bits, fmt="420"):
    """(the noisy clip, the clip filtered at 8:8): lists of N pictures (y, u, v); computed once per (depth, chroma format)"""
    key = (bits, fmt)
    if key not in _clips:
        rng = np.random.default_rng(31 + bits)
        s = 1 << (bits - 8)
        dtype = np.uint8 if bits == 8 else np.uint16
        pics = []
        for i in range(N):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=9)
            if fmt == "422":
                uv = np.repeat(uv, 2, axis=1)
            planes = []
            for p in (y, uv[0], uv[1]):
                v = p.astype(np.float64) * s + rng.normal(0, 3 * s, p.shape)
                planes.append(np.clip(np.rint(v), 0, (1 << bits) - 1).astype(dtype))
            pics.append(tuple(planes))
        filtered = denoise_np.denoise_clip(pics, 8, 8, bits)
        assert any(not np.array_equal(a, b) for f, p in zip(filtered, pics) for a, b in zip(f, p))      # the filter changes the clip
        _clips[key] = (pics, filtered)
    return _clips[key]


def _bytes(pics):
    return b"".join(p.astype("<u2" if p.dtype == np.uint16 else np.uint8).tobytes() for pic in pics for p in pic)


def _depth(bits):
    return ["--bit-depth", str(bits)] if bits > 8 else []


def _both(tmp_path, model, bits, dn_extra=()):
    """the --denoise 8 run on the noisy clip and the plain run on the pre-filtered one -> the two streams"""
    pics, filtered = _clip(bits)
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + model + _depth(bits) + QP + SIZE
    r = _run(args + ["-i", str(tmp_path / "in.yuv"), "--denoise", "8", "-o", str(tmp_path / "dn.bin")] + list(dn_extra))
    assert "denoise: spatial 8, temporal 8, %d pictures filtered" % N in r.stdout.decode(), r.stdout
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    return (tmp_path / "dn.bin").read_bytes(), (tmp_path / "pre.bin").read_bytes()


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("inter", ["intra", "ld"])
def test_denoise_writes_the_stream_of_the_prefiltered_clip(tmp_path, models, inter, bits):
    got, want = _both(tmp_path, models[inter], bits)
    assert len(want) > 100 and got == want


def test_a_ragged_hts_chunk(tmp_path, models):
    # 1 I picture, then a chunk of 2 pictures and 6 repeats of the last one: the repeats are the FILTERED picture, not filtered again
    got, want = _both(tmp_path, models["hts"], 8, dn_extra=["--denoise-out", str(tmp_path / "dn.yuv")])
    assert len(want) > 100 and got == want
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(_clip(8)[1])      # the padding pictures are not written


def test_uyvy_is_filtered_on_its_planar_carrier(tmp_path, models):
    pics, filtered = _clip(8, "422")
    carrier = [np.concatenate([p.ravel() for p in pic]) for pic in pics]
    (tmp_path / "wire.yuv").write_bytes(b"".join(wn.pack(c, wn.UYVY, 8, H, W).tobytes() for c in carrier))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + models["ld"] + QP + SIZE
    _run(args + ["-i", str(tmp_path / "wire.yuv"), "--src-type", "uyvy", "--denoise", "8", "--denoise-out", str(tmp_path / "dn.yuv"),
                 "-o", str(tmp_path / "dn.bin")])
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "--src-type", "yuv422", "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(filtered)         # the carrier type's raw layout
    assert (tmp_path / "dn.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_behind_scale_the_scaled_clip_is_filtered(tmp_path, models):
    pics, _ = _clip(8)
    small = [(resample_np.resample_plane(y, h, w, 255), resample_np.resample_plane(u, h // 2, w // 2, 255),
              resample_np.resample_plane(v, h // 2, w // 2, 255)) for y, u, v in pics]
    filtered = denoise_np.denoise_clip(small, 8, 8, 8)
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + models["ld"] + QP
    r = _run(args + SIZE + ["-i", str(tmp_path / "in.yuv"), "--scale", "%dx%d" % (w, h), "--denoise", "8", "--denoise-out",
                            str(tmp_path / "dn.yuv"), "-o", str(tmp_path / "dn.bin")])
    assert "(%dx%d)" % (w, h) in r.stdout.decode()
    _run(args + ["-W", str(w), "-H", str(h), "-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(filtered)         # the clip as coded: at the coded size
    assert (tmp_path / "dn.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_denoise_0_changes_nothing(tmp_path, models):
    pics, _ = _clip(8)
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    args = ["encode"] + models["ld"] + QP + SIZE + ["-i", str(tmp_path / "in.yuv")]
    _run(args + ["-o", str(tmp_path / "plain.bin")])
    _run(args + ["--denoise", "0", "--denoise-out", str(tmp_path / "dn.yuv"), "-o", str(tmp_path / "zero.bin")])
    _run(args + ["--denoise", "0:0", "-o", str(tmp_path / "zz.bin")])
    plain = (tmp_path / "plain.bin").read_bytes()
    assert (tmp_path / "zero.bin").read_bytes() == plain and (tmp_path / "zz.bin").read_bytes() == plain
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(pics)


def test_from_stdin_with_read_ahead(tmp_path, models):
    pics, filtered = _clip(8)
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + models["ld"] + QP + SIZE
    _run(args + ["-i", "-", "--read-ahead", "2", "--denoise", "8", "-o", str(tmp_path / "dn.bin")], data=_bytes(pics))
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "dn.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_denoise_out_and_the_quality_log_hold_the_filtered_clip(tmp_path, models):
    bits = 10
    pics, filtered = _clip(bits)
    (tmp_path / "in.yuv").write_bytes(_bytes(pics))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + models["ld"] + _depth(bits) + QP + SIZE
    _run(args + ["-i", str(tmp_path / "in.yuv"), "--denoise", "8:8", "--quality-log", str(tmp_path / "qd.json"), "--denoise-out",
                 str(tmp_path / "dn.yuv"), "-o", str(tmp_path / "dn.bin")])
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "--quality-log", str(tmp_path / "qp.json"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "dn.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    assert (tmp_path / "dn.yuv").read_bytes() == _bytes(filtered)         # N pictures as coded
    log, plain_log = json.loads((tmp_path / "qd.json").read_text()), json.loads((tmp_path / "qp.json").read_text())
    assert log == plain_log and len(log["units"]) == N                    # measured against the filtered samples
