"""dcvc encode --deinterlace / --field-order / --deinterlace-out on a real MI355X, against the numpy restatement
of the filter (tests/deinterlace_np.py) around the tool's own paths without the flag: the stream of a --deinterlace run is the
stream of a run without the flag on the clip deinterlaced in numpy - frame and field mode, both field orders, all-intra, LD and
HT-S with a ragged chunk, 8-bit and 10-bit yuv420, uyvy (on its planar 4:2:2 carrier), It / Ib Y4M files, in front of --scale and
--denoise, from stdin with --read-ahead, -n in field mode - --deinterlace-out holds the restatement's pictures and --quality-log
measures against them. Seeded synthetic weights; the clip is 352x288, three frames woven from six pictures of the synthetic
sequence."""
import json
import os
import subprocess

import numpy as np
import pytest

import deinterlace_np as dnp
import denoise_np
import resample_np
import wire_np as wn
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, pixfmt, synthetic

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
    d = tmp_path_factory.mktemp("deinterlace_models")
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "ld.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "hts.dcvw"), "hts", dmc_ht_model("hts", skip_thres=0.15), 0.15)
    intra = ["--intra", str(d / "i.dcvw")]
    return {"intra": intra, "ld": intra + ["--inter", str(d / "ld.dcvw")], "hts": intra + ["--inter", str(d / "hts.dcvw")]}


_frames, _outputs = {}, {}


def _clip(bits, order="tff", fmt="420"):
    """N woven frames (y, u, v): frame f holds the rows of the earlier field's parity from picture 2 f of the synthetic sequence
    and the others from picture 2 f + 1; chroma rows alternate between the fields as luma rows do. Computed once."""
    key = (bits, order, fmt)
    if key not in _frames:
        s = 1 << (bits - 8)
        dtype = np.uint8 if bits == 8 else np.uint16
        p0 = 0 if order == "tff" else 1
        pics = []
        for i in range(2 * N):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=9)
            if fmt == "422":
                uv = np.repeat(uv, 2, axis=1)
            # the low bits of a deeper sample are filled, so that the deeper clip is no scaled copy
            pics.append(tuple((p.astype(np.int64) * s + (p.astype(np.int64) * 7) % s).astype(dtype) for p in (y, uv[0], uv[1])))
        frames = []
        for f in range(N):
            planes = []
            for a, b in zip(pics[2 * f], pics[2 * f + 1]):
                wv = np.empty_like(a)
                wv[p0::2], wv[1 - p0::2] = a[p0::2], b[1 - p0::2]
                planes.append(wv)
            frames.append(tuple(planes))
        _frames[key] = frames
    return _frames[key]


def _restated(bits, mode, order, thr=10, fmt="420"):
    key = (bits, mode, order, thr, fmt)
    if key not in _outputs:
        frames = _clip(bits, order, fmt)
        out = dnp.deinterlace_clip(frames, mode, order, thr, bits)
        assert len(out) == N * (2 if mode == "field" else 1)
        k = 2 if mode == "field" else 1
        assert all(not np.array_equal(o[0], frames[i // k][0]) for i, o in enumerate(out))      # the filter changes the clip
        _outputs[key] = out
    return _outputs[key]


def _bytes(pics):
    return b"".join(p.astype("<u2" if p.dtype == np.uint16 else np.uint8).tobytes() for pic in pics for p in pic)


def _depth(bits):
    return ["--bit-depth", str(bits)] if bits > 8 else []


def _summary(mode, order, thr, pictures, frames):
    return "deinterlace: %s, %s, threshold %d, %d pictures from %d frames" % (mode, order, thr, pictures, frames)


def _both(tmp_path, model, bits, mode, order, extra=(), thr=None):
    """the --deinterlace run on the woven clip and the plain run on the clip deinterlaced in numpy -> the two streams"""
    t = 10 if thr is None else thr
    frames, pre = _clip(bits, order), _restated(bits, mode, order, t)
    (tmp_path / "in.yuv").write_bytes(_bytes(frames))
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    args = ["encode"] + model + _depth(bits) + QP + SIZE
    flag = mode if thr is None else "%s:%d" % (mode, thr)
    r = _run(args + ["-i", str(tmp_path / "in.yuv"), "--deinterlace", flag, "--field-order", order, "-o", str(tmp_path / "di.bin")] + list(extra))
    assert _summary(mode, order, t, len(pre), N) in r.stdout.decode(), r.stdout
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    return (tmp_path / "di.bin").read_bytes(), (tmp_path / "pre.bin").read_bytes()


@pytest.mark.parametrize("inter", ["intra", "ld"])
@pytest.mark.parametrize("order", ["tff", "bff"])
@pytest.mark.parametrize("mode", ["frame", "field"])
def test_deinterlace_writes_the_stream_of_the_deinterlaced_clip(tmp_path, models, mode, order, inter):
    got, want = _both(tmp_path, models[inter], 8, mode, order)
    assert len(want) > 100 and got == want


@pytest.mark.parametrize("mode", ["frame", "field"])
def test_10_bit_sources(tmp_path, models, mode):
    got, want = _both(tmp_path, models["ld"], 10, mode, "tff", thr=6)
    assert len(want) > 100 and got == want


def test_a_ragged_hts_chunk_in_field_mode(tmp_path, models):
    # 6 pictures: 1 I picture, then a chunk of 5 pictures and 3 repeats of the last OUTPUT picture
    got, want = _both(tmp_path, models["hts"], 8, "field", "tff", extra=["--deinterlace-out", str(tmp_path / "di.yuv")])
    assert len(want) > 100 and got == want
    assert (tmp_path / "di.yuv").read_bytes() == _bytes(_restated(8, "field", "tff"))      # the padding pictures are not written


def test_the_bob_interpolator(tmp_path, models):
    got, want = _both(tmp_path, models["intra"], 8, "field", "tff", thr=0)
    assert len(want) > 100 and got == want


def test_uyvy_is_deinterlaced_on_its_planar_carrier(tmp_path, models):
    frames, pre = _clip(8, "tff", "422"), _restated(8, "field", "tff", fmt="422")
    carrier = [np.concatenate([p.ravel() for p in pic]) for pic in frames]
    (tmp_path / "wire.yuv").write_bytes(b"".join(wn.pack(c, wn.UYVY, 8, H, W).tobytes() for c in carrier))
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    args = ["encode"] + models["ld"] + QP + SIZE
    _run(args + ["-i", str(tmp_path / "wire.yuv"), "--src-type", "uyvy", "--deinterlace", "field", "--deinterlace-out", str(tmp_path / "di.yuv"),
                 "-o", str(tmp_path / "di.bin")])
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "--src-type", "yuv422", "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "di.yuv").read_bytes() == _bytes(pre)              # the carrier type's raw layout
    assert (tmp_path / "di.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


@pytest.mark.parametrize("field,order", [("It", "tff"), ("Ib", "bff")])
def test_a_y4m_file_supplies_the_field_order(tmp_path, models, field, order):
    frames, pre = _clip(8, order), _restated(8, "frame", order)
    head = pixfmt.y4m_write_header(W, H, pixfmt.DCVC_PIX_YUV420P, 8)
    assert b" Ip " in head
    (tmp_path / "in.y4m").write_bytes(head.replace(b" Ip ", b" %s " % field.encode()) + b"".join(b"FRAME\n" + _bytes([f]) for f in frames))
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    args = ["encode"] + models["ld"] + QP
    r = _run(args + ["-i", str(tmp_path / "in.y4m"), "--deinterlace", "frame", "-o", str(tmp_path / "di.bin")])
    assert _summary("frame", order, 10, N, N) in r.stdout.decode()
    _run(args + SIZE + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "di.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    # without the flag the file is refused as ever
    r = _run(args + ["-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "no.bin")], check=False)
    assert r.returncode == 2 and b"interlaced material is not supported" in r.stderr and not (tmp_path / "no.bin").exists()


def test_in_front_of_scale_the_source_frames_are_deinterlaced(tmp_path, models):
    frames, pre = _clip(8), _restated(8, "field", "tff")
    small = [(resample_np.resample_plane(y, h, w, 255), resample_np.resample_plane(u, h // 2, w // 2, 255),
              resample_np.resample_plane(v, h // 2, w // 2, 255)) for y, u, v in pre]
    (tmp_path / "in.yuv").write_bytes(_bytes(frames))
    (tmp_path / "pre.yuv").write_bytes(_bytes(small))
    args = ["encode"] + models["ld"] + QP
    r = _run(args + SIZE + ["-i", str(tmp_path / "in.yuv"), "--scale", "%dx%d" % (w, h), "--deinterlace", "field", "--deinterlace-out",
                            str(tmp_path / "di.yuv"), "-o", str(tmp_path / "di.bin")])
    assert "(%dx%d)" % (w, h) in r.stdout.decode()
    _run(args + ["-W", str(w), "-H", str(h), "-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "di.yuv").read_bytes() == _bytes(pre)              # at the SOURCE size, in front of the resampler
    assert (tmp_path / "di.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_in_front_of_denoise(tmp_path, models):
    frames, pre = _clip(8), _restated(8, "frame", "tff")
    filtered = denoise_np.denoise_clip(pre, 8, 8, 8)
    (tmp_path / "in.yuv").write_bytes(_bytes(frames))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + models["ld"] + QP + SIZE
    _run(args + ["-i", str(tmp_path / "in.yuv"), "--deinterlace", "frame", "--denoise", "8", "--deinterlace-out", str(tmp_path / "di.yuv"),
                 "--denoise-out", str(tmp_path / "dn.yuv"), "-o", str(tmp_path / "di.bin")])
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "di.yuv").read_bytes() == _bytes(pre) and (tmp_path / "dn.yuv").read_bytes() == _bytes(filtered)
    assert (tmp_path / "di.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_from_stdin_with_read_ahead_in_field_mode(tmp_path, models):
    frames, pre = _clip(8), _restated(8, "field", "tff")
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    args = ["encode"] + models["ld"] + QP + SIZE
    r = _run(args + ["-i", "-", "--read-ahead", "2", "--deinterlace", "field", "-o", str(tmp_path / "di.bin")], data=_bytes(frames))
    assert _summary("field", "tff", 10, 2 * N, N) in r.stdout.decode()    # the pipe's end: both fields of the last frame are coded
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "di.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_n_counts_coded_pictures_in_field_mode(tmp_path, models):
    frames, pre = _clip(8), _restated(8, "field", "tff")
    (tmp_path / "in.yuv").write_bytes(_bytes(frames))
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    args = ["encode"] + models["ld"] + QP + SIZE
    r = _run(args + ["-i", str(tmp_path / "in.yuv"), "-n", "5", "--deinterlace", "field", "--deinterlace-out", str(tmp_path / "di.yuv"),
                     "--latency-log", str(tmp_path / "lat.json"), "-o", str(tmp_path / "di.bin")])
    assert _summary("field", "tff", 10, 5, 3) in r.stdout.decode()
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-n", "5", "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "di.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    assert (tmp_path / "di.yuv").read_bytes() == _bytes(pre[:5])
    units = json.loads((tmp_path / "lat.json").read_text())["units"]
    assert sum(u["pictures"] for u in units) == 5
    # and all six without -n
    _run(args + ["-i", str(tmp_path / "in.yuv"), "--deinterlace", "field", "-o", str(tmp_path / "all.bin")])
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre6.bin")])
    assert (tmp_path / "all.bin").read_bytes() == (tmp_path / "pre6.bin").read_bytes() != (tmp_path / "pre.bin").read_bytes()


def test_deinterlace_out_and_the_quality_log_hold_the_deinterlaced_clip(tmp_path, models):
    bits = 10
    frames, pre = _clip(bits), _restated(bits, "field", "tff")
    (tmp_path / "in.yuv").write_bytes(_bytes(frames))
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    args = ["encode"] + models["ld"] + _depth(bits) + QP + SIZE
    _run(args + ["-i", str(tmp_path / "in.yuv"), "--deinterlace", "field:10", "--quality-log", str(tmp_path / "qd.json"), "--deinterlace-out",
                 str(tmp_path / "di.yuv"), "-o", str(tmp_path / "di.bin")])
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "--quality-log", str(tmp_path / "qp.json"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "di.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    assert (tmp_path / "di.yuv").read_bytes() == _bytes(pre)              # 2 N pictures at the source size
    log, plain_log = json.loads((tmp_path / "qd.json").read_text()), json.loads((tmp_path / "qp.json").read_text())
    assert log == plain_log and len(log["units"]) == 2 * N                # measured against the deinterlaced samples
    # the decoder is given --deinterlace-out as its reference and needs no flag: the stream is an ordinary one
    r = _run(["decode"] + models["ld"] + _depth(bits) + ["-i", str(tmp_path / "di.bin"), "--ref", str(tmp_path / "di.yuv"), "--json",
                                                         str(tmp_path / "dec.json"), "-o", str(tmp_path / "rec.yuv")])
    assert r.returncode == 0 and len((tmp_path / "rec.yuv").read_bytes()) == len(_bytes(pre))


def test_a_run_without_the_flag_is_untouched(tmp_path, models):
    """the woven clip coded as it is, three ways that share no deinterlacer state: a raw file, an Ip Y4M file and stdin with
    read-ahead give one stream, and a --deinterlace run gives another"""
    frames = _clip(8)
    (tmp_path / "in.yuv").write_bytes(_bytes(frames))
    head = pixfmt.y4m_write_header(W, H, pixfmt.DCVC_PIX_YUV420P, 8)
    (tmp_path / "in.y4m").write_bytes(head + b"".join(b"FRAME\n" + _bytes([f]) for f in frames))
    args = ["encode"] + models["ld"] + QP
    r = _run(args + SIZE + ["-i", str(tmp_path / "in.yuv"), "-o", str(tmp_path / "raw.bin")])
    assert "deinterlace" not in r.stdout.decode()
    _run(args + ["-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "y4m.bin")])
    _run(args + SIZE + ["-i", "-", "--read-ahead", "2", "-o", str(tmp_path / "pipe.bin")], data=_bytes(frames))
    raw = (tmp_path / "raw.bin").read_bytes()
    assert len(raw) > 100 and (tmp_path / "y4m.bin").read_bytes() == raw and (tmp_path / "pipe.bin").read_bytes() == raw
    _run(args + SIZE + ["-i", str(tmp_path / "in.yuv"), "--deinterlace", "frame", "-o", str(tmp_path / "di.bin")])
    assert (tmp_path / "di.bin").read_bytes() != raw
