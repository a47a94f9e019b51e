"""dcvc encode --ivtc / --field-order / --ivtc-out / --ivtc-log on a real MI355X, against the numpy restatement
(tests/ivtc_np.py, with tests/deinterlace_np.py for the frames it finds combed) around the tool's own paths without the flag: the
stream of an --ivtc run is the stream of a run without the flag on the clip the restatement makes - film and match mode, both
field orders, all-intra, LD and HT-S with a ragged chunk, 8-bit and 10-bit yuv420, uyvy (on its planar 4:2:2 carrier), an It Y4M
file, in front of --scale and --denoise, from stdin with --read-ahead, -n that ends inside a cycle, a clip with a ragged last
cycle and one whose middle third is true video - --ivtc-out holds the restatement's pictures and --ivtc-log its words and
decisions. Seeded synthetic weights; the clips are 96x64 (128x96 in front of --scale): the synthetic sequence as film pictures,
carried by 2:3 pulldown."""
import json
import os
import subprocess

import numpy as np
import pytest

import denoise_np
import ivtc_np as inp
import resample_np
import wire_np as wn
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, pixfmt, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W = 64, 96
QP = ["--qp-i", "30", "--qp-p", "36"]


def _size(h=H, w=W):
    return ["-W", str(w), "-H", str(h)]


def _run(args, check=True, data=None):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    r = subprocess.run([TOOL] + args, input=data, capture_output=True, timeout=600)
    assert not check or r.returncode == 0, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("ivtc_models")
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "ld.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "hts.dcvw"), "hts", dmc_ht_model("hts", skip_thres=0.15), 0.15)
    intra = ["--intra", str(d / "i.dcvw")]
    return {"intra": intra, "ld": intra + ["--inter", str(d / "ld.dcvw")], "hts": intra + ["--inter", str(d / "hts.dcvw")]}


_films, _clips, _outputs = {}, {}, {}


def _film(bits, fmt, h, w, n=16):
    """n progressive pictures (y, u, v) of the synthetic sequence (a pan)"""
    key = (bits, fmt, h, w)
    if key not in _films:
        s = 1 << (bits - 8)
        dtype = np.uint8 if bits == 8 else np.uint16
        pics = []
        for i in range(n):
            y, uv = synthetic.synthetic_frame_yuv420(h, w, index=i, seed=9)
            if fmt == "422":
                uv = np.repeat(uv, 2, axis=1)
            # the low bits of a deeper sample are filled, so that the deeper clip is no scaled copy
            pics.append(tuple((p.astype(np.int64) * s + (p.astype(np.int64) * 7) % s).astype(dtype) for p in (y, uv[0], uv[1])))
        _films[key] = pics
    return _films[key]


def _weave(a, b, first):
    return tuple(inp.weave_fields(pa, pb, first) for pa, pb in zip(a, b))


def _clip(frames=10, bits=8, order="tff", fmt="420", h=H, w=W, video=False):
    """`frames` woven frames by 2:3 pulldown of the film; video: frames 5 .. 9 are true video instead - every field a picture of
    its own - between two telecined thirds"""
    key = (frames, bits, order, fmt, h, w, video)
    if key not in _clips:
        film = _film(bits, fmt, h, w)
        tc = [f for f, _, _ in inp.telecine(film, order)]
        assert len(tc) >= frames
        clip = tc[:frames]
        if video:
            first = 0 if order == "tff" else 1
            clip = tc[:5] + [_weave(film[(2 * f) % 16], film[(2 * f + 1) % 16], first) for f in range(5, 10)] + tc[10:frames]
        _clips[key] = clip
    return _clips[key]


def _restated(mode, frames=10, bits=8, order="tff", fmt="420", h=H, w=W, video=False, n=None, args=(9, 80, 10)):
    key = (mode, frames, bits, order, fmt, h, w, video, n, args)
    if key not in _outputs:
        _outputs[key] = inp.ivtc_clip(_clip(frames, bits, order, fmt, h, w, video), mode, order, bits, *args, n=n)
    return _outputs[key]


def _bytes(pics):
    return b"".join(p.astype("<u2" if p.dtype == np.uint16 else np.uint8).tobytes() for pic in pics for p in pic)


def _depth(bits):
    return ["--bit-depth", str(bits)] if bits > 8 else []


def _summary(mode, order, pics, log, args=(9, 80, 10), n_frames=None):
    """the tool's line: P and K count served pictures, D dropped frames"""
    served = [e for e in log if not e["dropped"]][:len(pics)]
    return "ivtc: %s, %s, cthresh %d, mi %d, threshold %d, %d pictures from %d frames (%d matched to the previous frame, %d deinterlaced, %d dropped)" % (
        mode, order, args[0], args[1], args[2], len(pics), len(log) if n_frames is None else n_frames, sum(e["match"] == "p" for e in served),
        sum(e["combed"] for e in served), sum(e["dropped"] for e in log))


def _log_of(path):
    js = json.loads(path.read_text())
    return [{"words": e["words"], "match": e["match"], "combed": e["combed"], "dropped": e["dropped"]} for e in js["frames"]], js


def _both(tmp_path, model, mode, order="tff", bits=8, frames=10, video=False, extra=(), flag=None, args=(9, 80, 10)):
    """the --ivtc run on the woven clip and the plain run on the clip the restatement makes -> the two streams"""
    clip = _clip(frames, bits, order, video=video)
    pre, log = _restated(mode, frames, bits, order, video=video, args=args)
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    common = ["encode"] + model + _depth(bits) + QP + _size()
    r = _run(common + ["-i", str(tmp_path / "in.yuv"), "--ivtc", flag or mode, "--field-order", order, "--ivtc-log", str(tmp_path / "iv.json"),
                       "--ivtc-out", str(tmp_path / "iv.yuv"), "-o", str(tmp_path / "iv.bin")] + list(extra))
    assert _summary(mode, order, pre, log, args) in r.stdout.decode(), r.stdout
    got_log, js = _log_of(tmp_path / "iv.json")
    assert got_log == log and js["mode"] == mode and js["field_order"] == order and js["pictures"] == len(pre)
    assert (js["cthresh"], js["mi"], js["threshold"]) == args
    assert (tmp_path / "iv.yuv").read_bytes() == _bytes(pre)
    _run(common + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    return (tmp_path / "iv.bin").read_bytes(), (tmp_path / "pre.bin").read_bytes()


def test_the_restated_clip_is_the_film():
    """what the streams below are held against: 10 frames -> the 8 film pictures, matches c c p p c, the repeats dropped"""
    film = _film(8, "420", H, W)
    for order in ("tff", "bff"):
        pre, log = _restated("film", order=order)
        assert len(pre) == 8 and "".join(e["match"] for e in log) == "ccppc" * 2 and not any(e["combed"] for e in log)
        assert [i for i, e in enumerate(log) if e["dropped"]] == [2, 7]
        assert all(np.array_equal(p, f) for pic, fp in zip(pre, film) for p, f in zip(pic, fp))
        pre, log = _restated("match", order=order)
        assert len(pre) == 10 and not any(e["dropped"] for e in log)


@pytest.mark.parametrize("order", ["tff", "bff"])
@pytest.mark.parametrize("mode", ["film", "match"])
def test_ivtc_writes_the_stream_of_the_restated_clip(tmp_path, models, mode, order):
    got, want = _both(tmp_path, models["intra"], mode, order)
    assert len(want) > 100 and got == want


@pytest.mark.parametrize("mode,order", [("film", "tff"), ("match", "bff")])
def test_low_delay_runs(tmp_path, models, mode, order):
    got, want = _both(tmp_path, models["ld"], mode, order)
    assert len(want) > 100 and got == want


def test_a_ragged_hts_chunk(tmp_path, models):
    # 8 pictures: 1 I picture, then a chunk of 7 pictures and a repeat of the last OUTPUT picture; --ivtc-out has no padding picture
    got, want = _both(tmp_path, models["hts"], "film")
    assert len(want) > 100 and got == want


@pytest.mark.parametrize("mode", ["film", "match"])
def test_10_bit_sources(tmp_path, models, mode):
    got, want = _both(tmp_path, models["ld"], mode, "tff", bits=10, flag=mode + ":7:60:6", args=(7, 60, 6))
    assert len(want) > 100 and got == want


def test_a_ragged_last_cycle_drops_nothing(tmp_path, models):
    pre, log = _restated("film", frames=12)
    assert len(pre) == 10 and sum(e["dropped"] for e in log) == 2 and not any(e["dropped"] for e in log[10:])
    got, want = _both(tmp_path, models["ld"], "film", frames=12)
    assert len(want) > 100 and got == want


@pytest.mark.parametrize("mode", ["film", "match"])
def test_true_video_in_the_middle_third_is_deinterlaced(tmp_path, models, mode):
    pre, log = _restated(mode, frames=15, video=True)
    assert all(e["combed"] for e in log[5:10]) and not any(e["combed"] for e in log[:5] + log[11:])
    got, want = _both(tmp_path, models["ld"], mode, frames=15, video=True)
    assert len(want) > 100 and got == want


def test_n_that_ends_inside_a_cycle(tmp_path, models):
    clip = _clip(10)
    pre, log = _restated("film", n=6)
    full, _ = _restated("film")
    assert len(pre) == 6 and len(log) == 10 and all(np.array_equal(a, b) for p, q in zip(pre, full) for a, b in zip(p, q))
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(full))
    args = ["encode"] + models["ld"] + QP + _size()
    r = _run(args + ["-i", str(tmp_path / "in.yuv"), "-n", "6", "--ivtc", "film", "--ivtc-out", str(tmp_path / "iv.yuv"), "--ivtc-log",
                     str(tmp_path / "iv.json"), "--latency-log", str(tmp_path / "lat.json"), "-o", str(tmp_path / "iv.bin")])
    assert _summary("film", "tff", pre, log) in r.stdout.decode(), r.stdout
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-n", "6", "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "iv.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    assert (tmp_path / "iv.yuv").read_bytes() == _bytes(pre)
    assert _log_of(tmp_path / "iv.json")[0] == log                # the second cycle was read whole
    assert sum(u["pictures"] for u in json.loads((tmp_path / "lat.json").read_text())["units"]) == 6
    # -n 4 ends with the first cycle: the second one is not read
    r = _run(args + ["-i", str(tmp_path / "in.yuv"), "-n", "4", "--ivtc", "film", "-o", str(tmp_path / "iv4.bin")])
    assert "4 pictures from 5 frames" in r.stdout.decode()
    # match mode: as many frames as pictures
    r = _run(args + ["-i", str(tmp_path / "in.yuv"), "-n", "3", "--ivtc", "match", "-o", str(tmp_path / "m3.bin")])
    assert "3 pictures from 3 frames" in r.stdout.decode()


def test_uyvy_on_its_planar_carrier(tmp_path, models):
    clip = _clip(10, fmt="422")
    pre, log = _restated("film", fmt="422")
    carrier = [np.concatenate([p.ravel() for p in pic]) for pic in clip]
    (tmp_path / "wire.yuv").write_bytes(b"".join(wn.pack(c, wn.UYVY, 8, H, W).tobytes() for c in carrier))
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    args = ["encode"] + models["ld"] + QP + _size()
    r = _run(args + ["-i", str(tmp_path / "wire.yuv"), "--src-type", "uyvy", "--ivtc", "film", "--ivtc-out", str(tmp_path / "iv.yuv"),
                     "-o", str(tmp_path / "iv.bin")])
    assert _summary("film", "tff", pre, log) in r.stdout.decode()
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "--src-type", "yuv422", "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "iv.yuv").read_bytes() == _bytes(pre)              # the carrier type's raw layout
    assert (tmp_path / "iv.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_a_y4m_file_supplies_the_field_order(tmp_path, models):
    clip = _clip(10)
    pre, log = _restated("match")
    head = pixfmt.y4m_write_header(W, H, pixfmt.DCVC_PIX_YUV420P, 8)
    assert b" Ip " in head
    (tmp_path / "in.y4m").write_bytes(head.replace(b" Ip ", b" It ") + b"".join(b"FRAME\n" + _bytes([f]) for f in clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    args = ["encode"] + models["ld"] + QP
    r = _run(args + ["-i", str(tmp_path / "in.y4m"), "--ivtc", "match", "-o", str(tmp_path / "iv.bin")])
    assert _summary("match", "tff", pre, log) in r.stdout.decode()
    _run(args + _size() + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "iv.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    # an Ib file: the other order, and other decisions
    (tmp_path / "b.y4m").write_bytes(head.replace(b" Ip ", b" Ib ") + b"".join(b"FRAME\n" + _bytes([f]) for f in clip))
    r = _run(args + ["-i", str(tmp_path / "b.y4m"), "--ivtc", "match", "-o", str(tmp_path / "b.bin")])
    assert "ivtc: match, bff," in r.stdout.decode() and (tmp_path / "b.bin").read_bytes() != (tmp_path / "iv.bin").read_bytes()


def test_in_front_of_scale_the_source_frames_are_matched(tmp_path, models):
    h2, w2 = 96, 128
    clip = _clip(10, h=h2, w=w2)
    pre, log = _restated("film", h=h2, w=w2)
    small = [(resample_np.resample_plane(y, H, W, 255), resample_np.resample_plane(u, H // 2, W // 2, 255),
              resample_np.resample_plane(v, H // 2, W // 2, 255)) for y, u, v in pre]
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(small))
    args = ["encode"] + models["ld"] + QP
    r = _run(args + _size(h2, w2) + ["-i", str(tmp_path / "in.yuv"), "--scale", "%dx%d" % (W, H), "--ivtc", "film", "--ivtc-out",
                                     str(tmp_path / "iv.yuv"), "-o", str(tmp_path / "iv.bin")])
    assert "(%dx%d)" % (W, H) in r.stdout.decode() and _summary("film", "tff", pre, log) in r.stdout.decode()
    _run(args + _size() + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "iv.yuv").read_bytes() == _bytes(pre)              # at the SOURCE size, in front of the resampler
    assert (tmp_path / "iv.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_in_front_of_denoise(tmp_path, models):
    clip = _clip(10)
    pre, _ = _restated("film")
    filtered = denoise_np.denoise_clip(pre, 8, 8, 8)
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    args = ["encode"] + models["ld"] + QP + _size()
    _run(args + ["-i", str(tmp_path / "in.yuv"), "--ivtc", "film", "--denoise", "8", "--ivtc-out", str(tmp_path / "iv.yuv"),
                 "--denoise-out", str(tmp_path / "dn.yuv"), "-o", str(tmp_path / "iv.bin")])
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "iv.yuv").read_bytes() == _bytes(pre) and (tmp_path / "dn.yuv").read_bytes() == _bytes(filtered)
    assert (tmp_path / "iv.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


@pytest.mark.parametrize("frames", [10, 12])
def test_from_stdin_with_read_ahead(tmp_path, models, frames):
    clip = _clip(frames)
    pre, log = _restated("film", frames=frames)
    (tmp_path / "pre.yuv").write_bytes(_bytes(pre))
    args = ["encode"] + models["ld"] + QP + _size()
    r = _run(args + ["-i", "-", "--read-ahead", "2", "--ivtc", "film", "--ivtc-log", str(tmp_path / "iv.json"), "-o", str(tmp_path / "iv.bin")],
             data=_bytes(clip))
    assert _summary("film", "tff", pre, log) in r.stderr.decode() + r.stdout.decode()          # the pipe's end closes a ragged cycle
    assert _log_of(tmp_path / "iv.json")[0] == log
    _run(args + ["-i", str(tmp_path / "pre.yuv"), "-o", str(tmp_path / "pre.bin")])
    assert (tmp_path / "iv.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_a_run_without_the_flag_is_untouched(tmp_path, models):
    """the woven clip coded as it is, from a file and from stdin with read-ahead, gives one stream without a word about ivtc, and
    an --ivtc run gives another"""
    clip = _clip(10)
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    args = ["encode"] + models["ld"] + QP + _size()
    r = _run(args + ["-i", str(tmp_path / "in.yuv"), "-o", str(tmp_path / "raw.bin")])
    assert "ivtc" not in r.stdout.decode() and "encoded 10 pictures" in r.stdout.decode()
    _run(args + ["-i", "-", "--read-ahead", "2", "-o", str(tmp_path / "pipe.bin")], data=_bytes(clip))
    raw = (tmp_path / "raw.bin").read_bytes()
    assert len(raw) > 100 and (tmp_path / "pipe.bin").read_bytes() == raw
    _run(args + ["-i", str(tmp_path / "in.yuv"), "--ivtc", "match", "-o", str(tmp_path / "iv.bin")])
    assert (tmp_path / "iv.bin").read_bytes() != raw
