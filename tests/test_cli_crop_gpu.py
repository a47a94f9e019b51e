"""dcvc encode --crop / --crop-log / --crop-out and dcvc decode --uncrop / --pad / --pad-fill on a real MI355X,
against the numpy restatement (tests/crop_np.py) around the tool's own paths without the flags: the stream of a --crop run is,
byte for byte, the stream of a run without the flag on the numpy-cropped clip - manual windows and auto, all-intra, LD and HT-S
with a ragged chunk, 8 and 10 bits, yuv420 / yuv422 / yuv444, uyvy on its planar carrier, a Y4M source, in front of
--deinterlace, --ivtc, --scale and --denoise, a manual window from stdin with --read-ahead; --crop-log holds the restatement's
probes and window, --crop-out the cropped clip; what a padded decode writes is the numpy pad of what the plain decode writes,
its JSON log is the plain run's and its hashes cover the padded bytes. Seeded synthetic weights; the clips are 96x64 (128x96 in
front of --scale), six pictures of the synthetic sequence inside bars of limited-range black, the first picture all black."""
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import crop_np as cnp
import denoise_np
import resample_np
import wire_np as wn
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, pixfmt, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 64, 96, 6
LETTER, BOTH = (12, 12, 0, 0), (12, 12, 16, 16)          # top, bottom, left, right
QP = ["--qp-i", "30", "--qp-p", "36"]
SUB = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}     # sx, sy


def _size(h=H, w=W):
    return ["-W", str(w), "-H", str(h)]


def _run(args, check=True, data=None):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    r = subprocess.run([TOOL] + [str(a) for a in args], input=data, capture_output=True, timeout=600)
    assert not check or r.returncode == 0, r.stderr.decode()
    return r


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("crop_models")
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "ld.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "hts.dcvw"), "hts", dmc_ht_model("hts", skip_thres=0.15), 0.15)
    intra = ["--intra", str(d / "i.dcvw")]
    return {"intra": intra, "ld": intra + ["--inter", str(d / "ld.dcvw")], "hts": intra + ["--inter", str(d / "hts.dcvw")]}


_clips = {}


def _clip(bars, bits=8, fmt="420", h=H, w=W, black_first=True):
    """N pictures (y, u, v): the synthetic sequence (luma at least 40 code values) inside the bars; made once per kind"""
    key = (bars, bits, fmt, h, w, black_first)
    if key not in _clips:
        s = 1 << (bits - 8)
        dtype = np.uint8 if bits == 8 else np.uint16
        sx, sy = SUB[fmt]
        t, b, l, r = bars
        pics = []
        for i in range(N):
            y, uv = synthetic.synthetic_frame_yuv420(h, w, index=i, seed=9)
            uv = np.repeat(np.repeat(uv, 2 // sy, axis=1), 2 // sx, axis=2)
            planes = [np.maximum(y.astype(np.int64), 40) * s + i % s, uv[0].astype(np.int64) * s, uv[1].astype(np.int64) * s]
            inside = np.zeros((h, w), bool)
            if not (black_first and i == 0):
                inside[t:h - b, l:w - r] = True
            planes[0][~inside] = 16 * s
            for p in (1, 2):
                planes[p][~inside[::sy, ::sx]] = 128 * s
            pics.append(tuple(p.astype(dtype) for p in planes))
        _clips[key] = pics
    return _clips[key]


def _window_of(bars, h=H, w=W):
    t, b, l, r = bars
    return l, t, w - l - r, h - t - b


def _cropped(pics, win, fmt="420"):
    x, y, w, h = win
    sx, sy = SUB[fmt]
    return [(cnp.window_planes(p[0][None], h, w, x, y, 0)[0], cnp.window_planes(p[1][None], h // sy, w // sx, x // sx, y // sy, 0)[0],
             cnp.window_planes(p[2][None], h // sy, w // sx, x // sx, y // sy, 0)[0]) for p in pics]


def _padded(pics, win, h, w, fill, fmt="420"):
    x, y, _, _ = win
    sx, sy = SUB[fmt]
    return [(cnp.window_planes(p[0][None], h, w, -x, -y, fill[0])[0], cnp.window_planes(p[1][None], h // sy, w // sx, -x // sx, -y // sy, fill[1])[0],
             cnp.window_planes(p[2][None], h // sy, w // sx, -x // sx, -y // sy, fill[2])[0]) for p in pics]


def _bytes(pics):
    return b"".join(p.astype("<u2" if p.dtype == np.uint16 else np.uint8).tobytes() for pic in pics for p in pic)


def _pictures(data, h, w, bits, fmt="420"):
    dt = np.dtype("<u2") if bits > 8 else np.dtype(np.uint8)
    sx, sy = SUB[fmt]
    hc, wc = h // sy, w // sx
    a = np.frombuffer(data, dt)
    per = h * w + 2 * hc * wc
    assert a.size % per == 0
    return [(a[i * per:i * per + h * w].reshape(h, w), a[i * per + h * w:i * per + h * w + hc * wc].reshape(hc, wc),
             a[i * per + h * w + hc * wc:(i + 1) * per].reshape(hc, wc)) for i in range(a.size // per)]


def _kind(bits, fmt):
    return (["--bit-depth", str(bits)] if bits > 8 else []) + (["--src-type", "yuv" + fmt] if fmt != "420" else [])


def _win_arg(win):
    return "%dx%d+%d+%d" % (win[2], win[3], win[0], win[1])


def _restated(pics, bits, ax, ay, limit=24, frac=4, min_bar=8, probes=16):
    """what --crop auto decides on the clip -> (window, votes, the log's probes)"""
    h, w = pics[0][0].shape
    idx = cnp.probe_indexes(probes, len(pics))
    counts = [cnp.crop_stats(pics[i][0], limit, bits) for i in idx]
    log = []
    for i, c in zip(idx, counts):
        v = cnp.picture_vote(c, h, w, frac)
        log.append({"idx": i, "voted": v is not None, "top": v and v[0], "bottom": v and v[1], "left": v and v[2], "right": v and v[3]})
    x, y, ww, hh, votes = cnp.crop_window(counts, h, w, frac, min_bar, ax, ay)
    return (x, y, ww, hh), votes, log


def _streams(tmp_path, model, bars, bits=8, fmt="420", extra=(), ay=2):
    """a manual --crop run, a --crop auto run and the plain run on the numpy-cropped clip -> the three streams; the auto run's
    log, output clip and summary line are held against the restatement on the way"""
    clip = _clip(bars, bits, fmt)
    win, votes, probes = _restated(clip, bits, 2, ay)
    assert win == _window_of(bars) and votes == N - 1 and not probes[0]["voted"]          # the black picture does not vote
    cropped = _cropped(clip, win, fmt)
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(cropped))
    common = ["encode"] + model + _kind(bits, fmt) + QP + list(extra)
    _run(common + _size() + ["-i", tmp_path / "in.yuv", "--crop", _win_arg(win), "-o", tmp_path / "manual.bin"])
    r = _run(common + _size() + ["-i", tmp_path / "in.yuv", "--crop", "auto", "--crop-log", tmp_path / "c.json", "--crop-out", tmp_path / "c.yuv",
                                 "-o", tmp_path / "auto.bin"])
    assert "crop: auto, %s of %dx%d (%d of %d pictures voted)" % (_win_arg(win), W, H, votes, N) in r.stdout.decode(), r.stdout
    js = json.loads((tmp_path / "c.json").read_text())
    assert js["probes"] == probes and js["votes"] == votes and js["mode"] == "auto"
    assert js["window"] == {"x": win[0], "y": win[1], "width": win[2], "height": win[3]}
    assert (js["limit"], js["frac"], js["min_bar"], js["source_width"], js["source_height"], js["bit_depth"]) == (24, 4, 8, W, H, bits)
    assert js["src_type"] == js["chroma_format"] == "yuv" + fmt and js["fill"] == [16 << (bits - 8), 128 << (bits - 8), 128 << (bits - 8)]
    if not extra:
        assert (tmp_path / "c.yuv").read_bytes() == _bytes(cropped)
    _run(common + _size(win[3], win[2]) + ["-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    return [(tmp_path / n).read_bytes() for n in ("manual.bin", "auto.bin", "pre.bin")]


@pytest.mark.parametrize("model,bars", [("intra", LETTER), ("ld", BOTH), ("hts", LETTER)])
def test_crop_writes_the_stream_of_the_cropped_clip(tmp_path, models, model, bars):
    # hts: 1 I picture, then a ragged chunk of 5 pictures and 3 repeats of the last one
    manual, auto, want = _streams(tmp_path, models[model], bars)
    assert len(want) > 100 and manual == want and auto == want


@pytest.mark.parametrize("bits,fmt", [(10, "420"), (8, "422"), (8, "444"), (10, "444")])
def test_depths_and_chroma_formats(tmp_path, models, bits, fmt):
    manual, auto, want = _streams(tmp_path, models["ld" if fmt == "420" else "intra"], BOTH, bits, fmt)
    assert len(want) > 100 and manual == want and auto == want


def test_in_front_of_deinterlace_and_ivtc_the_window_keeps_the_field_rows(tmp_path, models):
    # 12 rows of bar are a multiple of 4: the fields of the window are the window of the fields
    for extra in (["--deinterlace", "frame"], ["--ivtc", "film"]):
        manual, auto, want = _streams(tmp_path, models["ld"], LETTER, extra=extra, ay=4)
        assert len(want) > 100 and manual == want and auto == want
    # bars of 10 rows: auto rounds down to 8, a manual window at 10 is refused
    clip = _clip((10, 10, 0, 0))
    win, _, _ = _restated(clip, 8, 2, 4)
    assert win == (0, 8, W, H - 16)
    (tmp_path / "ten.yuv").write_bytes(_bytes(clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(_cropped(clip, win)))
    enc = ["encode"] + models["ld"] + QP + ["--deinterlace", "frame"]
    r = _run(enc + _size() + ["-i", tmp_path / "ten.yuv", "--crop", "auto", "-o", tmp_path / "ten.bin"])
    assert "crop: auto, 96x48+0+8 of 96x64" in r.stdout.decode()
    _run(enc + _size(win[3], win[2]) + ["-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    assert (tmp_path / "ten.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    r = _run(enc + _size() + ["-i", tmp_path / "ten.yuv", "--crop", "96x44+0+10", "-o", tmp_path / "no.bin"], check=False)
    assert r.returncode == 2 and b"4 (vertical)" in r.stderr and not (tmp_path / "no.bin").exists()


def test_in_front_of_denoise(tmp_path, models):
    clip = _clip(LETTER)
    win = _window_of(LETTER)
    cropped = _cropped(clip, win)
    filtered = denoise_np.denoise_clip(cropped, 8, 8, 8)
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(filtered))
    enc = ["encode"] + models["ld"] + QP
    _run(enc + _size() + ["-i", tmp_path / "in.yuv", "--crop", "auto", "--denoise", "8", "--crop-out", tmp_path / "c.yuv", "--denoise-out",
                          tmp_path / "dn.yuv", "-o", tmp_path / "c.bin"])
    _run(enc + _size(win[3], win[2]) + ["-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    assert (tmp_path / "c.yuv").read_bytes() == _bytes(cropped) and (tmp_path / "dn.yuv").read_bytes() == _bytes(filtered)
    assert (tmp_path / "c.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()


def test_in_front_of_scale_and_behind_out_size(tmp_path, models):
    h2, w2, bars = 96, 128, (16, 16, 0, 0)
    clip = _clip(bars, h=h2, w=w2)
    win = _window_of(bars, h2, w2)                      # 128x64+0+16, coded at 96x48
    cropped = _cropped(clip, win)
    small = [(resample_np.resample_plane(y, 48, 96, 255), resample_np.resample_plane(u, 24, 48, 255), resample_np.resample_plane(v, 24, 48, 255))
             for y, u, v in cropped]
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(small))
    enc = ["encode"] + models["ld"] + QP
    r = _run(enc + _size(h2, w2) + ["-i", tmp_path / "in.yuv", "--crop", "auto", "--scale", "96x48", "--crop-log", tmp_path / "c.json", "--crop-out",
                                    tmp_path / "c.yuv", "-o", tmp_path / "c.bin"])
    assert "crop: auto, 128x64+0+16 of 128x96" in r.stdout.decode()
    _run(enc + _size(48, 96) + ["-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    assert (tmp_path / "c.yuv").read_bytes() == _bytes(cropped)               # at the window's size, in front of the resampler
    assert (tmp_path / "c.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    # decode: resampled to the window's size, then padded to the source's
    dec = ["decode"] + models["ld"] + ["-i", tmp_path / "c.bin", "--out-size", "128x64"]
    _run(dec + ["-o", tmp_path / "plain.yuv"])
    _run(dec + ["--uncrop", tmp_path / "c.json", "-o", tmp_path / "full.yuv"])
    plain = _pictures((tmp_path / "plain.yuv").read_bytes(), 64, 128, 8)
    assert (tmp_path / "full.yuv").read_bytes() == _bytes(_padded(plain, win, h2, w2, (16, 128, 128)))
    # another size than the window's is refused, at the coded size and behind --out-size
    for size in (["--out-size", "64x32"], []):
        r = _run(["decode"] + models["ld"] + ["-i", tmp_path / "c.bin"] + size + ["--uncrop", tmp_path / "c.json", "-o", tmp_path / "no.yuv"],
                 check=False)
        assert r.returncode == 2 and b"--uncrop: the log's window is 128x64, the pictures arriving are" in r.stderr, r.stderr


def test_uyvy_on_its_planar_carrier(tmp_path, models):
    clip = _clip(BOTH, fmt="422")
    win = _window_of(BOTH)
    cropped = _cropped(clip, win, "422")
    carrier = [np.concatenate([p.ravel() for p in pic]) for pic in clip]
    (tmp_path / "wire.yuv").write_bytes(b"".join(wn.pack(c, wn.UYVY, 8, H, W).tobytes() for c in carrier))
    (tmp_path / "pre.yuv").write_bytes(_bytes(cropped))
    enc = ["encode"] + models["intra"] + QP
    r = _run(enc + _size() + ["-i", tmp_path / "wire.yuv", "--src-type", "uyvy", "--crop", "auto", "--crop-out", tmp_path / "c.yuv", "--crop-log",
                              tmp_path / "c.json", "-o", tmp_path / "c.bin"])
    assert "crop: auto, %s of 96x64" % _win_arg(win) in r.stdout.decode()
    _run(enc + _size(win[3], win[2]) + ["-i", tmp_path / "pre.yuv", "--src-type", "yuv422", "-o", tmp_path / "pre.bin"])
    assert (tmp_path / "c.yuv").read_bytes() == _bytes(cropped)               # the carrier type's raw layout
    assert (tmp_path / "c.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    js = json.loads((tmp_path / "c.json").read_text())
    assert js["src_type"] == "uyvy" and js["chroma_format"] == "yuv422"


def test_a_y4m_source(tmp_path, models):
    clip = _clip(LETTER)
    win = _window_of(LETTER)
    head = pixfmt.y4m_write_header(W, H, pixfmt.DCVC_PIX_YUV420P, 8)
    (tmp_path / "in.y4m").write_bytes(head + b"".join(b"FRAME\n" + _bytes([f]) for f in clip))
    (tmp_path / "pre.yuv").write_bytes(_bytes(_cropped(clip, win)))
    enc = ["encode"] + models["ld"] + QP
    r = _run(enc + ["-i", tmp_path / "in.y4m", "--crop", "auto", "-o", tmp_path / "c.bin"])
    assert "crop: auto, 96x40+0+12 of 96x64 (5 of 6 pictures voted)" in r.stdout.decode()
    _run(enc + _size(win[3], win[2]) + ["-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    assert (tmp_path / "c.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    # -n 3: the probes are spread over the three frames the run reads
    r = _run(enc + ["-i", tmp_path / "in.y4m", "-n", "3", "--crop", "auto:24:4:8:2", "--crop-log", tmp_path / "c.json", "-o", tmp_path / "n3.bin"])
    assert "(1 of 2 pictures voted)" in r.stdout.decode()              # frame 0 is the black one
    assert [p["idx"] for p in json.loads((tmp_path / "c.json").read_text())["probes"]] == cnp.probe_indexes(2, 3) == [0, 2]


def test_a_manual_window_from_stdin_with_read_ahead(tmp_path, models):
    clip = _clip(BOTH)
    win = _window_of(BOTH)
    (tmp_path / "pre.yuv").write_bytes(_bytes(_cropped(clip, win)))
    enc = ["encode"] + models["ld"] + QP
    r = _run(enc + _size() + ["-i", "-", "--read-ahead", "2", "--crop", _win_arg(win), "--crop-log", tmp_path / "c.json", "-o", tmp_path / "c.bin"],
             data=_bytes(clip))
    assert "crop: manual, %s of 96x64 (0 of 0 pictures voted)" % _win_arg(win) in r.stdout.decode()
    _run(enc + _size(win[3], win[2]) + ["-i", tmp_path / "pre.yuv", "-o", tmp_path / "pre.bin"])
    assert (tmp_path / "c.bin").read_bytes() == (tmp_path / "pre.bin").read_bytes()
    js = json.loads((tmp_path / "c.json").read_text())
    assert js["mode"] == "manual" and js["probes"] == [] and js["limit"] is None and js["window"]["x"] == 16


def test_a_clip_without_bars_and_a_run_without_the_flag(tmp_path, models):
    clip = _clip((0, 0, 0, 0), black_first=False)
    assert _restated(clip, 8, 2, 2)[0] == (0, 0, W, H)
    (tmp_path / "in.yuv").write_bytes(_bytes(clip))
    enc = ["encode"] + models["ld"] + QP + _size() + ["-i", tmp_path / "in.yuv"]
    r = _run(enc + ["-o", tmp_path / "raw.bin"])
    assert "crop" not in r.stdout.decode() and "encoded 6 pictures" in r.stdout.decode()
    raw = (tmp_path / "raw.bin").read_bytes()
    r = _run(enc + ["--crop", "auto", "--crop-out", tmp_path / "c.yuv", "-o", tmp_path / "auto.bin"])
    assert "crop: auto, 96x64+0+0 of 96x64 (6 of 6 pictures voted)" in r.stdout.decode()
    assert len(raw) > 100 and (tmp_path / "auto.bin").read_bytes() == raw and (tmp_path / "c.yuv").read_bytes() == _bytes(clip)
    _run(enc + ["--crop", "96x64+0+0", "-o", tmp_path / "whole.bin"])
    assert (tmp_path / "whole.bin").read_bytes() == raw
    # bars below min_bar stay: 6 rows are content as far as the window goes
    (tmp_path / "six.yuv").write_bytes(_bytes(_clip((6, 6, 0, 0))))
    r = _run(["encode"] + models["intra"] + QP + _size() + ["-i", tmp_path / "six.yuv", "--crop", "auto", "-o", tmp_path / "six.bin"])
    assert "crop: auto, 96x64+0+0 of 96x64" in r.stdout.decode()
    r = _run(["encode"] + models["intra"] + QP + _size() + ["-i", tmp_path / "six.yuv", "--crop", "auto:24:4:4", "-o", tmp_path / "six4.bin"])
    assert "crop: auto, 96x52+0+6 of 96x64" in r.stdout.decode()


# ---------------------------------------------------------------- decode
def _log(path):
    log = json.loads(path.read_text())
    log.pop("test_time")
    return log


@pytest.fixture(scope="module")
def coded(tmp_path_factory, models):
    """per (bits, fmt): an LD stream of the letter- and pillarboxed clip coded with --crop auto, its log, --crop-out and the
    plain decode"""
    made = {}

    def make(bits, fmt):
        if (bits, fmt) not in made:
            d = tmp_path_factory.mktemp("crop_coded")
            (d / "in.yuv").write_bytes(_bytes(_clip(BOTH, bits, fmt)))
            kind = _kind(bits, fmt)
            _run(["encode"] + models["ld"] + kind + QP + _size() + ["-i", d / "in.yuv", "--crop", "auto", "--crop-log", d / "c.json", "--crop-out",
                                                                      d / "c.yuv", "-o", d / "s.bin"])
            dec = ["decode"] + models["ld"] + kind + ["-i", d / "s.bin", "--ref", d / "c.yuv"]
            _run(dec + ["-o", d / "plain.yuv", "--json", d / "plain.json"])
            made[(bits, fmt)] = (d, dec, (d / "plain.yuv").read_bytes())
        return made[(bits, fmt)]
    return make


@pytest.mark.parametrize("bits,fmt", [(8, "420"), (10, "420"), (8, "422"), (8, "444")])
def test_uncrop_writes_the_numpy_pad_of_the_plain_decode(tmp_path, coded, bits, fmt):
    d, dec, plain = coded(bits, fmt)
    win = _window_of(BOTH)
    s = 1 << (bits - 8)
    pics = _pictures(plain, win[3], win[2], bits, fmt)
    assert len(pics) == N
    want = _bytes(_padded(pics, win, H, W, (16 * s, 128 * s, 128 * s), fmt))
    _run(dec + ["--uncrop", d / "c.json", "-o", tmp_path / "full.yuv", "--json", tmp_path / "full.json", "--hash-log", tmp_path / "h.txt"])
    assert (tmp_path / "full.yuv").read_bytes() == want and len(want) == len(_bytes(_clip(BOTH, bits, fmt)))
    # --ref (the cropped clip), PSNR and the JSON log read the unpadded picture
    assert _log(tmp_path / "full.json") == _log(d / "plain.json")
    # the hashes cover the padded picture at the source's size
    lines = (tmp_path / "h.txt").read_text().splitlines()
    assert lines[0].split()[-2:] == [str(W), str(H)]
    assert lines[-1] == "sequence %08x %d" % (zlib.crc32(want), len(want))
    r = _run(dec + ["--uncrop", d / "c.json", "--verify-hash", tmp_path / "h.txt"])
    assert "verified %d pictures" % N in r.stdout.decode()
    # the plain run's hashes are another picture's
    r = _run(dec + ["--verify-hash", tmp_path / "h.txt"], check=False)
    assert r.returncode == 2
    # --pad with values of its own; and --pad-fill over the log's
    fill = (200 * s, 90 * s, 1)
    want2 = _bytes(_padded(pics, win, H, W, fill, fmt))
    _run(dec + ["--pad", "%dx%d+%d+%d" % (W, H, win[0], win[1]), "--pad-fill", "%d:%d:%d" % fill, "-o", tmp_path / "p.yuv"])
    assert (tmp_path / "p.yuv").read_bytes() == want2
    _run(dec + ["--uncrop", d / "c.json", "--pad-fill", "%d:%d:%d" % fill, "-o", tmp_path / "q.yuv"])
    assert (tmp_path / "q.yuv").read_bytes() == want2
    _run(dec + ["--pad", "%dx%d+%d+%d" % (W, H, win[0], win[1]), "-o", tmp_path / "r.yuv"])
    assert (tmp_path / "r.yuv").read_bytes() == want


def test_a_y4m_output_carries_the_source_size_and_grain_stays_inside(tmp_path, coded):
    d, dec, plain = coded(8, "420")
    win = _window_of(BOTH)
    _run(dec + ["--uncrop", d / "c.json", "-o", tmp_path / "full.y4m"])
    y4m = (tmp_path / "full.y4m").read_bytes()
    head = y4m[:y4m.index(b"\n") + 1]
    assert b" W%d H%d " % (W, H) in head
    want = _padded(_pictures(plain, win[3], win[2], 8), win, H, W, (16, 128, 128))
    assert y4m == head + b"".join(b"FRAME\n" + _bytes([p]) for p in want)
    # shown = pad(grain(picture)): the inside is the grained plain output, the bars hold the fill and no grain
    _run(dec + ["--grain-strength", "40", "-o", tmp_path / "g.yuv"])
    grained = (tmp_path / "g.yuv").read_bytes()
    assert grained != plain
    _run(dec + ["--grain-strength", "40", "--uncrop", d / "c.json", "-o", tmp_path / "gfull.yuv"])
    assert (tmp_path / "gfull.yuv").read_bytes() == _bytes(_padded(_pictures(grained, win[3], win[2], 8), win, H, W, (16, 128, 128)))
    # a picture that does not fit the source, and a log of another depth
    r = _run(dec + ["--pad", "96x48+16+12", "-o", tmp_path / "no.yuv"], check=False)
    assert r.returncode == 2 and b"does not lie inside 96x48" in r.stderr, r.stderr
    r = _run(dec + ["--pad", "96x64+15+12", "-o", tmp_path / "no.yuv"], check=False)
    assert r.returncode == 2 and b"multiples of the chroma subsampling" in r.stderr, r.stderr
