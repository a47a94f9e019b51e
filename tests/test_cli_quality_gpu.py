"""dcvc encode --quality-log / --target-psnr on a real MI355X (-m gpu), DESIGN.md 21.

  * the log is the decoder's: the per-picture PSNR lists of --quality-log equal those of dcvc decode --ref --json
    --verbose-json 1 of the same file, for 10-bit yuv420, yuv444, nv12 and rgb24, all-intra, LD and HT-S with a ragged last
    chunk; for 8-bit yuv420, where the decoder sums on the host, within the bound of two fp64 sums;
  * --target-psnr equals rate_control.code_sequence_quality driven with the plug-in's compress / reconstruct / export_state /
    import_state on the same pictures, unit for unit; the target is met and not overshot by a q_index;
  * with --scale the log is the log of a run on the clip pre-scaled in numpy;
  * a run with --quality-log writes the file of the run without it."""
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import pixfmt_np as pn
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, pixfmt, rate_control as rc, synthetic
from oracle import frame_io
from test_cli_gpu import _gpu, _write_yuv
from test_cli_pixfmt_gpu import _file_bytes, _pictures as _pix_pictures
from test_cli_resample_gpu import _pictures as _big_pictures, _scaled, _write as _write_planes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W = 144, 176
SFX = ("", "_y", "_u", "_v")


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=900)


def _models(tmp_path, inter):
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    args = ["--intra", str(tmp_path / "i.dcvw")]
    if inter:
        mp = dmc_ld_model(skip_thres=0.15) if inter == "ld" else dmc_ht_model(inter, skip_thres=0.15)
        export_weights.write_dcvw(str(tmp_path / "p.dcvw"), inter, mp, 0.15)
        args += ["--inter", str(tmp_path / "p.dcvw")]
    return args


def _source(tmp_path, src_type, bits, n):
    """n pictures of the type in a raw file -> (path, the type's flags)"""
    path = str(tmp_path / "in.raw")
    if src_type == "rgb24":
        with open(path, "wb") as f:
            for i in range(n):
                y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=7)
                up = np.repeat(np.repeat(uv, 2, axis=1), 2, axis=2)
                f.write(np.ascontiguousarray(np.stack([y, up[0], up[1]], axis=-1)).tobytes())
        return path, ["--src-type", "rgb24"]
    fmt = {"yuv420": pn.YUV420P, "yuv444": pn.YUV444P, "nv12": pn.NV12}[src_type]
    with open(path, "wb") as f:
        f.write(_file_bytes(_pix_pictures(fmt, bits, H, W, n), fmt, bits))
    return path, ["--src-type", src_type] + (["--bit-depth", str(bits)] if bits > 8 else [])


def _encode_and_decode(tmp_path, models, src, flags, n, extra):
    binf, qlog, dlog = (str(tmp_path / name) for name in ("out.bin", "q.json", "d.json"))
    size = ["-W", str(W), "-H", str(H)]
    r = _run(["encode"] + models + flags + ["-i", src] + size + ["-o", binf, "--quality-log", qlog] + extra)
    print(r.stdout)
    _run(["decode"] + models + flags + ["-i", binf, "--ref", src, "--json", dlog, "--verbose-json", "1", "-n", str(n)])
    return json.loads(open(qlog).read()), json.loads(open(dlog).read())


def _flat(qlog, key):
    return [v for u in qlog["units"] for v in u[key]]


def _check_log_shape(q, n, delay, src_type, bits, target=None):
    assert q["target_psnr"] == target and (q["width"], q["height"]) == (W, H)
    assert (q["src_type"], q["bit_depth"]) == (src_type, bits) and (q["qp_min"], q["qp_max"]) == (0, 63)
    first = 0
    for k, u in enumerate(q["units"]):
        assert u["type"] == ("I" if k == 0 or delay == 0 else "P") and u["first_picture"] == first
        want = 1 if u["type"] == "I" else min(delay, n - first)
        assert u["pictures"] == want == len(u["frame_psnr"])          # the padding pictures of a ragged chunk do not count
        assert u["psnr"] == sum(u["frame_psnr"]) / want and u["bytes"] > 0
        first += want
    assert first == n
    frames = _flat(q, "frame_psnr")
    assert q["ave_all_frame_psnr"] == sum(frames) / n
    assert q["total_trials"] == sum(u["trials"] for u in q["units"])


CASES = [(s, b, inter, n) for s, b in (("yuv420", 10), ("yuv444", 8), ("nv12", 8), ("rgb24", 8)) for inter, n in ((None, 2), ("ld", 4))]
CASES.append(("yuv420", 10, "hts", 16))                               # 1 + 8 + 7: a ragged last chunk
CASES.append(("yuv444", 10, "hts", 16))


@pytest.mark.parametrize("src_type,bits,inter,n", CASES, ids=["%s-%d-%s" % (c[0], c[1], c[2] or "intra") for c in CASES])
def test_the_log_is_the_decoders(tmp_path, src_type, bits, inter, n):
    models = _models(tmp_path, inter)
    src, flags = _source(tmp_path, src_type, bits, n)
    q, d = _encode_and_decode(tmp_path, models, src, flags, n, ["--qp-i", "30", "--qp-p", "38", "--reset-interval", "3"])
    delay = {None: 0, "ld": 1, "hts": 8}[inter]
    _check_log_shape(q, n, delay, src_type, bits)
    assert all(u["trials"] == 0 for u in q["units"]) and [u["qp"] for u in q["units"]] == [30] + [30 if delay == 0 else 38] * (len(q["units"]) - 1)
    keys = ["frame_psnr"] if src_type == "rgb24" else ["frame_psnr" + s for s in SFX]
    for key in keys:
        # the same kernels on the same inputs, a fixed reduction order: equal, not close
        assert _flat(q, key) == d[key], key
        assert len(d[key]) == n
    if src_type == "rgb24":
        assert all("frame_psnr_y" not in u for u in q["units"])


def _sum_bound(n):
    """|dPSNR| of one plane of n samples between two fp64 sums of its n non-negative rounded squares taken in different
    orders: each sum is within (n + 1) 2^-53 of the exact one, relatively (n - 1 additions and the rounding of a term, first
    order), PSNR = 10 log10(peak^2 n / sum), so d PSNR = (10 / ln 10) d sum / sum"""
    return (10 / math.log(10)) * 2 * (n + 1) * 2.0 ** -53


@pytest.mark.parametrize("inter,n", [("ld", 4), ("hts", 16)])
def test_8_bit_yuv420_within_the_bound_of_two_sums(tmp_path, inter, n):
    """the decoder copies fp16 planes to the host and sums there; the encoder sums dcvc_x_to_pix's fp32 planes, which hold
    the same values, on the device"""
    models = _models(tmp_path, inter)
    src = str(tmp_path / "in.yuv")
    _write_yuv(src, H, W, n)
    q, d = _encode_and_decode(tmp_path, models, src, [], n, ["--qp-i", "30", "--qp-p", "38"])
    _check_log_shape(q, n, 1 if inter == "ld" else 8, "yuv420", 8)
    by, bc = _sum_bound(H * W), _sum_bound(H * W // 4)
    worst = 0.0
    for key, bound in (("frame_psnr_y", by), ("frame_psnr_u", bc), ("frame_psnr_v", bc)):
        got, want = _flat(q, key), d[key]
        assert len(got) == len(want) == n
        for a, b in zip(got, want):
            worst = max(worst, abs(a - b) / bound)
            assert abs(a - b) <= bound, (key, a, b, bound)
    # (6 Y + U + V) / 8: the planes' bounds weighted, and the four roundings of the combination on values below 8 x 100 dB
    bf = (6 * by + bc + bc) / 8 + 4 * 800 * 2.0 ** -53
    for a, b in zip(_flat(q, "frame_psnr"), d["frame_psnr"]):
        assert abs(a - b) <= bf, (a, b, bf)
    print("largest |dPSNR| of a plane: %.3f of its bound" % worst)


# ---------------------------------------------------------------- the target against the Python loop
def _x(frames, ids):
    xs = [torch.from_numpy(frame_io.yuv420_to_x(*frames[i])).permute(2, 0, 1)[None].cuda() for i in ids]
    return torch.cat(xs, dim=1).contiguous(memory_format=torch.channels_last)


def _psnr_of_sse(se, n):
    """the tool's psnr_of_sse at peak 255, with the C library's log10 (numpy's differs from it in the last place)"""
    mse = float(se) / n
    p = 10.0 * math.log10(255.0 * 255.0 / mse) if mse > 1e-10 else 999.9
    return p if p < 99.9 else 99.9


def _picture_psnr(frames, idx, x_hat):
    """the tool's measurement of an 8-bit yuv420 picture: dcvc_x_to_pix's fp32 planes against the source's u8 planes, summed
    on the device -> (6 Y + U + V) / 8"""
    y, uv = frames[idx]
    planar = torch.from_numpy(np.concatenate([y.reshape(-1), uv.reshape(-1)])).cuda()
    dist, _ = pixfmt.from_x(x_hat, H, W, pn.YUV420P, 8)
    (sy, sc), (dy, dc) = pixfmt.split_planes(planar, pn.YUV420P, H, W), pixfmt.split_planes(dist, pn.YUV420P, H, W)
    py = _psnr_of_sse(pixfmt.sse(sy, dy)[0], H * W)
    pu, pv = (_psnr_of_sse(v, H * W // 4) for v in pixfmt.sse(sc, dc))
    return (6 * py + pu + pv) / 8


@pytest.mark.parametrize("inter,n,reset_interval", [("ld", 10, 4), ("hts", 16, 32)])
def test_target_equals_the_python_loop(tmp_path, inter, n, reset_interval):
    models = _models(tmp_path, inter)
    mi = dmci_model(skip_thres=0.15)
    mp = dmc_ld_model(skip_thres=0.15) if inter == "ld" else dmc_ht_model(inter, skip_thres=0.15)
    delay = 1 if inter == "ld" else 8
    src = str(tmp_path / "in.yuv")
    frames = _write_yuv(src, H, W, n)
    base = ["encode"] + models + ["-i", src, "-W", str(W), "-H", str(H), "--reset-interval", str(reset_interval)]
    ave = {}
    for qp0 in (16, 48):
        _run(base + ["--qp-i", str(qp0), "-o", str(tmp_path / "c.bin"), "--quality-log", str(tmp_path / "c.json")])
        ave[qp0] = json.loads((tmp_path / "c.json").read_text())["ave_all_frame_psnr"]
    target = (ave[16] + ave[48]) / 2
    print("%s: %.4f dB at q 16, %.4f dB at q 48, target %.4f dB" % (inter, ave[16], ave[48], target))
    binf, qlog, dlog = (str(tmp_path / name) for name in ("out.bin", "q.json", "d.json"))
    r = _run(base + ["--qp-i", "32", "-o", binf, "--target-psnr", repr(float(target)), "--quality-log", qlog])
    print(r.stdout)
    got = json.loads(open(qlog).read())
    _check_log_shape(got, n, delay, "yuv420", 8, target=float(target))

    # the loop of rate_control.py on the plug-in
    i_enc, p_enc = _gpu(mi), _gpu(mp)
    pr, pb = i_enc.get_padding_size(H, W, 16)
    proxy = p_enc._ensure_proxy()
    kept, saved, quality = {}, {}, {}

    def ids_of(idx, count):
        ids = list(range(idx, idx + count))
        return ids + [ids[-1]] * (delay - count)                     # a short chunk repeats its last picture

    def trial_intra(idx, qp):
        enc = i_enc.compress(_x(frames, [idx]), qp, pb, pr)
        kept[(idx, qp)] = enc["bit_stream"]
        quality[(idx, qp)] = [_picture_psnr(frames, idx, enc["x_hat"])]
        return quality[(idx, qp)][0]

    def trial_inter(idx, count, qp, reset, first):
        if first:
            saved["state"] = proxy.export_state().clone()
        else:
            proxy.import_state(saved["state"], H, W)
        enc = p_enc.compress(_x(frames, ids_of(idx, count)), qp, 1 if reset else 0, pb, pr)
        rec = p_enc.reconstruct(H, W)
        rec = [rec] if delay == 1 else rec
        kept[(idx, qp)] = enc["bit_stream"]
        quality[(idx, qp)] = [_picture_psnr(frames, idx + j, rec[j]) for j in range(count)]
        return sum(quality[(idx, qp)]) / count

    def commit(intra, idx, count, qp, reset, last_qp):
        if intra:
            enc = i_enc.compress(_x(frames, [idx]), qp, pb, pr)      # coded again: the bytes of the trial
            p_enc.add_ref_feature_from_frame(enc["x_hat"])
        else:
            if qp != last_qp:
                proxy.import_state(saved["state"], H, W)
                enc = p_enc.compress(_x(frames, ids_of(idx, count)), qp, 1 if reset else 0, pb, pr)
            else:
                enc = {"bit_stream": kept[(idx, qp)]}
        assert enc["bit_stream"] == kept[(idx, qp)], "coding the chosen trial again gives other bytes"
        return enc["bit_stream"]

    want_log = []
    want = rc.code_sequence_quality(n, delay, trial_intra, trial_inter, commit, target, qp_i=32, intra_period=-1,
                                    reset_interval=reset_interval, log=want_log)
    units = got["units"]
    assert [u["type"] for u in units] == ["I" if u[0] else "P" for u in want]
    assert [u["qp"] for u in units] == [u[1] for u in want]
    assert [u["trials"] for u in units] == [e["trials"] for e in want_log]
    assert [u["bytes"] for u in units] == [len(u[3]) for u in want]
    for u, (intra, qp, reset, payload), e in zip(units, want, want_log):
        print("%s unit at %2d: q %2d, %2d trials %s, %.4f dB, %d bytes" % (u["type"], u["first_picture"], qp, u["trials"],
                                                                       [(t[0], round(t[1], 4)) for t in e["trace"]], u["psnr"], u["bytes"]))
    inside = 0
    for u, (intra, qp, reset, payload), e in zip(units, want, want_log):
        idx = u["first_picture"]
        # the same kernels on the same inputs: the same sums; log10 is the host library's in both, to within its last place
        assert u["frame_psnr"] == pytest.approx(quality[(idx, qp)], rel=8 * 2.0 ** -52, abs=0)
        assert 1 <= u["trials"] <= 12
        assert u["psnr"] >= target or qp == 63
        trace = dict(e["trace"])
        if u["psnr"] >= target:
            if qp > 0:                                               # not overshot: one q_index lower was tried and does not meet
                assert qp - 1 in trace and not trace[qp - 1] >= target, (idx, qp, e["trace"])
        else:
            # nothing met: the search's bracket ends above qp_max, which the gallop reached in steps - qp_max - 1 need not be
            # among the trials (rate_control.pick_qp_for_quality; test_quality_search_cpu.py walks the procedure) - and what
            # holds in its place is that qp_max was tried and no trial of the unit meets
            assert 63 in trace and not any(v >= target for v in trace.values()), (idx, qp, e["trace"])
        inside += (not intra) and 0 < qp < 63
    assert inside >= 1, "no P unit landed strictly inside (qp_min, qp_max): the run shows nothing"
    # the unchanged decoder reads the file; every unit's q_index comes from the container
    _run(["decode"] + models + ["-i", binf, "--ref", src, "--json", dlog, "--verbose-json", "1", "-n", str(n)])
    d = json.loads(open(dlog).read())
    by, bc = _sum_bound(H * W), _sum_bound(H * W // 4)
    for key, bound in (("frame_psnr_y", by), ("frame_psnr_u", bc), ("frame_psnr_v", bc)):      # 8-bit yuv420: the host's sums
        assert len(d[key]) == n and all(abs(a - b) <= bound for a, b in zip(_flat(got, key), d[key])), key


# ---------------------------------------------------------------- --scale, and the run without the flags
def test_with_scale_the_log_is_the_prescaled_clips(tmp_path):
    models = _models(tmp_path, "ld")
    pics = _big_pictures(8)
    h, w = 144, 176
    _write_planes(tmp_path / "in.yuv", pics)
    _write_planes(tmp_path / "small.yuv", _scaled(pics, h, w, 8))
    coding = ["--qp-i", "30", "--qp-p", "36"]
    _run(["encode"] + models + coding + ["-i", str(tmp_path / "in.yuv"), "-W", "352", "-H", "288", "--scale", "%dx%d" % (w, h),
                                         "-o", str(tmp_path / "a.bin"), "--quality-log", str(tmp_path / "a.json")])
    _run(["encode"] + models + coding + ["-i", str(tmp_path / "small.yuv"), "-W", str(w), "-H", str(h), "-o", str(tmp_path / "b.bin"),
                                         "--quality-log", str(tmp_path / "b.json")])
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes()
    a = json.loads((tmp_path / "a.json").read_text())
    assert (a["width"], a["height"]) == (w, h) and len(_flat(a, "frame_psnr")) == len(pics)
    assert (tmp_path / "a.json").read_text() == (tmp_path / "b.json").read_text()


@pytest.mark.parametrize("inter,n,coding", [("ld", 6, ["--qp-i", "30", "--qp-p", "40", "--reset-interval", "4"]),
                                            ("hts", 12, ["--qp-i", "30"]),
                                            ("ld", 6, ["--target-bpp", "0.3", "--rc-mode", "probe", "--rc-horizon", "8"])],
                         ids=["ld", "hts", "ld-rate-probe"])
def test_the_quality_log_changes_no_byte(tmp_path, inter, n, coding):
    models = _models(tmp_path, inter)
    src = str(tmp_path / "in.yuv")
    _write_yuv(src, H, W, n)
    base = ["encode"] + models + coding + ["-i", src, "-W", str(W), "-H", str(H)]
    rate = "--target-bpp" in coding
    _run(base + ["-o", str(tmp_path / "a.bin")] + (["--rc-log", str(tmp_path / "a.rc")] if rate else []))
    _run(base + ["-o", str(tmp_path / "b.bin"), "--quality-log", str(tmp_path / "b.json")] + (["--rc-log", str(tmp_path / "b.rc")] if rate else []))
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes()
    if rate:
        assert (tmp_path / "a.rc").read_text() == (tmp_path / "b.rc").read_text()
    q = json.loads((tmp_path / "b.json").read_text())
    assert q["target_psnr"] is None and len(_flat(q, "frame_psnr")) == n
