"""dcvc encode / decode --bit-depth 10 on a real MI355X: uint16 YUV420 pictures -> .bin -> u16 reconstruction + log, against
the SAME sequence driven through the Python plugin surface the way test_video.py:166-399 does it, with the picture I/O of
DCVC-FM's YUVReader / YUVWriter as torch ops (v / max_val on the CPU, then .half() - 0.5; the writer's fp32 planes and their
round) and none of the new C ABI: byte-identical stream, identical u16 file, the PSNR at data range max_val, --calc-ssim, the
log's key set (the 8-bit YUV420 log's), --bit-depth 8 byte-identical to no flag, and the refusals."""
import copy
import io
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import msssim_range_np
import yuv16_np
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, rgb, stream_helper as sh, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
SFX = ("", "_y", "_u", "_v")
YUV_KEYS = ({"arith_policy", "frame_pixel_num", "i_frame_num", "p_frame_num", "test_time"}
            | {"ave_%s_frame_%s%s" % (c, m, s) for c in ("i", "p", "all") for m in ("bpp", "psnr") for s in SFX} - {
                "ave_%s_frame_bpp%s" % (c, s) for c in ("i", "p", "all") for s in SFX[1:]})


def _run(args, check=True):
    return subprocess.run([TOOL] + args, check=check, capture_output=True, text=True, timeout=600)


def _pictures(H, W, n, bits=10, seed=5):
    """(y [H, W], uv [2, H/2, W/2]) uint16 pictures: the synthetic 8-bit sequence scaled to `bits` plus low-order noise"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=seed)
        s = 1 << (bits - 8)
        out.append(tuple((p.astype(np.uint16) * s + rng.integers(0, s, p.shape)).astype(np.uint16) for p in (y, uv)))
    return out


def _write(path, pics):
    with open(path, "wb") as f:
        for y, uv in pics:
            f.write(y.astype("<u2").tobytes())
            f.write(uv.astype("<u2").tobytes())


def _x_of(pics, bits):
    """YUVReader + get_src_frame as torch ops: v / max_val on the CPU (true division), .half() - 0.5, nearest chroma
    -> [1, 3 n, H, W] fp16, channels_last"""
    m = (1 << bits) - 1
    xs = []
    for y, uv in pics:
        yf = torch.from_numpy(y.astype(np.float32)) / m
        uvf = torch.from_numpy(uv.astype(np.float32)) / m
        up = uvf.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        xs.append((torch.cat((yf[None], up), dim=0).half() - 0.5)[None])
    return torch.cat(xs, dim=1).cuda().contiguous(memory_format=torch.channels_last)


def _rec_of(x_hat, H, W, bits):
    """get_distortion before its * 255, then clamp(t * max_val) in fp32 and YUVWriter's round, as torch ops on the GPU
    -> (dist_y, dist_uv fp32 numpy, the u16 picture bytes)"""
    m = float((1 << bits) - 1)
    t = x_hat[0, :, :H, :W] + 0.5
    c = t[1:].float()
    s = ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + c[:, 1::2, 0::2]) + c[:, 1::2, 1::2]
    dy = torch.clamp(t[0].float() * m, 0, m)
    duv = torch.clamp((s * 0.25).half().float() * m, 0, m)
    samples = torch.cat((torch.round(dy).flatten(), torch.round(duv).flatten())).to(torch.int32).cpu().numpy()
    return dy.cpu().numpy(), duv.cpu().numpy(), samples.astype("<u2").tobytes()


def _gpu(m):
    g = copy.deepcopy(m).half().cuda()
    g.proxy = None
    return g


def _python_reference(pics, H, W, bits, i_model, p_model, delay, qp_i, qp_p, reset_interval):
    """test_video.py:204-399 on the plugin surface -> (stream bytes, reconstruction bytes, [psnr list], [(dist_y, dist_uv)])"""
    i_enc, i_dec = _gpu(i_model), _gpu(i_model)
    p_enc = p_dec = None
    if p_model is not None:
        p_enc, p_dec = _gpu(p_model), _gpu(p_model)
    pr, pb = i_enc.get_padding_size(H, W, 16)
    out = io.BytesIO()
    helper = sh.SPSHelper()
    n, idx = len(pics), 0
    while idx < n:
        intra = idx == 0 or p_model is None
        want = 1 if intra else min(delay, n - idx)
        ids = list(range(idx, idx + want))
        while not intra and len(ids) < delay:
            ids.append(ids[-1])
        x = _x_of([pics[i] for i in ids], bits)
        if intra:
            qp, reset = qp_i, 0
            enc = i_enc.compress(x, qp, pb, pr)
            if p_enc is not None:
                p_enc.add_ref_feature_from_frame(enc["x_hat"])
        else:
            qp = qp_p
            reset = 1 if (reset_interval > 0 and (idx + delay) % reset_interval == 1) else 0
            enc = p_enc.compress(x, qp, reset, pb, pr)
        sps_id, new = helper.get_sps_id({"sps_id": -1, "height": H, "width": W})
        if new:
            sh.write_sps(out, {"sps_id": sps_id, "height": H, "width": W})
        sh.write_ip(out, intra, sps_id, qp, enc["ec_parallel"], reset, enc["bit_stream"])
        idx += want
    data = out.getvalue()
    f = io.BytesIO(data)
    helper = sh.SPSHelper()
    rec, psnr, dists = [], [], []
    while len(rec) < n:
        h = sh.read_header(f)
        while h["nal_type"] == sh.NalType.NAL_SPS:
            helper.add_sps_by_id(sh.read_sps_remaining(f, h["sps_id"]))
            h = sh.read_header(f)
        sps = helper.get_sps_by_id(h["sps_id"])
        qp, ec, reset, payload = sh.read_ip_remaining(f)
        if h["nal_type"] == sh.NalType.NAL_I:
            xs = [i_dec.decompress(payload, sps, qp, ec)["x_hat"]]
            if p_dec is not None:
                p_dec.add_ref_feature_from_frame(xs[0], apply_feature_adaptor=False)
        else:
            r = p_dec.decompress(payload, sps, qp, ec, reset)["x_hat"]
            xs = r if isinstance(r, (list, tuple)) else [r]
        for x_hat in xs:
            if len(rec) >= n:
                break
            dy, duv, samples = _rec_of(x_hat, H, W, bits)
            y, uv = pics[len(rec)]
            rec.append(samples)
            dists.append((dy, duv))
            psnr.append(yuv16_np.psnr_yuv420(y, uv, dy, duv, bits))
    return data, b"".join(rec), psnr, dists


def _models(tmp_path, inter):
    mi = dmci_model(skip_thres=0.15)
    mp = None if inter is None else dmc_ld_model(skip_thres=0.15) if inter == "ld" else dmc_ht_model(inter, skip_thres=0.15)
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", mi, 0.15)
    args = ["--intra", str(tmp_path / "i.dcvw")]
    if mp is not None:
        export_weights.write_dcvw(str(tmp_path / "p.dcvw"), inter, mp, 0.15)
        args += ["--inter", str(tmp_path / "p.dcvw")]
    return mi, mp, args


@pytest.mark.parametrize("inter,n", [(None, 2), ("ld", 3), ("hts", 10)])
def test_10_bit_files_equal_the_plugin_path(tmp_path, inter, n):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    H, W, qp_i, qp_p, reset_interval, bits = 96, 128, 30, 36, 4, 10
    pics = _pictures(H, W, n)
    _write(tmp_path / "in.yuv", pics)
    mi, mp, args = _models(tmp_path, inter)
    coding = ["--qp-i", str(qp_i), "--qp-p", str(qp_p), "--reset-interval", str(reset_interval)]
    _run(["encode"] + args + coding + ["--bit-depth", "10", "-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H),
                                       "-o", str(tmp_path / "out.bin")])
    _run(["decode"] + args + ["--bit-depth", "10", "-i", str(tmp_path / "out.bin"), "-o", str(tmp_path / "rec.yuv"),
                              "--ref", str(tmp_path / "in.yuv"), "--json", str(tmp_path / "log.json"), "--verbose-json", "1"])
    delay = 1 if inter in (None, "ld") else 8
    want_bin, want_rec, want_psnr, _ = _python_reference(pics, H, W, bits, mi, mp, delay, qp_i, qp_p, reset_interval)
    assert (tmp_path / "out.bin").read_bytes() == want_bin, "the tool's stream differs from the plugin path's"
    assert (tmp_path / "rec.yuv").read_bytes() == want_rec, "the u16 reconstruction differs"
    log = json.loads((tmp_path / "log.json").read_text())
    verbose = {"frame_bpp", "frame_type"} | {"frame_psnr" + s for s in SFX}
    assert set(log) == YUV_KEYS | verbose, set(log) ^ (YUV_KEYS | verbose)
    n_i = n if inter is None else 1
    assert log["i_frame_num"] == n_i and log["p_frame_num"] == n - n_i
    for k, s in enumerate(SFX):
        for got, want in zip(log["frame_psnr" + s], want_psnr):
            assert got == pytest.approx(want[k], rel=1e-9, abs=0), (s, got, want)
        assert log["ave_all_frame_psnr" + s] == pytest.approx(np.mean([p[k] for p in want_psnr]), rel=1e-8)   # 9 digits
    assert log["ave_all_frame_bpp"] == pytest.approx(8.0 * len(want_bin) / (n * H * W), rel=1e-8)


def test_calc_ssim_at_max_val(tmp_path):
    H, W, bits = 176, 192, 10
    pics = _pictures(H, W, 1, seed=6)
    _write(tmp_path / "in.yuv", pics)
    mi, _, args = _models(tmp_path, None)
    _run(["encode"] + args + ["--bit-depth", "10", "-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "30",
                              "-o", str(tmp_path / "out.bin")])
    _run(["decode"] + args + ["--bit-depth", "10", "-i", str(tmp_path / "out.bin"), "--ref", str(tmp_path / "in.yuv"),
                              "--json", str(tmp_path / "log.json"), "--calc-ssim", "1", "--verbose-json", "1"])
    log = json.loads((tmp_path / "log.json").read_text())
    data, _, psnr, dists = _python_reference(pics, H, W, bits, mi, None, 1, 30, 30, 0)
    assert (tmp_path / "out.bin").read_bytes() == data
    (y, uv), (dy, duv) = pics[0], dists[0]
    want = [msssim_range_np.msssim(y, dy, 1023.0)] + [msssim_range_np.msssim(uv[c], duv[c], 1023.0) for c in range(2)]
    want = [(6 * want[0] + want[1] + want[2]) / 8] + want
    for k, s in enumerate(SFX):
        assert abs(log["frame_msssim" + s][0] - want[k]) <= 1e-10, (s, log["frame_msssim" + s], want[k])
        assert abs(log["ave_all_frame_msssim" + s] - want[k]) <= 1e-10 and log["ave_p_frame_msssim" + s] == 0
        assert log["frame_psnr" + s][0] == pytest.approx(psnr[0][k], rel=1e-9, abs=0)


def test_bit_depth_8_equals_no_flag_and_shares_the_key_set(tmp_path):
    H, W = 96, 128
    _, _, args = _models(tmp_path, None)
    with open(tmp_path / "in8.yuv", "wb") as f:
        for i in range(2):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=2)
            f.write(y.tobytes() + uv.tobytes())
    _write(tmp_path / "in10.yuv", _pictures(H, W, 2, seed=2))
    size = ["-W", str(W), "-H", str(H), "--qp-i", "30"]
    outs = {}
    for name, flag in (("plain", []), ("b8", ["--bit-depth", "8"]), ("b10", ["--bit-depth", "10"])):
        src = tmp_path / ("in10.yuv" if name == "b10" else "in8.yuv")
        _run(["encode"] + args + size + flag + ["-i", str(src), "-o", str(tmp_path / (name + ".bin"))])
        r = _run(["decode"] + args + flag + ["-i", str(tmp_path / (name + ".bin")), "-o", str(tmp_path / (name + ".rec")),
                                             "--ref", str(src), "--json", str(tmp_path / (name + ".json"))])
        log = json.loads((tmp_path / (name + ".json")).read_text())
        log.pop("test_time")
        outs[name] = ((tmp_path / (name + ".bin")).read_bytes(), (tmp_path / (name + ".rec")).read_bytes(), log,
                      r.stdout.split(",")[0])
    assert outs["b8"] == outs["plain"]
    assert set(outs["b10"][2]) == set(outs["plain"][2]) == YUV_KEYS - {"test_time"}
    assert len(outs["b10"][1]) == 2 * len(outs["plain"][1])       # u16 samples


def test_refusals(tmp_path):
    _, _, args = _models(tmp_path, None)
    _write(tmp_path / "in.yuv", _pictures(96, 128, 1))
    rgb.write_png(str(tmp_path / "im1.png"), np.zeros((96, 128, 3), np.uint8))
    base = ["encode"] + args + ["-W", "128", "-H", "96", "-o", str(tmp_path / "o.bin")]
    for extra in (["--src-type", "rgb24", "-i", str(tmp_path / "in.yuv"), "--bit-depth", "10"],
                  ["--src-type", "rgb24", "-i", str(tmp_path / "in.yuv"), "--bit-depth", "8"],
                  ["--src-type", "png", "-i", str(tmp_path), "--bit-depth", "10"]):
        r = _run(base + extra, check=False)
        assert r.returncode != 0 and "--bit-depth is for --src-type yuv420" in r.stderr, r.stderr
    for bad in ("7", "17", "0", "10x", ""):
        r = _run(base + ["-i", str(tmp_path / "in.yuv"), "--bit-depth", bad], check=False)
        assert r.returncode != 0 and "--bit-depth must be 8 or 9..16" in r.stderr, (bad, r.stderr)
    r = _run(["decode"] + args + ["--bit-depth", "4", "-i", str(tmp_path / "in.yuv")], check=False)
    assert r.returncode != 0 and "--bit-depth must be 8 or 9..16" in r.stderr
    assert not (tmp_path / "o.bin").exists()
