"""dcvc encode / decode --src-type rgb24 | png on a real MI355X: RGB pictures -> .bin -> reconstruction + log, against the
SAME sequence driven through the Python plugin surface the way test_video.py:166-399 does it for src_type 'png', with the
colour conversions as torch ops on the GPU (test_video.py:55-64, 87-122, 366-370; transforms.py:17-27, 53-66) and none of
the new C ABI: byte-identical stream, identical RGB24 file and PNG pixels, the RGB PSNR, the log's key set (no _y / _u / _v),
--calc-ssim against metrics.msssim_rgb, and the refusal of odd sizes, mismatched PNG sizes and unknown PNG names."""
import copy
import io
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, metrics, rgb, stream_helper as sh, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
KR, KG, KB = 0.2126, 0.7152, 0.0722
RGB_KEYS = ({"arith_policy", "frame_pixel_num", "i_frame_num", "p_frame_num", "test_time"}
            | {"ave_%s_frame_%s" % (c, m) for c in ("i", "p", "all") for m in ("bpp", "psnr")})
SSIM_KEYS = RGB_KEYS | {"ave_%s_frame_msssim" % c for c in ("i", "p", "all")} | {"frame_bpp", "frame_type", "frame_psnr",
                                                                                  "frame_msssim"}


def _run(args, check=True):
    return subprocess.run([TOOL] + args, check=check, capture_output=True, text=True, timeout=600)


def _pictures(H, W, n, seed=11):
    """[H, W, 3] u8 RGB pictures: a panning smooth picture in three differently mixed channels"""
    out = []
    for i in range(n):
        y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=seed)
        up = np.repeat(np.repeat(uv.astype(np.int32) - 128, 2, axis=1), 2, axis=2)
        y = y.astype(np.int32)
        out.append(np.clip(np.stack([y + 2 * up[1], y - up[0] - up[1], y + 2 * up[0]], axis=-1), 0, 255).astype(np.uint8))
    return out


def _write_sources(tmp_path, pics):
    with open(tmp_path / "in.rgb", "wb") as f:
        for p in pics:
            f.write(p.tobytes())
    (tmp_path / "src").mkdir()
    for i, p in enumerate(pics):
        rgb.write_png(str(tmp_path / "src" / ("im%05d.png" % (i + 1))), p)


def _x_of(pics):
    """get_src_frame's png branch as torch ops on the GPU: [1, 3 n, H, W] fp16, channels_last"""
    xs = []
    for p in pics:
        x = torch.from_numpy(p).permute(2, 0, 1).unsqueeze(0).cuda().float() / 255.0
        r, g, b = x.chunk(3, -3)
        y = KR * r + KG * g + KB * b
        cb = 0.5 * (b - y) / (1 - KB) + 0.5
        cr = 0.5 * (r - y) / (1 - KR) + 0.5
        xs.append(torch.clamp(torch.cat((y, cb, cr), dim=-3), 0., 1.))
    return (torch.cat(xs, dim=1).half() - 0.5).contiguous(memory_format=torch.channels_last)


def _rec_of(x_hat, H, W):
    """get_distortion's png branch and the writer as torch ops on the GPU -> (rgb16 [3, H, W] fp16, rgb8 [H, W, 3] u8)"""
    t = x_hat[:, :, :H, :W] + 0.5
    y, cb, cr = t.float().chunk(3, -3)
    r = y + (2 - 2 * KR) * (cr - 0.5)
    b = y + (2 - 2 * KB) * (cb - 0.5)
    g = (y - KR * r - KB * b) / KG
    rec16 = torch.clamp(torch.clamp(torch.cat((r, g, b), dim=-3), 0., 1.).half() * 255, 0, 255)
    return rec16[0], rec16.round().byte()[0].permute(1, 2, 0)


def _psnr(src, rec16):
    mse = np.mean(np.square(src.astype(np.float64) - rec16.astype(np.float64)))
    return min(10 * np.log10(255.0 * 255.0 / mse), 99.9) if mse > 1e-10 else 99.9


def _gpu(m):
    g = copy.deepcopy(m).half().cuda()
    g.proxy = None
    return g


def _python_reference(pics, H, W, i_model, p_model, delay, qp_i, qp_p, reset_interval):
    """test_video.py:204-399 with src_type 'png' on the plugin surface -> (stream bytes, [rgb8], [rgb16], [psnr])"""
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
        x = _x_of([pics[i] for i in ids])
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
    rec8, rec16, psnr = [], [], []
    while len(rec8) < n:
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
            if len(rec8) >= n:
                break
            r16, r8 = _rec_of(x_hat, H, W)
            rec16.append(r16)
            rec8.append(r8.cpu().numpy())
            psnr.append(_psnr(pics[len(psnr)].transpose(2, 0, 1), r16.cpu().numpy()))
    return data, rec8, rec16, psnr


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
def test_rgb24_and_png_files_equal_the_plugin_path(tmp_path, inter, n):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    H, W, qp_i, qp_p, reset_interval = 96, 128, 30, 36, 4
    pics = _pictures(H, W, n)
    _write_sources(tmp_path, pics)
    mi, mp, args = _models(tmp_path, inter)
    coding = ["--qp-i", str(qp_i), "--qp-p", str(qp_p), "--reset-interval", str(reset_interval)]
    _run(["encode"] + args + coding + ["--src-type", "rgb24", "-i", str(tmp_path / "in.rgb"), "-W", str(W), "-H", str(H),
                                       "-o", str(tmp_path / "rgb24.bin")])
    _run(["encode"] + args + coding + ["--src-type", "png", "-i", str(tmp_path / "src"), "-o", str(tmp_path / "png.bin")])
    dec = ["decode"] + args + ["--json"]
    _run(dec + [str(tmp_path / "rgb24.json"), "--src-type", "rgb24", "-i", str(tmp_path / "rgb24.bin"),
                "-o", str(tmp_path / "rec.rgb"), "--ref", str(tmp_path / "in.rgb")])
    _run(dec + [str(tmp_path / "png.json"), "--src-type", "png", "-i", str(tmp_path / "png.bin"),
                "-o", str(tmp_path / "rec"), "--ref", str(tmp_path / "src")])
    delay = 1 if inter in (None, "ld") else 8
    want_bin, want_rec, _, want_psnr = _python_reference(pics, H, W, mi, mp, delay, qp_i, qp_p, reset_interval)
    assert (tmp_path / "rgb24.bin").read_bytes() == want_bin, "the tool's stream differs from the plugin path's"
    assert (tmp_path / "png.bin").read_bytes() == want_bin
    assert (tmp_path / "rec.rgb").read_bytes() == b"".join(r.tobytes() for r in want_rec), "RGB24 reconstruction differs"
    names = sorted(os.listdir(tmp_path / "rec"))
    assert names == ["im%05d.png" % (i + 1) for i in range(n)]
    for name, want in zip(names, want_rec):
        assert np.array_equal(rgb.read_png(str(tmp_path / "rec" / name)), want), name
    n_i = n if inter is None else 1
    for log_name in ("rgb24.json", "png.json"):
        log = json.loads((tmp_path / log_name).read_text())
        assert set(log) == RGB_KEYS, set(log) ^ RGB_KEYS
        assert log["i_frame_num"] == n_i and log["p_frame_num"] == n - n_i
        assert abs(log["ave_all_frame_psnr"] - float(np.mean(want_psnr))) <= 1e-9
        assert log["ave_all_frame_bpp"] == pytest.approx(8.0 * len(want_bin) / (n * H * W), rel=1e-8)   # written with 9 digits


def test_calc_ssim_matches_msssim_rgb(tmp_path):
    H, W = 192, 256
    pics = _pictures(H, W, 1, seed=4)
    _write_sources(tmp_path, pics)
    mi, _, args = _models(tmp_path, None)
    _run(["encode"] + args + ["--src-type", "rgb24", "-i", str(tmp_path / "in.rgb"), "-W", str(W), "-H", str(H), "--qp-i", "30",
                              "-o", str(tmp_path / "out.bin")])
    _run(["decode"] + args + ["--src-type", "rgb24", "-i", str(tmp_path / "out.bin"), "--ref", str(tmp_path / "in.rgb"),
                              "--json", str(tmp_path / "log.json"), "--calc-ssim", "1", "--verbose-json", "1"])
    log = json.loads((tmp_path / "log.json").read_text())
    assert set(log) == SSIM_KEYS, set(log) ^ SSIM_KEYS
    data, _, rec16, psnr = _python_reference(pics, H, W, mi, None, 1, 30, 30, 0)
    assert (tmp_path / "out.bin").read_bytes() == data
    want = metrics.msssim_rgb(torch.from_numpy(pics[0]).permute(2, 0, 1).contiguous().cuda(), rec16[0])
    assert abs(log["frame_msssim"][0] - want) <= 1e-10
    assert abs(log["ave_all_frame_msssim"] - want) <= 1e-10 and log["ave_p_frame_msssim"] == 0
    assert abs(log["frame_psnr"][0] - psnr[0]) <= 1e-9 and log["frame_type"] == [0]


def test_refusals(tmp_path):
    _, _, args = _models(tmp_path, None)
    # odd sides
    (tmp_path / "odd.rgb").write_bytes(bytes(95 * 128 * 3))
    r = _run(["encode"] + args + ["--src-type", "rgb24", "-i", str(tmp_path / "odd.rgb"), "-W", "128", "-H", "95",
                                  "-o", str(tmp_path / "o.bin")], check=False)
    assert r.returncode != 0 and "even" in r.stderr and "128x95" in r.stderr
    odd = tmp_path / "odd"
    odd.mkdir()
    rgb.write_png(str(odd / "im1.png"), np.zeros((96, 127, 3), np.uint8))
    r = _run(["encode"] + args + ["--src-type", "png", "-i", str(odd), "-o", str(tmp_path / "o.bin")], check=False)
    assert r.returncode != 0 and "even" in r.stderr
    # a picture whose size differs from the first one's, and -W / -H that disagree with the first picture
    mixed = tmp_path / "mixed"
    mixed.mkdir()
    rgb.write_png(str(mixed / "im00001.png"), np.zeros((96, 128, 3), np.uint8))
    rgb.write_png(str(mixed / "im00002.png"), np.zeros((96, 130, 3), np.uint8))
    r = _run(["encode"] + args + ["--src-type", "png", "-i", str(mixed), "-o", str(tmp_path / "o.bin")], check=False)
    assert r.returncode != 0 and "im00002.png is 130x96" in r.stderr
    r = _run(["encode"] + args + ["--src-type", "png", "-i", str(mixed), "-W", "64", "-o", str(tmp_path / "o.bin")], check=False)
    assert r.returncode != 0 and "not the -W x -H" in r.stderr
    # unknown naming scheme
    other = tmp_path / "other"
    other.mkdir()
    rgb.write_png(str(other / "frame0001.png"), np.zeros((96, 128, 3), np.uint8))
    r = _run(["encode"] + args + ["--src-type", "png", "-i", str(other), "-o", str(tmp_path / "o.bin")], check=False)
    assert r.returncode != 0 and "naming convention" in r.stderr
    # rgb24 without a size, an unknown source type
    r = _run(["encode"] + args + ["--src-type", "rgb24", "-i", str(tmp_path / "odd.rgb"), "-o", str(tmp_path / "o.bin")], check=False)
    assert r.returncode != 0 and "-W and -H" in r.stderr
    r = _run(["encode"] + args + ["--src-type", "bgr", "-i", str(tmp_path / "odd.rgb"), "-W", "128", "-H", "96",
                                  "-o", str(tmp_path / "o.bin")], check=False)
    assert r.returncode != 0 and "unknown --src-type" in r.stderr
    # --calc-ssim below 88 is refused before anything is decoded
    (tmp_path / "small.rgb").write_bytes(bytes(64 * 128 * 3))
    _run(["encode"] + args + ["--src-type", "rgb24", "-i", str(tmp_path / "small.rgb"), "-W", "128", "-H", "64",
                              "-o", str(tmp_path / "s.bin")])
    r = _run(["decode"] + args + ["--src-type", "rgb24", "-i", str(tmp_path / "s.bin"), "--ref", str(tmp_path / "small.rgb"),
                                  "--json", str(tmp_path / "s.json"), "--calc-ssim", "1"], check=False)
    assert r.returncode != 0 and "88" in r.stderr and "decoded" not in r.stdout
    assert not (tmp_path / "s.json").exists()
