"""dcvc decode --calc-ssim / --verbose-json on a real MI355X: the per-picture MS-SSIM of the tool's log against the fp64
numpy restatement (tests/msssim_np.py) on the plugin path's distortion planes, the averages and key set of the reference's
log (src/utils/common.py:46-116 generate_log_json with calc_ssim and verbose_json), the log without the flags as it was,
and the refusal of pictures whose chroma planes are below MS-SSIM's minimum of 88."""
import copy
import ctypes
import io
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import msssim_np
from codec_util import dmc_ld_model, dmci_model
from dcvc_amd import _lib, export_weights, stream_helper as sh, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
vp, ci = ctypes.c_void_p, ctypes.c_int
SFX = ["", "_y", "_u", "_v"]
# the keys the tool wrote before --calc-ssim / --verbose-json existed ("arith_policy" is the tool's own)
PLAIN_KEYS = ({"arith_policy", "frame_pixel_num", "i_frame_num", "p_frame_num", "test_time"}
              | {"ave_%s_frame_bpp" % c for c in ("i", "p", "all")}
              | {"ave_%s_frame_psnr%s" % (c, s) for c in ("i", "p", "all") for s in SFX})
# generate_log_json with include_yuv, calc_ssim and verbose (plus "arith_policy")
FULL_KEYS = (PLAIN_KEYS | {"ave_%s_frame_msssim%s" % (c, s) for c in ("i", "p", "all") for s in SFX}
             | {"frame_bpp", "frame_type"} | {"frame_%s%s" % (m, s) for m in ("psnr", "msssim") for s in SFX})


def _run(args, check=True):
    return subprocess.run([TOOL] + args, check=check, capture_output=True, text=True, timeout=600)


def _write_yuv(path, H, W, n):
    frames = []
    with open(path, "wb") as f:
        for i in range(n):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=7)
            f.write(y.tobytes())
            f.write(uv.tobytes())
            frames.append((y, uv))
    return frames


def _gpu(m):
    g = copy.deepcopy(m).half().cuda()
    g.proxy = None
    return g


def _planes(x_hat, H, W):
    fn = _lib.fn("dcvc_x_to_yuv420", ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp])
    xh = x_hat[0].permute(1, 2, 0).contiguous()
    y16 = torch.empty((H, W), dtype=torch.float16, device="cuda")
    uv16 = torch.empty((2, H // 2, W // 2), dtype=torch.float16, device="cuda")
    _lib.check(fn(vp(xh.data_ptr()), xh.shape[1], H, W, vp(y16.data_ptr()), vp(uv16.data_ptr()), None, None,
                  vp(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return y16.cpu().numpy(), uv16.cpu().numpy()


def _plugin_decode(data, n, i_model, p_model):
    """the tool's stream decoded through the plugin surface (test_video.py:300-363) -> fp16 distortion planes per picture"""
    i_dec = _gpu(i_model)
    p_dec = _gpu(p_model) if p_model is not None else None
    f = io.BytesIO(data)
    helper = sh.SPSHelper()
    out = []
    while len(out) < n:
        h = sh.read_header(f)
        while h["nal_type"] == sh.NalType.NAL_SPS:
            helper.add_sps_by_id(sh.read_sps_remaining(f, h["sps_id"]))
            h = sh.read_header(f)
        sps = helper.get_sps_by_id(h["sps_id"])
        qp, ec, reset, payload = sh.read_ip_remaining(f)
        if h["nal_type"] == sh.NalType.NAL_I:
            x_hat = i_dec.decompress(payload, sps, qp, ec)["x_hat"]
            if p_dec is not None:
                p_dec.add_ref_feature_from_frame(x_hat, apply_feature_adaptor=False)
        else:
            x_hat = p_dec.decompress(payload, sps, qp, ec, reset)["x_hat"]
            x_hat = x_hat[0] if isinstance(x_hat, (list, tuple)) else x_hat
        out.append(_planes(x_hat, sps["height"], sps["width"]))
    return out


def _encode(tmp_path, H, W, n, inter):
    frames = _write_yuv(str(tmp_path / "in.yuv"), H, W, n)
    mi = dmci_model(skip_thres=0.15)
    mp = dmc_ld_model(skip_thres=0.15) if inter else None
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", mi, 0.15)
    args = ["--intra", str(tmp_path / "i.dcvw")]
    if mp is not None:
        export_weights.write_dcvw(str(tmp_path / "p.dcvw"), "ld", mp, 0.15)
        args += ["--inter", str(tmp_path / "p.dcvw")]
    _run(["encode"] + args + ["-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "30", "--qp-p", "36",
                              "--reset-interval", "2", "-o", str(tmp_path / "out.bin")])
    return frames, args, mi, mp


@pytest.mark.parametrize("inter,n", [(False, 2), (True, 4)])
def test_decode_logs_msssim_of_every_picture(tmp_path, inter, n):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    H, W = 240, 416          # luma: 5 levels; chroma 120 x 208: 4 levels
    frames, args, mi, mp = _encode(tmp_path, H, W, n, inter)
    dec = ["decode"] + args + ["-i", str(tmp_path / "out.bin"), "--ref", str(tmp_path / "in.yuv")]
    _run(dec + ["--json", str(tmp_path / "full.json"), "--calc-ssim", "1", "--verbose-json", "1"])
    _run(dec + ["--json", str(tmp_path / "plain.json")])
    log = json.loads((tmp_path / "full.json").read_text())
    plain = json.loads((tmp_path / "plain.json").read_text())
    assert set(log) == FULL_KEYS
    assert set(plain) == PLAIN_KEYS
    for k in PLAIN_KEYS - {"test_time"}:
        assert plain[k] == log[k], k

    planes = _plugin_decode((tmp_path / "out.bin").read_bytes(), n, mi, mp)
    types = [0] + [1 if inter else 0] * (n - 1)
    assert log["frame_type"] == types
    for i, ((y, uv), (y16, uv16)) in enumerate(zip(frames, planes)):
        want = [msssim_np.msssim(y, y16), msssim_np.msssim(uv[0], uv16[0]), msssim_np.msssim(uv[1], uv16[1])]
        got = [log["frame_msssim_y"][i], log["frame_msssim_u"][i], log["frame_msssim_v"][i]]
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-10, (i, got, want)
        assert log["frame_msssim"][i] == (6 * got[0] + got[1] + got[2]) / 8
    for s in SFX:
        per = np.array(log["frame_msssim" + s])
        per_i, per_p = per[np.array(types) == 0], per[np.array(types) == 1]
        assert log["ave_i_frame_msssim" + s] == pytest.approx(per_i.mean(), abs=1e-15)
        assert log["ave_p_frame_msssim" + s] == (pytest.approx(per_p.mean(), abs=1e-15) if len(per_p) else 0)
        assert log["ave_all_frame_msssim" + s] == pytest.approx(per.mean(), abs=1e-15)
        assert log["ave_all_frame_psnr" + s] == pytest.approx(np.mean(log["frame_psnr" + s]), abs=1e-6)
    assert sum(log["frame_bpp"]) * H * W == pytest.approx(8.0 * (tmp_path / "out.bin").stat().st_size, rel=1e-12)
    # what BD-rate reads for --distortion_metrics msssim msssim_y
    from dcvc_amd import bd_rate
    assert not any(math.isnan(log["ave_all_frame_msssim" + s]) for s in SFX)
    assert bd_rate.curves({"seq": {"q": log}}, metric="msssim")["seq"][1][0] == log["ave_all_frame_msssim"]


def test_small_pictures_are_refused_before_decoding(tmp_path):
    H, W = 96, 128
    _, args, _, _ = _encode(tmp_path, H, W, 1, False)
    r = _run(["decode"] + args + ["-i", str(tmp_path / "out.bin"), "--ref", str(tmp_path / "in.yuv"),
                                  "--json", str(tmp_path / "log.json"), "--calc-ssim", "1"], check=False)
    assert r.returncode != 0
    assert "176" in r.stderr and "decoded" not in r.stdout
    assert not (tmp_path / "log.json").exists()
