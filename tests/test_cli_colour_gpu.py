"""dcvc --matrix / --range / --yuv-depth on a real MI355X: RGB pictures -> .bin -> reconstruction + log, against
the same sequence driven through the Python plugin surface (test_video.py:166-399) with the colour conversions restated in
numpy (tests/colour_np.py) and none of the new C ABI: byte-identical stream, identical RGB24 file and PNG pixels, the RGB
PSNR, the log's keys; bt709 / full against a run without the flags; a 10-bit YUV420 stream decoded to PNG; and the picture
hashes with and without the flags."""
import copy
import io
import json
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import colour_np
from codec_util import dmc_ld_model, dmci_model
from dcvc_amd import export_weights, rgb, stream_helper as sh, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W = 96, 128
RGB_KEYS = ({"arith_policy", "frame_pixel_num", "i_frame_num", "p_frame_num", "test_time"}
            | {"ave_%s_frame_%s" % (c, m) for c in ("i", "p", "all") for m in ("bpp", "psnr")})
COLOUR_KEYS = RGB_KEYS | {"color_matrix", "color_range", "color_yuv_depth"}


def _run(args, check=True):
    return subprocess.run([TOOL] + [str(a) for a in args], check=check, capture_output=True, text=True, timeout=600)


def _pictures(n, seed=11):
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


def _gpu(m):
    g = copy.deepcopy(m).half().cuda()
    g.proxy = None
    return g


def _models(tmp_path, inter):
    mi = dmci_model(skip_thres=0.15)
    mp = dmc_ld_model(skip_thres=0.15) if inter == "ld" else None
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", mi, 0.15)
    args = ["--intra", tmp_path / "i.dcvw"]
    if mp is not None:
        export_weights.write_dcvw(str(tmp_path / "p.dcvw"), inter, mp, 0.15)
        args += ["--inter", tmp_path / "p.dcvw"]
    return mi, mp, args


def _plugin_encode(xs, i_model, p_model, qp_i, qp_p, reset_interval):
    """test_video.py:204-257 on the plugin surface for one-picture units: xs [H, W, 3] fp16 numpy pictures -> stream bytes"""
    i_enc = _gpu(i_model)
    p_enc = _gpu(p_model) if p_model is not None else None
    pr, pb = i_enc.get_padding_size(H, W, 16)
    out = io.BytesIO()
    helper = sh.SPSHelper()
    for idx, xn in enumerate(xs):
        x = torch.from_numpy(xn).cuda().permute(2, 0, 1).unsqueeze(0)          # [1, 3, H, W], channels_last
        intra = idx == 0 or p_model is None
        if intra:
            qp, reset = qp_i, 0
            enc = i_enc.compress(x, qp, pb, pr)
            if p_enc is not None:
                p_enc.add_ref_feature_from_frame(enc["x_hat"])
        else:
            qp = qp_p
            reset = 1 if (reset_interval > 0 and (idx + 1) % reset_interval == 1) else 0
            enc = p_enc.compress(x, qp, reset, pb, pr)
        sps_id, new = helper.get_sps_id({"sps_id": -1, "height": H, "width": W})
        if new:
            sh.write_sps(out, {"sps_id": sps_id, "height": H, "width": W})
        sh.write_ip(out, intra, sps_id, qp, enc["ec_parallel"], reset, enc["bit_stream"])
    return out.getvalue()


def _plugin_decode(data, n, i_model, p_model):
    """test_video.py:259-399 on the plugin surface -> n x_hat pictures [Hp, Wp, 3] fp16 numpy"""
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
        out.append(x_hat[0].permute(1, 2, 0).contiguous().cpu().numpy())
    return out


def _psnr(src, rec16):
    mse = np.mean(np.square(src.astype(np.float64) - rec16.astype(np.float64)))
    return min(10 * np.log10(255.0 * 255.0 / mse), 99.9) if mse > 1e-10 else 99.9


@pytest.mark.parametrize("inter,n", [(None, 2), ("ld", 3)])
def test_bt601_limited_files_equal_the_plugin_path(tmp_path, inter, n):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    qp_i, qp_p, reset_interval = 30, 36, 4
    colour = ["--matrix", "bt601", "--range", "limited"]
    pics = _pictures(n)
    _write_sources(tmp_path, pics)
    mi, mp, args = _models(tmp_path, inter)
    coding = ["--qp-i", qp_i, "--qp-p", qp_p, "--reset-interval", reset_interval]
    _run(["encode"] + args + coding + colour + ["--src-type", "rgb24", "-i", tmp_path / "in.rgb", "-W", W, "-H", H, "-o", tmp_path / "rgb24.bin"])
    _run(["encode"] + args + coding + colour + ["--src-type", "png", "-i", tmp_path / "src", "-o", tmp_path / "png.bin"])
    dec = ["decode"] + args + colour + ["--json"]
    _run(dec + [tmp_path / "rgb24.json", "--src-type", "rgb24", "-i", tmp_path / "rgb24.bin", "-o", tmp_path / "rec.rgb", "--ref", tmp_path / "in.rgb"])
    _run(dec + [tmp_path / "png.json", "--src-type", "png", "-i", tmp_path / "png.bin", "-o", tmp_path / "rec", "--ref", tmp_path / "src"])
    want_bin = _plugin_encode([colour_np.rgb_to_x(p.transpose(2, 0, 1), "bt601", "limited", 8) for p in pics], mi, mp, qp_i, qp_p,
                              reset_interval)
    assert (tmp_path / "rgb24.bin").read_bytes() == want_bin, "the tool's stream differs from the plugin path's"
    assert (tmp_path / "png.bin").read_bytes() == want_bin
    recs = [colour_np.x_to_rgb(xh, H, W, "bt601", "limited", 8) for xh in _plugin_decode(want_bin, n, mi, mp)]
    assert (tmp_path / "rec.rgb").read_bytes() == b"".join(r8.tobytes() for _, r8 in recs), "RGB24 reconstruction differs"
    names = sorted(os.listdir(tmp_path / "rec"))
    assert names == ["im%05d.png" % (i + 1) for i in range(n)]
    for name, (_, r8) in zip(names, recs):
        assert np.array_equal(rgb.read_png(str(tmp_path / "rec" / name)), r8), name
    want_psnr = [_psnr(p.transpose(2, 0, 1), r16) for p, (r16, _) in zip(pics, recs)]
    n_i = n if inter is None else 1
    for log_name in ("rgb24.json", "png.json"):
        log = json.loads((tmp_path / log_name).read_text())
        assert set(log) == COLOUR_KEYS, set(log) ^ COLOUR_KEYS
        assert (log["color_matrix"], log["color_range"], log["color_yuv_depth"]) == ("bt601", "limited", 8)
        assert log["i_frame_num"] == n_i and log["p_frame_num"] == n - n_i
        print("ave_all_frame_psnr %.17g, restated %.17g" % (log["ave_all_frame_psnr"], float(np.mean(want_psnr))))
        assert abs(log["ave_all_frame_psnr"] - float(np.mean(want_psnr))) <= 1e-9


def test_bt709_full_is_a_run_without_the_flags(tmp_path):
    pics = _pictures(2)
    _write_sources(tmp_path, pics)
    _, _, args = _models(tmp_path, None)
    logs = {}
    for tag, colour in (("plain", []), ("flags", ["--matrix", "bt709", "--range", "full"])):
        _run(["encode"] + args + colour + ["--qp-i", 30, "--src-type", "rgb24", "-i", tmp_path / "in.rgb", "-W", W, "-H", H,
                                           "-o", tmp_path / (tag + ".bin")])
        _run(["decode"] + args + colour + ["--src-type", "rgb24", "-i", tmp_path / (tag + ".bin"), "-o", tmp_path / (tag + ".rgb"),
                                           "--ref", tmp_path / "in.rgb", "--json", tmp_path / (tag + ".json")])
        logs[tag] = json.loads((tmp_path / (tag + ".json")).read_text())
    assert (tmp_path / "flags.bin").read_bytes() == (tmp_path / "plain.bin").read_bytes()
    assert (tmp_path / "flags.rgb").read_bytes() == (tmp_path / "plain.rgb").read_bytes()
    assert set(logs["plain"]) == RGB_KEYS, set(logs["plain"]) ^ RGB_KEYS
    assert set(logs["flags"]) == COLOUR_KEYS, set(logs["flags"]) ^ COLOUR_KEYS
    assert (logs["flags"]["color_matrix"], logs["flags"]["color_range"], logs["flags"]["color_yuv_depth"]) == ("bt709", "full", 8)
    for k in RGB_KEYS - {"test_time"}:
        assert logs["flags"][k] == logs["plain"][k], k


def test_a_10_bit_yuv420_stream_decodes_to_png_with_bt2020_limited(tmp_path):
    rng = np.random.default_rng(5)
    n = 2
    with open(tmp_path / "in.yuv", "wb") as f:
        for i in range(n):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=5)
            for p, lo, hi in ((y, 64, 940), (uv, 64, 960)):                  # a limited-range 10-bit clip
                v = lo + (p.astype(np.float64) / 255.0) * (hi - lo) + rng.integers(0, 2, p.shape)
                f.write(np.clip(np.rint(v), lo, hi).astype("<u2").tobytes())
    mi, _, args = _models(tmp_path, None)
    _run(["encode"] + args + ["--qp-i", 40, "--bit-depth", 10, "-i", tmp_path / "in.yuv", "-W", W, "-H", H, "-o", tmp_path / "out.bin"])
    colour = ["--matrix", "bt2020", "--range", "limited", "--yuv-depth", 10]
    _run(["decode"] + args + colour + ["--src-type", "png", "-i", tmp_path / "out.bin", "-o", tmp_path / "rec"])
    _run(["decode"] + args + ["--src-type", "png", "-i", tmp_path / "out.bin", "-o", tmp_path / "plain"])
    x_hats = _plugin_decode((tmp_path / "out.bin").read_bytes(), n, mi, None)
    differs = False
    for i, xh in enumerate(x_hats):
        name = "im%05d.png" % (i + 1)
        got = rgb.read_png(str(tmp_path / "rec" / name))
        assert np.array_equal(got, colour_np.x_to_rgb(xh, H, W, "bt2020", "limited", 10)[1]), name
        differs = differs or not np.array_equal(got, rgb.read_png(str(tmp_path / "plain" / name)))
    assert differs


def test_hashes_follow_the_flags(tmp_path):
    pics = _pictures(2)
    _write_sources(tmp_path, pics)
    _, _, args = _models(tmp_path, None)
    colour = ["--matrix", "bt601", "--range", "limited"]
    _run(["encode"] + args + colour + ["--qp-i", 30, "--src-type", "rgb24", "-i", tmp_path / "in.rgb", "-W", W, "-H", H,
                                       "-o", tmp_path / "out.bin", "--hash-log", tmp_path / "enc.txt"])
    dec = ["decode"] + args + ["--src-type", "rgb24", "-i", tmp_path / "out.bin"]
    _run(dec + colour + ["-o", tmp_path / "rec.rgb", "--hash-log", tmp_path / "m.txt"])
    data = (tmp_path / "rec.rgb").read_bytes()
    lines = (tmp_path / "m.txt").read_text().splitlines()
    assert lines[0] == "# dcvc-hash 1 crc32 rgb24 8 %d %d" % (W, H)
    assert lines[-1] == "sequence %08x %d" % (zlib.crc32(data), len(data))
    assert (tmp_path / "enc.txt").read_bytes() == (tmp_path / "m.txt").read_bytes()      # encode --hash-log, all-intra
    r = _run(dec + colour + ["--verify-hash", tmp_path / "m.txt"], check=False)
    assert r.returncode == 0 and "verified 2 pictures" in r.stdout, r.stderr
    r = _run(dec + ["--verify-hash", tmp_path / "m.txt"], check=False)
    assert r.returncode == 3, (r.returncode, r.stderr)
