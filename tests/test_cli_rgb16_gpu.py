"""dcvc encode / decode --src-type rgb48 | png16 on a real MI355X: 9..16-bit RGB pictures -> .bin -> reconstruction + log, against
the SAME sequence driven through the Python plug-in surface (rgb.rgb16_to_x -> DMCIProxy.compress / DMCLDProxy.compress,
wrapped by stream_helper; rgb.x_to_rgb16 of the plug-in's decode): byte-identical stream, identical rgb48 file and PNG pixels,
the log's PSNR and MS-SSIM against the Python wrappers (==) and against an independent numpy sum, the rgb24 log's key set,
--hash-log / --verify-hash, --quality-log, and a BT.2020 limited-range 10-bit YUV stream decoded to 16-bit PNG against the
numpy restatement. Seeded synthetic weights, 3 pictures of 88x88 - the smallest size --calc-ssim accepts for RGB."""
import copy
import io
import json
import math
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import rgb16_np
from codec_util import dmc_ld_model, dmci_model
from dcvc_amd import export_weights, picture_hash, rgb, stream_helper as sh, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 88, 88, 3
QP_I, QP_P, RESET = 30, 36, 4
RGB_KEYS = ({"arith_policy", "frame_pixel_num", "i_frame_num", "p_frame_num", "test_time"}
            | {"ave_%s_frame_%s" % (c, m) for c in ("i", "p", "all") for m in ("bpp", "psnr")})
SSIM_KEYS = RGB_KEYS | {"ave_%s_frame_msssim" % c for c in ("i", "p", "all")} | {"frame_bpp", "frame_type", "frame_psnr",
                                                                                  "frame_msssim"}


def _run(args, check=True):
    return subprocess.run([TOOL] + args, check=check, capture_output=True, text=True, timeout=600)


def _pictures(depth, seed=11):
    """[H, W, 3] u16 RGB pictures at `depth` bits: a panning smooth picture in three differently mixed channels plus low-order noise"""
    rng = np.random.default_rng(seed + depth)
    s = 1 << (depth - 8)
    out = []
    for i in range(N):
        y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=seed)
        up = np.repeat(np.repeat(uv.astype(np.int32) - 128, 2, axis=1), 2, axis=2)
        y = y.astype(np.int32)
        p8 = np.clip(np.stack([y + 2 * up[1], y - up[0] - up[1], y + 2 * up[0]], axis=-1), 0, 255)
        out.append((p8 * s + rng.integers(0, s, p8.shape)).astype(np.uint16))
    return out


def _dev(p):
    return torch.from_numpy(p.view(np.int16)).cuda()


def _gpu(m):
    g = copy.deepcopy(m).half().cuda()
    g.proxy = None
    return g


def _plugin(xs, i_model, p_model):
    """test_video.py:204-399 on the plug-in surface over the model inputs xs ([1, 3, H, W] fp16, channels_last) -> (stream
    bytes, [x_hat [1, 3, Hp, Wp]])"""
    i_enc, i_dec = _gpu(i_model), _gpu(i_model)
    p_enc = p_dec = None
    if p_model is not None:
        p_enc, p_dec = _gpu(p_model), _gpu(p_model)
    pr, pb = i_enc.get_padding_size(H, W, 16)
    out = io.BytesIO()
    helper = sh.SPSHelper()
    for idx, x in enumerate(xs):
        intra = idx == 0 or p_model is None
        if intra:
            qp, reset = QP_I, 0
            enc = i_enc.compress(x, qp, pb, pr)
            if p_enc is not None:
                p_enc.add_ref_feature_from_frame(enc["x_hat"])
        else:
            qp = QP_P
            reset = 1 if (idx + 1) % RESET == 1 else 0
            enc = p_enc.compress(x, qp, reset, pb, pr)
        sps_id, new = helper.get_sps_id({"sps_id": -1, "height": H, "width": W})
        if new:
            sh.write_sps(out, {"sps_id": sps_id, "height": H, "width": W})
        sh.write_ip(out, intra, sps_id, qp, enc["ec_parallel"], reset, enc["bit_stream"])
    data = out.getvalue()
    return data, _plugin_decode(data, len(xs), i_dec, p_dec)


def _plugin_decode(data, n, i_dec, p_dec):
    f = io.BytesIO(data)
    helper = sh.SPSHelper()
    x_hats = []
    while len(x_hats) < n:
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
        x_hats.append(x_hat.clone())
    return x_hats


def _x_of(p, depth, **colour):
    return rgb.rgb16_to_x(_dev(p), depth, **colour).permute(2, 0, 1).unsqueeze(0).contiguous(memory_format=torch.channels_last)


def _host16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("rgb16_models")
    mi, mp = dmci_model(skip_thres=0.15), dmc_ld_model(skip_thres=0.15)
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", mi, 0.15)
    export_weights.write_dcvw(str(d / "p.dcvw"), "ld", mp, 0.15)
    return mi, mp, ["--intra", str(d / "i.dcvw")], ["--inter", str(d / "p.dcvw")]


def _write_rgb48(path, pics):
    with open(path, "wb") as f:
        for p in pics:
            f.write(p.astype("<u2").tobytes())


def _psnr_c(se, n, peak):
    """the tool's psnr_of_sse with the C library's log10"""
    mse = float(se) / n
    p = 10.0 * math.log10(peak * peak / mse) if mse > 1e-10 else 999.9
    return p if p < 99.9 else 99.9


@pytest.mark.parametrize("depth", [10, 16])
def test_rgb48_all_intra_equals_the_plugin_path(tmp_path, models, depth):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    mi, _, intra, _ = models
    pics = _pictures(depth)
    peak = (1 << depth) - 1
    _write_rgb48(tmp_path / "in.rgb48", pics)
    src = ["--src-type", "rgb48", "--bit-depth", str(depth)]
    _run(["encode"] + intra + src + ["-i", str(tmp_path / "in.rgb48"), "-W", str(W), "-H", str(H), "--qp-i", str(QP_I), "-o", str(tmp_path / "out.bin"),
                                     "--hash-log", str(tmp_path / "enc.hash"), "--quality-log", str(tmp_path / "quality.json")])
    _run(["decode"] + intra + src + ["-i", str(tmp_path / "out.bin"), "-o", str(tmp_path / "rec.rgb48"), "--ref", str(tmp_path / "in.rgb48"),
                                     "--json", str(tmp_path / "log.json"), "--calc-ssim", "1", "--verbose-json", "1",
                                     "--hash-log", str(tmp_path / "dec.hash")])
    want_bin, x_hats = _plugin([_x_of(p, depth) for p in pics], mi, None)
    assert (tmp_path / "out.bin").read_bytes() == want_bin, "the tool's stream differs from the plug-in path's"
    rec = (tmp_path / "rec.rgb48").read_bytes()
    assert len(rec) == N * 6 * H * W
    log = json.loads((tmp_path / "log.json").read_text())
    assert set(log) == SSIM_KEYS, set(log) ^ SSIM_KEYS
    assert log["i_frame_num"] == N and log["p_frame_num"] == 0 and log["frame_type"] == [0] * N
    for i, (p, x_hat) in enumerate(zip(pics, x_hats)):
        dist, out = rgb.x_to_rgb16(x_hat, H, W, depth)
        assert rec[i * 6 * H * W:(i + 1) * 6 * H * W] == _host16(out).astype("<u2").tobytes(), "picture %d of -o differs" % i
        # the log against the Python wrappers, which make the same device calls on the same operands
        _, planar = rgb.rgb16_to_x(_dev(p), depth, planar=True)
        assert log["frame_psnr"][i] == rgb.psnr_rgb16(planar, dist, depth), i
        assert log["frame_msssim"][i] == rgb.msssim_rgb16(planar, dist, depth), i
        # ... and against an independent fp64 sum over dist32 on the host: the two sums of n = 3 H W non-negative terms differ
        # by their order alone, at most 2 (n + 1) 2^-53 relative, which the logarithm turns into
        # (10 / ln 10) 2 (n + 1) 2^-53 dB; the division and the logarithm themselves add a few ulps of the result
        d = p.transpose(2, 0, 1).astype(np.float64) - dist.cpu().numpy().astype(np.float64)
        n = d.size
        want = _psnr_c(float((d * d).sum()), n, float(peak))
        bound = (10 / math.log(10)) * 2 * (n + 1) * 2.0 ** -53 + 4 * 2.0 ** -52 * want
        print("picture %d: psnr %.17g, numpy %.17g, |diff| %.3g (bound %.3g)" % (i, log["frame_psnr"][i], want, abs(log["frame_psnr"][i] - want), bound))
        assert abs(log["frame_psnr"][i] - want) <= bound
        assert 5 < want < 99
    assert log["ave_all_frame_psnr"] == pytest.approx(float(np.mean(log["frame_psnr"])), rel=1e-15)
    # hashes: the manifest's sequence CRC is zlib's of the -o file; the encoder's manifest is the decoder's; --verify-hash passes
    m = picture_hash.read_manifest(str(tmp_path / "dec.hash"))
    assert (m.src_type, m.bit_depth, m.width, m.height, len(m.pictures)) == ("rgb48", depth, W, H, N)
    assert m.sequence_crc == zlib.crc32(rec) and m.total_bytes == len(rec)
    assert [c for c, _ in m.pictures] == [zlib.crc32(rec[i * 6 * H * W:(i + 1) * 6 * H * W]) for i in range(N)]
    assert (tmp_path / "enc.hash").read_bytes() == (tmp_path / "dec.hash").read_bytes()
    r = _run(["decode"] + intra + src + ["-i", str(tmp_path / "out.bin"), "--verify-hash", str(tmp_path / "dec.hash")])
    assert "verified %d pictures" % N in r.stdout
    # --quality-log: the encoder's own measurement is the decoder's log's
    q = json.loads((tmp_path / "quality.json").read_text())
    assert (q["src_type"], q["bit_depth"]) == ("rgb48", depth)
    assert [v for u in q["units"] for v in u["frame_psnr"]] == log["frame_psnr"]


def test_rgb48_with_the_ld_model_equals_the_plugin_path(tmp_path, models):
    mi, mp, intra, inter = models
    depth = 10
    pics = _pictures(depth)
    _write_rgb48(tmp_path / "in.rgb48", pics)
    src = ["--src-type", "rgb48", "--bit-depth", str(depth)]
    coding = ["--qp-i", str(QP_I), "--qp-p", str(QP_P), "--reset-interval", str(RESET)]
    _run(["encode"] + intra + inter + src + coding + ["-i", str(tmp_path / "in.rgb48"), "-W", str(W), "-H", str(H), "-o", str(tmp_path / "out.bin")])
    _run(["decode"] + intra + inter + src + ["-i", str(tmp_path / "out.bin"), "-o", str(tmp_path / "rec.rgb48"), "--ref", str(tmp_path / "in.rgb48"),
                                             "--json", str(tmp_path / "log.json")])
    want_bin, x_hats = _plugin([_x_of(p, depth) for p in pics], mi, mp)
    assert (tmp_path / "out.bin").read_bytes() == want_bin, "the tool's stream differs from the plug-in path's"
    want_rec = b"".join(_host16(rgb.x_to_rgb16(x_hat, H, W, depth)[1]).astype("<u2").tobytes() for x_hat in x_hats)
    assert (tmp_path / "rec.rgb48").read_bytes() == want_rec
    log = json.loads((tmp_path / "log.json").read_text())
    assert set(log) == RGB_KEYS, set(log) ^ RGB_KEYS
    assert log["i_frame_num"] == 1 and log["p_frame_num"] == N - 1


def test_png16_in_and_out_equal_rgb48_at_16_bits(tmp_path, models):
    _, _, intra, _ = models
    pics = _pictures(16)
    _write_rgb48(tmp_path / "in.rgb48", pics)
    (tmp_path / "src").mkdir()
    for i, p in enumerate(pics):
        rgb.write_png16(str(tmp_path / "src" / ("im%05d.png" % (i + 1))), p)
    _run(["encode"] + intra + ["--src-type", "rgb48", "-i", str(tmp_path / "in.rgb48"), "-W", str(W), "-H", str(H), "--qp-i", str(QP_I),
                               "-o", str(tmp_path / "rgb48.bin")])                          # --bit-depth defaults to 16
    _run(["encode"] + intra + ["--src-type", "png16", "-i", str(tmp_path / "src"), "--qp-i", str(QP_I), "-o", str(tmp_path / "png16.bin")])
    assert (tmp_path / "png16.bin").read_bytes() == (tmp_path / "rgb48.bin").read_bytes()
    _run(["encode"] + intra + ["--src-type", "png16", "-i", str(tmp_path / "src"), "--qp-i", str(QP_I), "--batch", "2", "-o", str(tmp_path / "batch.bin")])
    assert (tmp_path / "batch.bin").read_bytes() == (tmp_path / "rgb48.bin").read_bytes()
    _run(["decode"] + intra + ["--src-type", "rgb48", "-i", str(tmp_path / "rgb48.bin"), "-o", str(tmp_path / "rec.rgb48"),
                               "--ref", str(tmp_path / "in.rgb48"), "--json", str(tmp_path / "rgb48.json")])
    _run(["decode"] + intra + ["--src-type", "png16", "-i", str(tmp_path / "png16.bin"), "-o", str(tmp_path / "rec"), "--ref", str(tmp_path / "src"),
                               "--json", str(tmp_path / "png16.json"), "--hash-log", str(tmp_path / "png16.hash")])
    rec = np.frombuffer((tmp_path / "rec.rgb48").read_bytes(), dtype="<u2").reshape(N, H, W, 3)
    names = sorted(os.listdir(tmp_path / "rec"))
    assert names == ["im%05d.png" % (i + 1) for i in range(N)]
    for i, name in enumerate(names):
        assert rgb.png_info2(str(tmp_path / "rec" / name)) == (W, H, 16)
        assert np.array_equal(rgb.read_png16(str(tmp_path / "rec" / name)), rec[i]), name
    a, b = (json.loads((tmp_path / n).read_text()) for n in ("rgb48.json", "png16.json"))
    assert set(a) == set(b) == RGB_KEYS
    assert a["ave_all_frame_psnr"] == b["ave_all_frame_psnr"] and a["ave_all_frame_bpp"] == b["ave_all_frame_bpp"]
    m = picture_hash.read_manifest(str(tmp_path / "png16.hash"))
    assert (m.src_type, m.bit_depth) == ("png16", 16) and m.sequence_crc == zlib.crc32(rec.astype("<u2").tobytes())
    # an 8-bit picture among the references is refused with its name
    rgb.write_png(str(tmp_path / "src" / "im00002.png"), np.zeros((H, W, 3), np.uint8))
    r = _run(["decode"] + intra + ["--src-type", "png16", "-i", str(tmp_path / "png16.bin"), "--ref", str(tmp_path / "src")], check=False)
    assert r.returncode != 0 and "im00002.png is an 8-bit PNG" in r.stderr


def test_a_bt2020_limited_10_bit_yuv_stream_decodes_to_16_bit_png(tmp_path, models):
    """what README advertises for --matrix bt2020 --range limited --yuv-depth 10, now without losing the bits: a stream coded
    from yuv420 --bit-depth 10 is decoded to png16, and the pixels are the numpy restatement's of the plug-in's x_hat"""
    mi, _, intra, _ = models
    rng = np.random.default_rng(2)
    with open(tmp_path / "in.yuv", "wb") as f:
        for i in range(N):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=9)
            for p in (y, uv):
                f.write((p.astype(np.uint16) * 4 + rng.integers(0, 4, p.shape)).astype("<u2").tobytes())
    _run(["encode"] + intra + ["--src-type", "yuv420", "--bit-depth", "10", "-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H),
                               "--qp-i", str(QP_I), "-o", str(tmp_path / "out.bin")])
    colour = ["--matrix", "bt2020", "--range", "limited", "--yuv-depth", "10"]
    _run(["decode"] + intra + ["--src-type", "png16", "-i", str(tmp_path / "out.bin"), "-o", str(tmp_path / "rec")] + colour)
    x_hats = _plugin_decode((tmp_path / "out.bin").read_bytes(), N, _gpu(mi), None)
    for i, x_hat in enumerate(x_hats):
        host = x_hat[0].permute(1, 2, 0).contiguous().cpu().numpy()
        _, want = rgb16_np.x_to_rgb16(host, H, W, 16, "bt2020", "limited", 10)
        got = rgb.read_png16(str(tmp_path / "rec" / ("im%05d.png" % (i + 1))))
        assert np.array_equal(got, want), i
        assert len(np.unique(got)) > 256                       # more levels than an 8-bit PNG could hold


def test_rgb48_searches_and_scene_cuts_measure_what_the_decoder_logs(tmp_path, models):
    """--target-psnr with --scene-cut and an LD model, and --target-bpp on an all-intra run: the encoder converts, measures and
    searches on rgb48 pictures; what --quality-log holds per picture is == the decoder's log of the stream it wrote"""
    _, _, intra, inter = models
    depth = 12
    pics = _pictures(depth)
    _write_rgb48(tmp_path / "in.rgb48", pics)
    src = ["--src-type", "rgb48", "--bit-depth", str(depth)]
    size = ["-i", str(tmp_path / "in.rgb48"), "-W", str(W), "-H", str(H)]
    _run(["encode"] + intra + inter + src + size + ["--qp-i", str(QP_I), "--target-psnr", "11.9", "--quality-log", str(tmp_path / "q.json"),
                                                   "--scene-cut", "5", "--scene-log", str(tmp_path / "scene.json"), "-o", str(tmp_path / "ld.bin")])
    _run(["decode"] + intra + inter + src + ["-i", str(tmp_path / "ld.bin"), "--ref", str(tmp_path / "in.rgb48"), "--json", str(tmp_path / "ld.json"),
                                             "--verbose-json", "1"])
    q, log = json.loads((tmp_path / "q.json").read_text()), json.loads((tmp_path / "ld.json").read_text())
    assert (q["src_type"], q["bit_depth"], q["target_psnr"]) == ("rgb48", depth, 11.9)
    assert [v for u in q["units"] for v in u["frame_psnr"]] == log["frame_psnr"] and len(log["frame_psnr"]) == N
    assert len(json.loads((tmp_path / "scene.json").read_text())["pictures"]) == N
    _run(["encode"] + intra + src + size + ["--target-bpp", "0.5", "--quality-log", str(tmp_path / "q2.json"), "-o", str(tmp_path / "rate.bin")])
    _run(["decode"] + intra + src + ["-i", str(tmp_path / "rate.bin"), "--ref", str(tmp_path / "in.rgb48"), "--json", str(tmp_path / "rate.json"),
                                     "--verbose-json", "1"])
    q, log = json.loads((tmp_path / "q2.json").read_text()), json.loads((tmp_path / "rate.json").read_text())
    assert [v for u in q["units"] for v in u["frame_psnr"]] == log["frame_psnr"] and log["i_frame_num"] == N
