"""dcvc encode / decode with --src-type yuv444 | yuv422 | nv12 | p010 and Y4M files on a real MI355X, against the SAME sequence
driven through the Python plugin surface the way test_video.py:166-399 does it, with the picture I/O as torch ops (v / max_val
on the CPU, .half() - 0.5, repeated chroma; x_hat + 0.5, the chroma mean, the scale, clamp and round) and none of the new C
ABI: byte-identical streams, identical -o files, PSNR per picture; nv12 against yuv420 on one clip; Y4M in and out; --batch;
--calc-ssim against the numpy MS-SSIM."""
import copy
import io
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import msssim_range_np
import pixfmt_np as pn
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, pixfmt, stream_helper as sh, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
SFX = ("", "_y", "_u", "_v")
YUV_KEYS = ({"arith_policy", "frame_pixel_num", "i_frame_num", "p_frame_num", "test_time"}
            | {"ave_%s_frame_%s%s" % (c, m, s) for c in ("i", "p", "all") for m in ("bpp", "psnr") for s in SFX} - {
                "ave_%s_frame_bpp%s" % (c, s) for c in ("i", "p", "all") for s in SFX[1:]})
VERBOSE = {"frame_bpp", "frame_type"} | {"frame_psnr" + s for s in SFX}


def _run(args, check=True):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, check=check, capture_output=True, text=True, timeout=600)


def _pictures(fmt, bits, H, W, n, seed=5):
    """LSB-aligned planes (y [H, W], cbcr [2, Hc, Wc]) per picture: the synthetic 8-bit 4:2:0 sequence, its chroma repeated
    to the format's resolution plus noise, scaled to `bits` plus low-order noise"""
    rng = np.random.default_rng(seed)
    sh_, sw_ = pn.sub(fmt)
    out = []
    for i in range(n):
        y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=seed)
        c = np.repeat(np.repeat(uv, 2 >> sh_, axis=1), 2 >> sw_, axis=2).astype(np.int32)
        c = np.clip(c + rng.integers(-3, 4, c.shape), 0, 255)
        s = 1 << (bits - 8)
        out.append(tuple((p.astype(np.uint32) * s + rng.integers(0, s, p.shape)).astype(pn.dtype(bits)) for p in (y, c)))
    return out


def _file_bytes(pics, fmt, bits, rng=None):
    """the pictures in file layout; P010: random low bits below the value when rng is given"""
    out = []
    for y, c in pics:
        pic = pn.pack(y, c, fmt, bits)
        s = pn.shift(fmt, bits)
        if s and rng is not None:
            pic = pic | rng.integers(0, 1 << s, pic.size).astype(pic.dtype)
        out.append(pic.astype("<u2" if bits > 8 else np.uint8).tobytes())
    return b"".join(out)


def _x_of(pics, fmt, bits):
    """the reader as torch ops: v / max_val on the CPU (true division), .half() - 0.5, chroma repeated over its luma positions
    -> [1, 3 n, H, W] fp16, channels_last"""
    m = (1 << bits) - 1
    sh_, sw_ = pn.sub(fmt)
    xs = []
    for y, c in pics:
        yf = torch.from_numpy(y.astype(np.float32)) / m
        cf = torch.from_numpy(c.astype(np.float32)) / m
        up = cf.repeat_interleave(1 << sh_, dim=1).repeat_interleave(1 << sw_, dim=2)
        xs.append((torch.cat((yf[None], up), dim=0).half() - 0.5)[None])
    return torch.cat(xs, dim=1).cuda().contiguous(memory_format=torch.channels_last)


def _rec_of(x_hat, H, W, fmt, bits):
    """the writer as torch ops on the GPU -> (dist_y [H, W], dist_c [2, Hc, Wc] fp32 numpy, the picture's bytes in file layout)"""
    m = float((1 << bits) - 1)
    sh_, sw_ = pn.sub(fmt)
    t = x_hat[0, :, :H, :W] + 0.5
    c = t[1:].float()
    if sh_:
        tc = ((((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + c[:, 1::2, 0::2]) + c[:, 1::2, 1::2]) * 0.25).half()
    elif sw_:
        tc = ((c[:, :, 0::2] + c[:, :, 1::2]) * 0.5).half()
    else:
        tc = t[1:]
    if bits == 8:
        dy, dc = (torch.clamp(p * 255, 0, 255).float() for p in (t[0], tc))          # fp16 product and clamp
    else:
        dy, dc = (torch.clamp(p.float() * m, 0, m) for p in (t[0], tc))
    sy = torch.round(dy).to(torch.int32).cpu().numpy()
    sc = (torch.trunc(dc) if bits == 8 and sh_ else torch.round(dc)).to(torch.int32).cpu().numpy()
    return dy.cpu().numpy(), dc.cpu().numpy(), _file_bytes([(sy, sc)], fmt, bits)


def _psnr(src, dist, peak):
    d = src.astype(np.float64) - dist.astype(np.float64)
    mse = float((d * d).sum()) / d.size
    return min(10 * np.log10(peak * peak / mse) if mse > 1e-10 else 999.9, 99.9)


def _gpu(m):
    g = copy.deepcopy(m).half().cuda()
    g.proxy = None
    return g


def _python_reference(pics, H, W, fmt, bits, i_model, p_model, delay, qp_i, qp_p, reset_interval):
    """test_video.py:204-399 on the plugin surface -> (stream bytes, reconstruction bytes, [psnr list], [(dist_y, dist_c)])"""
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
        x = _x_of([pics[i] for i in ids], fmt, bits)
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
    peak = float((1 << bits) - 1)
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
            dy, dc, samples = _rec_of(x_hat, H, W, fmt, bits)
            y, c = pics[len(rec)]
            rec.append(samples)
            dists.append((dy, dc))
            p = [_psnr(y, dy, peak), _psnr(c[0], dc[0], peak), _psnr(c[1], dc[1], peak)]
            psnr.append([(6 * p[0] + p[1] + p[2]) / 8] + p)
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


CASES = [("yuv444", [], pn.YUV444P, 8, None, 2), ("yuv422", ["--bit-depth", "10"], pn.YUV422P, 10, "ld", 3),
         ("p010", [], pn.NV12, 10, "hts", 10)]


@pytest.mark.parametrize("name,depth_flag,fmt,bits,inter,n", CASES, ids=[c[0] for c in CASES])
def test_files_equal_the_plugin_path(tmp_path, name, depth_flag, fmt, bits, inter, n):
    H, W, qp_i, qp_p, reset_interval = 96, 128, 30, 36, 4
    pics = _pictures(fmt, bits, H, W, n)
    (tmp_path / "in.yuv").write_bytes(_file_bytes(pics, fmt, bits, np.random.default_rng(1)))       # P010: non-zero low bits
    mi, mp, args = _models(tmp_path, inter)
    kind = ["--src-type", name] + depth_flag
    coding = ["--qp-i", str(qp_i), "--qp-p", str(qp_p), "--reset-interval", str(reset_interval)]
    _run(["encode"] + args + coding + kind + ["-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H), "-o", str(tmp_path / "out.bin")])
    _run(["decode"] + args + kind + ["-i", str(tmp_path / "out.bin"), "-o", str(tmp_path / "rec.yuv"), "--ref", str(tmp_path / "in.yuv"),
                                     "--json", str(tmp_path / "log.json"), "--verbose-json", "1"])
    delay = 1 if inter in (None, "ld") else 8
    want_bin, want_rec, want_psnr, _ = _python_reference(pics, H, W, fmt, bits, mi, mp, delay, qp_i, qp_p, reset_interval)
    assert (tmp_path / "out.bin").read_bytes() == want_bin, "the tool's stream differs from the plugin path's"
    assert (tmp_path / "rec.yuv").read_bytes() == want_rec, "the reconstruction differs"
    log = json.loads((tmp_path / "log.json").read_text())
    assert set(log) == YUV_KEYS | VERBOSE, set(log) ^ (YUV_KEYS | VERBOSE)
    n_i = n if inter is None else 1
    assert log["i_frame_num"] == n_i and log["p_frame_num"] == n - n_i and log["frame_pixel_num"] == H * W
    for k, s in enumerate(SFX):
        assert len(log["frame_psnr" + s]) == n
        for got, want in zip(log["frame_psnr" + s], want_psnr):
            assert got == pytest.approx(want[k], rel=1e-9, abs=0), (s, got, want)
        assert log["ave_all_frame_psnr" + s] == pytest.approx(np.mean([p[k] for p in want_psnr]), rel=1e-8)   # 9 digits
    assert log["ave_all_frame_bpp"] == pytest.approx(8.0 * len(want_bin) / (n * H * W), rel=1e-8)


def _numbers(log):
    log = dict(log)
    log.pop("test_time")
    return log


def test_nv12_equals_yuv420_on_the_same_clip(tmp_path):
    H, W, n = 96, 128, 2
    pics = _pictures(pn.YUV420P, 8, H, W, n, seed=3)
    (tmp_path / "p.yuv").write_bytes(_file_bytes(pics, pn.YUV420P, 8))
    (tmp_path / "n.yuv").write_bytes(_file_bytes(pics, pn.NV12, 8))
    _, _, args = _models(tmp_path, None)
    logs = {}
    for k, t in (("p", "yuv420"), ("n", "nv12")):
        _run(["encode"] + args + ["--src-type", t, "--qp-i", "30", "-i", str(tmp_path / (k + ".yuv")), "-W", str(W), "-H", str(H),
                                  "-o", str(tmp_path / (k + ".bin"))])
        _run(["decode"] + args + ["--src-type", t, "-i", str(tmp_path / (k + ".bin")), "-o", str(tmp_path / (k + ".rec")),
                                  "--ref", str(tmp_path / (k + ".yuv")), "--json", str(tmp_path / (k + ".json")), "--verbose-json", "1"])
        logs[k] = _numbers(json.loads((tmp_path / (k + ".json")).read_text()))
    assert (tmp_path / "n.bin").read_bytes() == (tmp_path / "p.bin").read_bytes()
    planar = np.frombuffer((tmp_path / "p.rec").read_bytes(), np.uint8).reshape(n, -1)
    nv = np.frombuffer((tmp_path / "n.rec").read_bytes(), np.uint8).reshape(n, -1)
    for a, b in zip(planar, nv):
        assert np.array_equal(pn.planar(b, pn.NV12, 8, H, W), a), "the samples differ after de-interleaving"
    assert set(logs["n"]) == set(logs["p"])
    for key, want in logs["p"].items():
        assert logs["n"][key] == pytest.approx(want, rel=1e-9, abs=0), key


def _y4m(path, head, pictures):
    with open(path, "wb") as f:
        f.write(head)
        for i, p in enumerate(pictures):
            f.write(b"FRAME\n" if i % 2 == 0 else b"FRAME Ip XPICTURE=%d\n" % i)
            f.write(p)


def test_a_420_y4m_file_gives_the_raw_files_stream(tmp_path):
    H, W, n = 96, 128, 3
    _, _, args = _models(tmp_path, None)
    raw = _file_bytes(_pictures(pn.YUV420P, 8, H, W, n, seed=2), pn.YUV420P, 8)
    fb = len(raw) // n
    (tmp_path / "a.yuv").write_bytes(raw)
    _y4m(tmp_path / "a.y4m", b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG\n" % (W, H), [raw[i * fb:(i + 1) * fb] for i in range(n)])
    _run(["encode"] + args + ["--qp-i", "30", "-i", str(tmp_path / "a.yuv"), "-W", str(W), "-H", str(H), "-o", str(tmp_path / "a_raw.bin")])
    _run(["encode"] + args + ["--qp-i", "30", "-i", str(tmp_path / "a.y4m"), "-o", str(tmp_path / "a_y4m.bin")])
    assert (tmp_path / "a_y4m.bin").read_bytes() == (tmp_path / "a_raw.bin").read_bytes()
    # a Y4M file that ends inside a picture, and a reference of another size
    (tmp_path / "short.y4m").write_bytes((tmp_path / "a.y4m").read_bytes()[:-10])
    r = _run(["encode"] + args + ["--qp-i", "30", "-i", str(tmp_path / "short.y4m"), "-o", str(tmp_path / "short.bin")], check=False)
    assert r.returncode != 0 and "ends inside picture 3" in r.stderr and not (tmp_path / "short.bin").exists(), r.stderr
    _y4m(tmp_path / "small.y4m", b"YUV4MPEG2 W64 H48 C444p10\n", [bytes(64 * 48 * 6)])
    r = _run(["decode"] + args + ["-i", str(tmp_path / "a_raw.bin"), "--ref", str(tmp_path / "small.y4m"), "--json", str(tmp_path / "x.json")], check=False)
    assert r.returncode != 0 and "holds 64x48 pictures, the output is 128x96" in r.stderr, r.stderr


def test_a_444p10_y4m_file_needs_no_flags_and_batch_2_equals_batch_1(tmp_path):
    H, W, n = 96, 128, 3
    _, _, args = _models(tmp_path, None)
    fmt, bits = pn.YUV444P, 10
    raw = _file_bytes(_pictures(fmt, bits, H, W, n, seed=4), fmt, bits)
    fb = len(raw) // n
    (tmp_path / "b.yuv").write_bytes(raw)
    _y4m(tmp_path / "b.y4m", b"YUV4MPEG2 C444p10 W%d H%d F60:1\n" % (W, H), [raw[i * fb:(i + 1) * fb] for i in range(n)])
    flags = ["--src-type", "yuv444", "--bit-depth", "10"]
    _run(["encode"] + args + flags + ["--qp-i", "30", "-i", str(tmp_path / "b.yuv"), "-W", str(W), "-H", str(H), "-o", str(tmp_path / "b_raw.bin")])
    _run(["encode"] + args + ["--qp-i", "30", "-i", str(tmp_path / "b.y4m"), "-o", str(tmp_path / "b_y4m.bin")])
    _run(["encode"] + args + ["--qp-i", "30", "--batch", "2", "-i", str(tmp_path / "b.y4m"), "-o", str(tmp_path / "b_batch.bin")])
    stream = (tmp_path / "b_raw.bin").read_bytes()
    assert (tmp_path / "b_y4m.bin").read_bytes() == stream and (tmp_path / "b_batch.bin").read_bytes() == stream
    _run(["decode"] + args + flags + ["-i", str(tmp_path / "b_raw.bin"), "-o", str(tmp_path / "b_raw.rec"), "--ref", str(tmp_path / "b.yuv"),
                                      "--json", str(tmp_path / "b_raw.json"), "--verbose-json", "1"])
    for name, extra, rate in (("b_y4m", [], (60, 1)), ("b_batch", ["--batch", "2", "--fps", "24000:1001"], (24000, 1001))):
        _run(["decode"] + args + extra + ["-i", str(tmp_path / "b_raw.bin"), "-o", str(tmp_path / (name + ".y4m")), "--ref", str(tmp_path / "b.y4m"),
                                          "--json", str(tmp_path / (name + ".json")), "--verbose-json", "1"])
        assert _numbers(json.loads((tmp_path / (name + ".json")).read_text())) == _numbers(json.loads((tmp_path / "b_raw.json").read_text()))
        # -o rec.y4m parses back to the same pictures; the rate is --fps, else --ref's
        data = (tmp_path / (name + ".y4m")).read_bytes()
        h = pixfmt.y4m_header(data)
        assert (h["width"], h["height"], h["pix_fmt"], h["bit_depth"], h["fps_num"], h["fps_den"]) == (W, H, fmt, bits) + rate
        at, got = h["header_bytes"], []
        while at < len(data):
            at += pixfmt.y4m_frame_header_bytes(data[at:at + 64])
            got.append(data[at:at + fb])
            at += fb
        assert at == len(data) and b"".join(got) == (tmp_path / "b_raw.rec").read_bytes()
    assert (tmp_path / "b_batch.y4m").read_bytes().startswith(b"YUV4MPEG2 W%d H%d F24000:1001 Ip C444p10\nFRAME\n" % (W, H))


def test_calc_ssim_on_yuv422(tmp_path):
    H, W, fmt, bits = 176, 192, pn.YUV422P, 8
    pics = _pictures(fmt, bits, H, W, 1, seed=6)
    (tmp_path / "in.yuv").write_bytes(_file_bytes(pics, fmt, bits))
    mi, _, args = _models(tmp_path, None)
    kind = ["--src-type", "yuv422"]
    _run(["encode"] + args + kind + ["-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "30", "-o", str(tmp_path / "out.bin")])
    _run(["decode"] + args + kind + ["-i", str(tmp_path / "out.bin"), "--ref", str(tmp_path / "in.yuv"), "--json", str(tmp_path / "log.json"),
                                     "--calc-ssim", "1", "--verbose-json", "1"])
    log = json.loads((tmp_path / "log.json").read_text())
    data, _, psnr, dists = _python_reference(pics, H, W, fmt, bits, mi, None, 1, 30, 30, 0)
    assert (tmp_path / "out.bin").read_bytes() == data
    (y, c), (dy, dc) = pics[0], dists[0]
    want = [msssim_range_np.msssim(y, dy, 255.0)] + [msssim_range_np.msssim(c[k], dc[k], 255.0) for k in range(2)]
    want = [(6 * want[0] + want[1] + want[2]) / 8] + want
    for k, s in enumerate(SFX):
        assert abs(log["frame_msssim" + s][0] - want[k]) <= 1e-10, (s, log["frame_msssim" + s], want[k])
        assert abs(log["ave_all_frame_msssim" + s] - want[k]) <= 1e-10 and log["ave_p_frame_msssim" + s] == 0
        assert log["frame_psnr" + s][0] == pytest.approx(psnr[0][k], rel=1e-9, abs=0)
    # a picture whose chroma planes fall below 88 (96 x 96 in 4:2:2: 48 wide) is refused before anything is decoded
    _run(["encode"] + args + kind + ["-i", str(tmp_path / "in.yuv"), "-W", "96", "-H", "96", "-n", "1", "--qp-i", "30", "-o", str(tmp_path / "s.bin")])
    r = _run(["decode"] + args + kind + ["-i", str(tmp_path / "s.bin"), "--ref", str(tmp_path / "in.yuv"), "--json", str(tmp_path / "s.json"),
                                         "--calc-ssim", "1"], check=False)
    assert r.returncode != 0 and "--calc-ssim needs the sides of every plane >= 88" in r.stderr, r.stderr
