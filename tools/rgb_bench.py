"""Timing of the RGB picture kernels (dcvc_rgb_to_x, dcvc_x_to_rgb, dcvc_sse) and of the standalone tool's RGB modes, printed as
one JSON line.

  * per picture at 1920x1080 and 3840x2160: HIP events around --batch back-to-back calls after a warm-up, the median of
    --reps such batches divided by the batch. The calls rotate over enough distinct buffers (> 512 MB in all) that the
    256 MB Infinity Cache cannot hold them, so the bytes come from HBM. Each entry also gives the bytes one call moves and
    the fraction of 6.3 TB/s (MI355X_MICROARCH.md) that is;
      rgb_to_x: packed u8 RGB -> x (fp16, ldx 3);
      x_to_rgb: x_hat (fp16, rows padded to 16) -> the fp16 planes and the packed u8 pixels;
      sse_psnr: dcvc_sse of the u8 source planes against the fp16 planes (3 planes, one call, its workspace included) and
                the PSNR from the three sums on the host;
  * the standalone tool (dcvc_amd/bin/dcvc) on one 1080p intra stream from synthetic weights: pictures/s of `dcvc encode` and
    `dcvc decode --ref --json` in --src-type yuv420, rgb24 and png from the same pictures (file I/O included, as the tool
    reports it; PNG rates are bound by the host's inflate / deflate).

Needs the GPU. Usage: python tools/rgb_bench.py [--batch 20] [--reps 30] [--pictures 8] [--out profiles/rgb_bench.json]
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dcvc_amd import _lib, arch, export_weights, models, rgb, synthetic  # noqa: E402

TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
HBM_TBPS = 6.3
vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


def _rgb_pictures(H, W, n, seed=3):
    """[H, W, 3] u8 pictures and the YUV420 planes they are made from (synthetic content, three mixed channels)"""
    out = []
    for i in range(n):
        y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=seed)
        up = np.repeat(np.repeat(uv.astype(np.int32) - 128, 2, axis=1), 2, axis=2)
        yy = y.astype(np.int32)
        pic = np.clip(np.stack([yy + 2 * up[1], yy - up[0] - up[1], yy + 2 * up[0]], axis=-1), 0, 255).astype(np.uint8)
        out.append((pic, y, uv))
    return out


def _timed(call, n_bufs, batch, reps, warmup=3):
    for k in range(warmup * n_bufs):
        call(k % n_bufs)
    torch.cuda.synchronize()
    per = []
    k = 0
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            call(k % n_bufs)
            k += 1
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1000.0 / batch)
    return per


def _entry(per_us, nbytes):
    med = float(np.median(per_us))
    floor = nbytes / (HBM_TBPS * 1e12) * 1e6
    return {"median_us": med, "min_us": float(np.min(per_us)), "max_us": float(np.max(per_us)), "bytes": int(nbytes),
            "hbm_floor_us": floor, "fraction_of_hbm": floor / med}


def time_kernels(H, W, batch, reps):
    f_to_x = _lib.fn("dcvc_rgb_to_x", ci, [vp, ll, ll, ll, ci, ci, vp, ci, vp, vp])
    f_to_rgb = _lib.fn("dcvc_x_to_rgb", ci, [vp, ci, ci, ci, vp, vp, vp])
    f_sse = _lib.fn("dcvc_sse", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, vp, vp])
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = lambda t: vp(t.data_ptr())
    res = {}
    pic = torch.from_numpy(np.ascontiguousarray(np.tile(_rgb_pictures(1080, 1920, 1)[0][0], (H // 1080, W // 1920, 1)))).cuda()

    # rgb_to_x: 3 HW in, 6 HW out
    nbytes = 9 * H * W
    n = max(2, -(-(512 << 20) // nbytes))
    srcs = [pic.clone() for _ in range(n)]
    xs = [torch.empty((H, W, 3), dtype=torch.float16, device="cuda") for _ in range(n)]
    res["rgb_to_x"] = _entry(_timed(lambda k: _lib.check(f_to_x(p(srcs[k]), 3 * W, 3, 1, H, W, p(xs[k]), 3, None, st)),
                                    n, batch, reps), nbytes)
    x0 = xs[0]
    del srcs, xs

    # x_to_rgb: 6 Hp Wp in, 6 HW + 3 HW out
    nbytes = 6 * Hp * Wp + 9 * H * W
    n = max(2, -(-(512 << 20) // nbytes))
    xh = torch.zeros((Hp, Wp, 3), dtype=torch.float16, device="cuda")
    xh[:H, :W] = x0
    xhs = [xh.clone() for _ in range(n)]
    r16 = [torch.empty((3, H, W), dtype=torch.float16, device="cuda") for _ in range(n)]
    r8 = [torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(n)]
    res["x_to_rgb"] = _entry(_timed(lambda k: _lib.check(f_to_rgb(p(xhs[k]), Wp, H, W, p(r16[k]), p(r8[k]), st)),
                                    n, batch, reps), nbytes)
    rec16 = r16[0]
    del xhs, r16, r8

    # sse + PSNR: 3 HW u8 + 6 HW fp16 in
    nbytes = 9 * H * W
    n = max(2, -(-(512 << 20) // nbytes))
    planar = pic.permute(2, 0, 1).contiguous()
    src = [planar.clone() for _ in range(n)]
    rec = [rec16.clone() for _ in range(n)]
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    res["sse"] = _entry(_timed(lambda k: _lib.check(f_sse(p(src[k]), 0, p(rec[k]), 1, 3, H, W, W, H * W, p(out), st)),
                               n, batch, reps), nbytes)
    # the PSNR as the tool takes it: the three sums to the host, then calc_psnr
    per = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(batch):
            rgb.psnr_rgb(src[k % n], rec[k % n])
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1000.0 / batch)
    res["sse_psnr"] = _entry(per, nbytes)
    res["sse_psnr"]["psnr"] = rgb.psnr_rgb(src[0], rec[0])
    return res


def time_tool(pictures):
    H, W = 1080, 1920
    m = models.DMCI()
    m.load_state_dict(synthetic.synthetic_state_dict(arch.dmci_spec(), 0))
    m.update(0.15)
    pics = _rgb_pictures(H, W, pictures)
    res = {"pictures": pictures, "stream": "1080p intra, synthetic weights, qp 32"}
    with tempfile.TemporaryDirectory() as d:
        j = lambda *a: os.path.join(d, *a)
        with open(j("in.yuv"), "wb") as fy, open(j("in.rgb"), "wb") as fr:
            for pic, y, uv in pics:
                fy.write(y.tobytes())
                fy.write(uv.tobytes())
                fr.write(pic.tobytes())
        os.mkdir(j("src"))
        for i, (pic, _, _) in enumerate(pics):
            rgb.write_png(j("src", "im%05d.png" % (i + 1)), pic)
        export_weights.write_dcvw(j("i.dcvw"), "dmci", m, 0.15)
        run = lambda a: subprocess.run([TOOL] + a, check=True, capture_output=True, text=True, timeout=600).stdout
        rate = lambda s: float(re.search(r"([0-9.]+) pictures/s", s).group(1))
        base = ["--intra", j("i.dcvw")]
        src = {"yuv420": j("in.yuv"), "rgb24": j("in.rgb"), "png": j("src")}
        size = {"yuv420": ["-W", str(W), "-H", str(H)], "rgb24": ["-W", str(W), "-H", str(H)], "png": []}
        enc = lambda t: ["encode"] + base + ["--src-type", t, "-i", src[t], "--qp-i", "32", "-o", j(t + ".bin")] + size[t]
        dec = lambda t: ["decode"] + base + ["--src-type", t, "-i", j(t + ".bin"), "--ref", src[t], "--json", j(t + ".json")]
        modes = ("yuv420", "rgb24", "png")
        for t in modes:                        # warm-up (code objects, file cache); makes the streams
            run(enc(t))
            run(dec(t))
        for t in modes:
            res[t] = {"encode": [], "decode_ref_json": []}
        for _ in range(3):                     # alternating
            for t in modes:
                res[t]["encode"].append(rate(run(enc(t))))
                res[t]["decode_ref_json"].append(rate(run(dec(t))))
        for t in modes:
            for k in ("encode", "decode_ref_json"):
                res[t][k + "_median"] = float(np.median(res[t][k]))
            with open(j(t + ".json")) as f:
                res[t]["ave_all_frame_psnr"] = json.load(f)["ave_all_frame_psnr"]
        for t in ("rgb24", "png"):
            for k in ("encode", "decode_ref_json"):
                res[t][k + "_vs_yuv420"] = res[t][k + "_median"] / res["yuv420"][k + "_median"]
        res["rgb24_png_same_stream"] = open(j("rgb24.bin"), "rb").read() == open(j("png.bin"), "rb").read()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pictures", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgb_bench needs the GPU")
    res = {"what": "RGB picture kernels per picture (HIP events, batches of back-to-back calls over > 512 MB of buffers) and "
                   "the dcvc tool's pictures/s per --src-type",
           "device": torch.cuda.get_device_name(0), "hbm_tbps": HBM_TBPS,
           "1920x1080": time_kernels(1080, 1920, a.batch, a.reps),
           "3840x2160": time_kernels(2160, 3840, a.batch, a.reps),
           "tool_1080p_intra_pictures_per_s": time_tool(a.pictures)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
