"""Timing of the picture kernels of the other chroma formats (dcvc_pix_to_x, dcvc_x_to_pix), printed as one JSON line. The
method is tools/rgb_bench.py's and tools/yuv16_bench.py's:

  * per picture at 1920x1080 and 3840x2160, for each of yuv420p, yuv422p, yuv444p and nv12 at 8 and 10 bits: HIP events
    around --batch back-to-back calls after a warm-up, the median of --reps such batches divided by the batch, rotating over
    > 512 MB of distinct buffers so that the bytes come from HBM; each entry gives the bytes one call moves, its HBM floor at
    6.3 TB/s, the GB/s reached and the time as a multiple of the floor;
      pix_to_x: the picture (file layout) -> x (fp16, ldx 3);
      x_to_pix: x_hat (fp16, rows padded to 16) -> the fp32 distortion planes and the samples in file layout;
  * in the same run the existing planar 4:2:0 kernels at the same size and depth (dcvc_yuv420_to_x / dcvc_x_to_yuv420 at 8
    bits, dcvc_yuv420p16_to_x / dcvc_x_to_yuv420p16 at 10), whose bytes NV12 / P010 and yuv420p move exactly (the 8-bit
    dcvc_x_to_yuv420 writes fp16 planes, 3 H W bytes, where dcvc_x_to_pix writes fp32 ones, 6 H W), and each new-to-planar
    ratio of the medians. Since the picture kernels were merged (profiles/picture_io_merge.json) those entry points run the
    kernels of dcvc_pix_to_x / dcvc_x_to_pix, so the two columns time the same kernel.

Needs the GPU. Usage: python tools/pixfmt_bench.py [--batch 20] [--reps 30] [--out profiles/pixfmt_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dcvc_amd import _lib, pixfmt  # noqa: E402
from tools.rgb_bench import _entry, _timed  # noqa: E402

vp, ci = ctypes.c_void_p, ctypes.c_int
FORMATS = (("yuv420p", pixfmt.DCVC_PIX_YUV420P), ("yuv422p", pixfmt.DCVC_PIX_YUV422P), ("yuv444p", pixfmt.DCVC_PIX_YUV444P),
           ("nv12", pixfmt.DCVC_PIX_NV12))


def _full(entry):
    entry["gb_per_s"] = entry["bytes"] / entry["median_us"] * 1e-3
    entry["times_hbm_floor"] = entry["median_us"] / entry["hbm_floor_us"]
    return entry


def _bufs(nbytes):
    return max(2, -(-(512 << 20) // nbytes))


def time_size(H, W, batch, reps):
    f_to_x = _lib.fn("dcvc_pix_to_x", ci, [vp, ci, ci, ci, ci, vp, ci, vp, vp])
    f_to_pix = _lib.fn("dcvc_x_to_pix", ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp])
    f_old_to_x8 = _lib.fn("dcvc_yuv420_to_x", ci, [vp, vp, ci, ci, vp, ci, vp])
    f_old_to_x16 = _lib.fn("dcvc_yuv420p16_to_x", ci, [vp, vp, ci, ci, ci, vp, ci, vp])
    f_old_from8 = _lib.fn("dcvc_x_to_yuv420", ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp])
    f_old_from16 = _lib.fn("dcvc_x_to_yuv420p16", ci, [vp, ci, ci, ci, ci, vp, vp, vp])
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: vp(t.data_ptr() + off)
    rng = np.random.default_rng(0)
    x_hat = torch.from_numpy((rng.random((Hp, Wp, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float16)).cuda()
    ny = H * W
    res = {}
    for bits in (8, 10):
        es = 1 if bits == 8 else 2
        sdt = torch.uint8 if bits == 8 else torch.int16
        out = res["%d_bit" % bits] = {}

        def to_x(call, samples):
            nbytes = samples * es + 6 * ny
            n = _bufs(nbytes)
            shift = 6 if bits == 10 and call == "nv12" else 0
            srcs = [torch.from_numpy((rng.integers(0, 1 << bits, samples) << shift).astype(np.uint16).view(np.int16)
                                     if es == 2 else rng.integers(0, 256, samples).astype(np.uint8)).cuda() for _ in range(2)]
            srcs = [srcs[k % 2].clone() for k in range(n)]
            xs = [torch.empty((H, W, 3), dtype=torch.float16, device="cuda") for _ in range(n)]
            if call == "planar420":
                if bits == 8:
                    fn = lambda k: _lib.check(f_old_to_x8(p(srcs[k]), p(srcs[k], ny), H, W, p(xs[k]), 3, st))
                else:
                    fn = lambda k: _lib.check(f_old_to_x16(p(srcs[k]), p(srcs[k], 2 * ny), H, W, bits, p(xs[k]), 3, st))
            else:
                fmt = dict(FORMATS)[call]
                fn = lambda k: _lib.check(f_to_x(p(srcs[k]), fmt, bits, H, W, p(xs[k]), 3, None, st))
            return _full(_entry(_timed(fn, n, batch, reps), nbytes))

        def from_x(call, samples):
            dist_bytes = 2 if call == "planar420" and bits == 8 else 4         # dcvc_x_to_yuv420 writes fp16 planes
            nbytes = 6 * Hp * Wp + samples * (dist_bytes + es)
            n = _bufs(nbytes)
            xhs = [x_hat.clone() for _ in range(n)]
            dists = [torch.empty(samples * dist_bytes, dtype=torch.uint8, device="cuda") for _ in range(n)]
            outs = [torch.empty(samples, dtype=sdt, device="cuda") for _ in range(n)]
            if call == "planar420":
                if bits == 8:
                    fn = lambda k: _lib.check(f_old_from8(p(xhs[k]), Wp, H, W, p(dists[k]), p(dists[k], 2 * ny), p(outs[k]), p(outs[k], ny), st))
                else:
                    fn = lambda k: _lib.check(f_old_from16(p(xhs[k]), Wp, H, W, bits, p(dists[k]), p(outs[k]), st))
            else:
                fmt = dict(FORMATS)[call]
                fn = lambda k: _lib.check(f_to_pix(p(xhs[k]), Wp, H, W, fmt, bits, p(dists[k]), p(outs[k]), st))
            return _full(_entry(_timed(fn, n, batch, reps), nbytes))

        for name, fmt in FORMATS:
            samples = pixfmt.picture_samples(fmt, H, W)
            out[name] = {"pix_to_x": to_x(name, samples), "x_to_pix": from_x(name, samples)}
        samples = pixfmt.picture_samples(pixfmt.DCVC_PIX_YUV420P, H, W)
        out["existing_planar_420"] = {"to_x": to_x("planar420", samples), "from_x": from_x("planar420", samples)}
        old = out["existing_planar_420"]
        out["new_to_planar_ratio"] = {name: {"pix_to_x": out[name]["pix_to_x"]["median_us"] / old["to_x"]["median_us"],
                                             "x_to_pix": out[name]["x_to_pix"]["median_us"] / old["from_x"]["median_us"]}
                                      for name in ("yuv420p", "nv12")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixfmt_bench needs the GPU")
    res = {"what": "dcvc_pix_to_x / dcvc_x_to_pix per picture for each format at 8 and 10 bits (HIP events, batches of back-to-back "
                   "calls over > 512 MB of buffers), the existing planar 4:2:0 kernels in the same run, and the new-to-planar "
                   "ratios of the medians",
           "device": torch.cuda.get_device_name(0),
           "1920x1080": time_size(1080, 1920, a.batch, a.reps),
           "3840x2160": time_size(2160, 3840, a.batch, a.reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
