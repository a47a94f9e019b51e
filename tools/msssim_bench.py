"""Timing of MS-SSIM on the GPU (dcvc_msssim), printed as one JSON line.

  * per picture: the two calls of one YUV420 picture (Y as one plane, U + V as two planes; u8 source, fp16 reconstruction),
    bracketed by HIP events after a warm-up; median / min / max of --calls pictures at 1920x1080 and 3840x2160;
  * the standalone decoder (dcvc_amd/bin/dcvc) on a short 1080p intra stream from synthetic weights: pictures/s of
    `dcvc decode --ref --json` with and without `--calc-ssim 1` (file I/O and the host PSNR included, as the tool reports it).

Needs the GPU. Usage: python tools/msssim_bench.py [--calls 200] [--pictures 8] [--out profiles/msssim_bench.json]
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

from dcvc_amd import _lib, arch, export_weights, models, synthetic  # noqa: E402

TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")


def _planes(H, W, seed):
    y, uv = synthetic.synthetic_frame_yuv420(min(H, 1080), min(W, 1920), index=0, seed=seed)
    reps = (H // y.shape[0], W // y.shape[1])
    y, uv = np.tile(y, reps), np.tile(uv, (1,) + reps)
    rng = np.random.default_rng(seed)
    y16 = np.clip(y + rng.normal(0, 4, y.shape), 0, 255).astype(np.float16)
    uv16 = np.clip(uv + rng.normal(0, 4, uv.shape), 0, 255).astype(np.float16)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return cuda(y), cuda(uv), cuda(y16), cuda(uv16)


def time_picture(H, W, calls, warmup=20):
    f = _lib.fn("dcvc_msssim", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p,
                                              ctypes.c_void_p])
    y, uv, y16, uv16 = _planes(H, W, 1)
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def picture():
        _lib.check(f(p(y), 0, p(y16), 1, 1, H, W, W, H * W, p(out), st))
        _lib.check(f(p(uv), 0, p(uv16), 1, 2, H // 2, W // 2, W // 2, H * W // 4, ctypes.c_void_p(out.data_ptr() + 8), st))

    for _ in range(warmup):
        picture()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        picture()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    vals = out.cpu().numpy()
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "calls": calls,
            "msssim_yuv": [float(v) for v in vals]}


def time_decoder(pictures):
    H, W = 1080, 1920
    m = models.DMCI()
    m.load_state_dict(synthetic.synthetic_state_dict(arch.dmci_spec(), 0))
    m.update(0.15)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "in.yuv"), "wb") as f:
            for i in range(pictures):
                y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=3)
                f.write(y.tobytes())
                f.write(uv.tobytes())
        export_weights.write_dcvw(os.path.join(d, "i.dcvw"), "dmci", m, 0.15)
        run = lambda a: subprocess.run([TOOL] + a, check=True, capture_output=True, text=True, timeout=600).stdout
        base = ["--intra", os.path.join(d, "i.dcvw")]
        run(["encode"] + base + ["-i", os.path.join(d, "in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "32",
                                 "-o", os.path.join(d, "out.bin")])
        dec = ["decode"] + base + ["-i", os.path.join(d, "out.bin"), "--ref", os.path.join(d, "in.yuv"),
                                   "--json", os.path.join(d, "log.json")]
        rate = lambda s: float(re.search(r"([0-9.]+) pictures/s", s).group(1))
        res = {"pictures": pictures, "without": [], "with_calc_ssim": []}
        run(dec)                               # warm-up (code objects, file cache)
        for _ in range(2):                     # alternating
            res["without"].append(rate(run(dec)))
            res["with_calc_ssim"].append(rate(run(dec + ["--calc-ssim", "1"])))
        with open(os.path.join(d, "log.json")) as f:
            res["ave_all_frame_msssim"] = json.load(f)["ave_all_frame_msssim"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--pictures", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msssim_bench needs the GPU")
    res = {"what": "dcvc_msssim per YUV420 picture (Y call + U,V call), HIP events",
           "device": torch.cuda.get_device_name(0),
           "1920x1080": time_picture(1080, 1920, a.calls),
           "3840x2160": time_picture(2160, 3840, a.calls),
           "decode_1080p_intra_pictures_per_s": time_decoder(a.pictures)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
