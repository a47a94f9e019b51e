"""Timing of the high-bit-depth YUV420 kernels (dcvc_yuv420p16_to_x, dcvc_x_to_yuv420p16, dcvc_sse on u16 / fp32 planes) and
of the standalone tool's --bit-depth 10 mode, printed as one JSON line. The method is tools/rgb_bench.py's:

  * per picture at 1920x1080 and 3840x2160: HIP events around --batch back-to-back calls after a warm-up, the median of
    --reps such batches divided by the batch, rotating over > 512 MB of distinct buffers so that the bytes come from HBM;
    each entry gives the bytes one call moves and the fraction of 6.3 TB/s that is;
      yuv420p16_to_x: u16 planes (3 H W bytes) -> x (fp16, ldx 3);
      x_to_yuv420p16: x_hat (fp16, rows padded to 16) -> the fp32 distortion planes and the u16 samples;
      sse: dcvc_sse of the u16 source against the fp32 planes, Y then U + V (two calls, as the tool makes them);
  * the tool (dcvc_amd/bin/dcvc) on one 1080p intra stream from synthetic weights: pictures/s of `dcvc encode` and
    `dcvc decode --ref --json` for an 8-bit YUV420 source, the same pictures at 10 bits, and as RGB24 (file I/O included).

Needs the GPU. Usage: python tools/yuv16_bench.py [--batch 20] [--reps 30] [--pictures 8] [--out profiles/yuv16_bench.json]
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
from tools.rgb_bench import _entry, _rgb_pictures, _timed  # noqa: E402

TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


def _ten_bit(y, uv, seed=0):
    rng = np.random.default_rng(seed)
    return tuple((p.astype(np.uint16) * 4 + rng.integers(0, 4, p.shape)).astype(np.uint16) for p in (y, uv))


def time_kernels(H, W, batch, reps):
    f_to_x = _lib.fn("dcvc_yuv420p16_to_x", ci, [vp, vp, ci, ci, ci, vp, ci, vp])
    f_to_yuv = _lib.fn("dcvc_x_to_yuv420p16", ci, [vp, ci, ci, ci, ci, vp, vp, vp])
    f_sse = _lib.fn("dcvc_sse", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, vp, vp])
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = lambda t: vp(t.data_ptr())
    ny, nc = H * W, (H // 2) * (W // 2)
    y8, uv8 = synthetic.synthetic_frame_yuv420(H, W, index=0, seed=3)
    y, uv = _ten_bit(y8, uv8)
    pic = torch.from_numpy(np.concatenate([y.ravel(), uv.ravel()]).view(np.int16)).cuda()
    res = {}

    # yuv420p16_to_x: 3 HW in, 6 HW out
    nbytes = 9 * H * W
    n = max(2, -(-(512 << 20) // nbytes))
    srcs = [pic.clone() for _ in range(n)]
    xs = [torch.empty((H, W, 3), dtype=torch.float16, device="cuda") for _ in range(n)]
    res["yuv420p16_to_x"] = _entry(_timed(lambda k: _lib.check(f_to_x(p(srcs[k]), vp(srcs[k].data_ptr() + 2 * ny), H, W, 10,
                                                                      p(xs[k]), 3, st)), n, batch, reps), nbytes)
    x0 = xs[0]
    del srcs, xs

    # x_to_yuv420p16: 6 Hp Wp in, 6 HW (fp32) + 3 HW (u16) out
    nbytes = 6 * Hp * Wp + 9 * H * W
    n = max(2, -(-(512 << 20) // nbytes))
    xh = torch.zeros((Hp, Wp, 3), dtype=torch.float16, device="cuda")
    xh[:H, :W] = x0
    xhs = [xh.clone() for _ in range(n)]
    d32 = [torch.empty(ny + 2 * nc, dtype=torch.float32, device="cuda") for _ in range(n)]
    s16 = [torch.empty(ny + 2 * nc, dtype=torch.int16, device="cuda") for _ in range(n)]
    res["x_to_yuv420p16"] = _entry(_timed(lambda k: _lib.check(f_to_yuv(p(xhs[k]), Wp, H, W, 10, p(d32[k]), p(s16[k]), st)),
                                          n, batch, reps), nbytes)
    dist = d32[0]
    del xhs, d32, s16

    # sse: 3 HW (u16) + 6 HW (fp32) in, Y and U + V
    nbytes = 9 * H * W
    n = max(2, -(-(512 << 20) // nbytes))
    src = [pic.clone() for _ in range(n)]
    rec = [dist.clone() for _ in range(n)]
    out = torch.empty(3, dtype=torch.float64, device="cuda")

    def sse(k):
        _lib.check(f_sse(p(src[k]), 3, p(rec[k]), 4, 1, H, W, W, ny, p(out), st))
        _lib.check(f_sse(vp(src[k].data_ptr() + 2 * ny), 3, vp(rec[k].data_ptr() + 4 * ny), 4, 2, H // 2, W // 2, W // 2, nc,
                         vp(out.data_ptr() + 8), st))
    res["sse"] = _entry(_timed(sse, n, batch, reps), nbytes)
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
        with open(j("in8.yuv"), "wb") as f8, open(j("in10.yuv"), "wb") as f10, open(j("in.rgb"), "wb") as fr:
            for i, (pic, y, uv) in enumerate(pics):
                f8.write(y.tobytes() + uv.tobytes())
                y10, uv10 = _ten_bit(y, uv, i)
                f10.write(y10.astype("<u2").tobytes() + uv10.astype("<u2").tobytes())
                fr.write(pic.tobytes())
        export_weights.write_dcvw(j("i.dcvw"), "dmci", m, 0.15)
        run = lambda a: subprocess.run([TOOL] + a, check=True, capture_output=True, text=True, timeout=600).stdout
        rate = lambda s: float(re.search(r"([0-9.]+) pictures/s", s).group(1))
        base = ["--intra", j("i.dcvw"), "-W", str(W), "-H", str(H)]
        modes = {"yuv420_8bit": (j("in8.yuv"), []), "yuv420_10bit": (j("in10.yuv"), ["--bit-depth", "10"]),
                 "rgb24": (j("in.rgb"), ["--src-type", "rgb24"])}
        enc = lambda t: ["encode"] + base + modes[t][1] + ["-i", modes[t][0], "--qp-i", "32", "-o", j(t + ".bin")]
        dec = lambda t: ["decode"] + base + modes[t][1] + ["-i", j(t + ".bin"), "--ref", modes[t][0], "--json", j(t + ".json")]
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
        for t in ("yuv420_10bit", "rgb24"):
            for k in ("encode", "decode_ref_json"):
                res[t][k + "_vs_8bit"] = res[t][k + "_median"] / res["yuv420_8bit"][k + "_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pictures", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv16_bench needs the GPU")
    res = {"what": "high-bit-depth YUV420 kernels per picture at 10 bits (HIP events, batches of back-to-back calls over > 512 MB "
                   "of buffers) and the dcvc tool's pictures/s for 8-bit, 10-bit and RGB24 sources",
           "device": torch.cuda.get_device_name(0),
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
