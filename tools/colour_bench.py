"""Timing of the colour-matrix / range kernels (dcvc_rgb_to_x_cs, dcvc_x_to_rgb_cs) against the BT.709 / full
range entry points they generalise (dcvc_rgb_to_x, dcvc_x_to_rgb), in one run, printed as one JSON line.

Per picture at 1920x1080 and 3840x2160, as tools/rgb_bench.py measures (its _timed and _entry: HIP events around --batch
back-to-back calls after a warm-up, over enough distinct buffers - > 512 MB in all - that the bytes come from HBM). Three
variants per direction - "old" (the entry point without _cs), "bt709_full" and "bt2020_limited_10" (the _cs entry point) -
take turns over --rounds rounds, so a drift of the machine falls on all three; each entry is the median over every batch of
its variant, and "ratio_to_old" is that median over the old entry point's. All variants move the same bytes. Since the
picture kernels were merged (profiles/picture_io_merge.json) "old" and "bt709_full" run the same kernel.

Needs the GPU. Usage: python tools/colour_bench.py [--batch 20] [--reps 10] [--rounds 3] [--out profiles/colour_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from dcvc_amd import _lib  # noqa: E402
from rgb_bench import HBM_TBPS, _entry, _rgb_pictures, _timed  # noqa: E402

vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
VARIANTS = {"old": None, "bt709_full": (1, 0, 8), "bt2020_limited_10": (2, 1, 10)}      # DCVC_MATRIX_*, DCVC_RANGE_*, depth


def _rounds(calls, n, batch, reps, rounds, nbytes):
    per = {name: [] for name in calls}
    for _ in range(rounds):
        for name, call in calls.items():
            per[name] += _timed(call, n, batch, reps)
    res = {name: _entry(v, nbytes) for name, v in per.items()}
    for name in res:
        res[name]["ratio_to_old"] = res[name]["median_us"] / res["old"]["median_us"]
    return res


def time_kernels(H, W, batch, reps, rounds):
    f_to_x = _lib.fn("dcvc_rgb_to_x", ci, [vp, ll, ll, ll, ci, ci, vp, ci, vp, vp])
    f_to_rgb = _lib.fn("dcvc_x_to_rgb", ci, [vp, ci, ci, ci, vp, vp, vp])
    f_to_x_cs = _lib.fn("dcvc_rgb_to_x_cs", ci, [vp, ll, ll, ll, ci, ci, vp, ci, vp, ci, ci, ci, vp])
    f_to_rgb_cs = _lib.fn("dcvc_x_to_rgb_cs", ci, [vp, ci, ci, ci, vp, vp, ci, ci, ci, vp])
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

    def to_x(colour):
        if colour is None:
            return lambda k: _lib.check(f_to_x(p(srcs[k]), 3 * W, 3, 1, H, W, p(xs[k]), 3, None, st))
        return lambda k: _lib.check(f_to_x_cs(p(srcs[k]), 3 * W, 3, 1, H, W, p(xs[k]), 3, None, *colour, st))

    res["rgb_to_x"] = _rounds({name: to_x(c) for name, c in VARIANTS.items()}, n, batch, reps, rounds, nbytes)
    _lib.check(f_to_x(p(srcs[0]), 3 * W, 3, 1, H, W, p(xs[0]), 3, None, st))
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

    def to_rgb(colour):
        if colour is None:
            return lambda k: _lib.check(f_to_rgb(p(xhs[k]), Wp, H, W, p(r16[k]), p(r8[k]), st))
        return lambda k: _lib.check(f_to_rgb_cs(p(xhs[k]), Wp, H, W, p(r16[k]), p(r8[k]), *colour, st))

    res["x_to_rgb"] = _rounds({name: to_rgb(c) for name, c in VARIANTS.items()}, n, batch, reps, rounds, nbytes)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("colour_bench needs the GPU")
    res = {"what": "dcvc_rgb_to_x_cs / dcvc_x_to_rgb_cs per picture against dcvc_rgb_to_x / dcvc_x_to_rgb in one run (HIP events, "
                   "batches of back-to-back calls over > 512 MB of buffers, the variants taking turns)",
           "device": torch.cuda.get_device_name(0), "hbm_tbps": HBM_TBPS, "batch": a.batch, "reps": a.reps, "rounds": a.rounds,
           "1920x1080": time_kernels(1080, 1920, a.batch, a.reps, a.rounds),
           "3840x2160": time_kernels(2160, 3840, a.batch, a.reps, a.rounds)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
