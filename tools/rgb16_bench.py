"""Timing of the 9..16-bit RGB kernels (dcvc_rgb16_to_x_cs, dcvc_x_to_rgb16_cs) next to the 8-bit pair
(dcvc_rgb_to_x_cs, dcvc_x_to_rgb_cs) in one run, each figure against the HBM floor of the bytes it moves, and dcvc encode
pictures/s on one 1080p intra stream for rgb48 against rgb24. One JSON line.

Per picture at 1920x1080 and 3840x2160, as tools/colour_bench.py measures (rgb_bench's _timed and _entry: HIP events around
--batch back-to-back calls after a warm-up, the same operands every call, over enough distinct buffers - > 512 MB in all -
that the bytes come from HBM). The variants of a direction - "u8", "u16_10" and "u16_16", all BT.709 / full range - take
turns over --rounds rounds, so a drift of the machine falls on all of them; each entry is the median over every batch of its
variant. The variants do not move the same bytes (a u16 picture is twice a u8 one, the fp32 planes twice the fp16 ones): the
yardstick is "times_floor" = median / HBM floor, side by side.

Needs the GPU. Usage: python tools/rgb16_bench.py [--batch 20] [--reps 10] [--rounds 3] [--pictures 8] [--out profiles/rgb16_bench.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from dcvc_amd import _lib, arch, export_weights, models, synthetic  # noqa: E402
from rgb_bench import HBM_TBPS, TOOL, _entry, _rgb_pictures, _timed  # noqa: E402

vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
COLOUR = (1, 0, 8)                                    # DCVC_MATRIX_BT709, DCVC_RANGE_FULL, depth


def _rounds(calls, batch, reps, rounds):
    """calls: {name: (call, n_bufs, nbytes)}"""
    per = {name: [] for name in calls}
    for _ in range(rounds):
        for name, (call, n, _) in calls.items():
            per[name] += _timed(call, n, batch, reps)
    res = {name: _entry(per[name], calls[name][2]) for name in calls}
    for e in res.values():
        e["times_floor"] = e["median_us"] / e["hbm_floor_us"]
    return res


def _pictures16(H, W, depth):
    """[H, W, 3] int16-storage CUDA picture of `depth`-bit samples: the 8-bit synthetic picture scaled, plus low-order noise"""
    p8 = np.tile(_rgb_pictures(1080, 1920, 1)[0][0], (H // 1080, W // 1920, 1)).astype(np.uint16)
    s = 1 << (depth - 8)
    p = (p8 * s + np.random.default_rng(depth).integers(0, s, p8.shape)).astype(np.uint16)
    return torch.from_numpy(p.view(np.int16)).cuda()


def time_kernels(H, W, batch, reps, rounds):
    f_to_x8 = _lib.fn("dcvc_rgb_to_x_cs", ci, [vp, ll, ll, ll, ci, ci, vp, ci, vp, ci, ci, ci, vp])
    f_to_rgb8 = _lib.fn("dcvc_x_to_rgb_cs", ci, [vp, ci, ci, ci, vp, vp, ci, ci, ci, vp])
    f_to_x16 = _lib.fn("dcvc_rgb16_to_x_cs", ci, [vp, ll, ll, ll, ci, ci, ci, vp, ci, vp, ci, ci, ci, vp])
    f_to_rgb16 = _lib.fn("dcvc_x_to_rgb16_cs", ci, [vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, vp])
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    st = vp(torch.cuda.current_stream().cuda_stream)
    p = lambda t: vp(t.data_ptr())
    res = {}
    count = lambda nbytes: max(2, -(-(512 << 20) // nbytes))
    pic8 = torch.from_numpy(np.ascontiguousarray(np.tile(_rgb_pictures(1080, 1920, 1)[0][0], (H // 1080, W // 1920, 1)))).cuda()

    # to x: 3 HW (u8) or 6 HW (u16) in, 6 HW out
    calls, keep = {}, []
    n8 = count(9 * H * W)
    src8 = [pic8.clone() for _ in range(n8)]
    xs8 = [torch.empty((H, W, 3), dtype=torch.float16, device="cuda") for _ in range(n8)]
    calls["u8"] = (lambda k: _lib.check(f_to_x8(p(src8[k]), 3 * W, 3, 1, H, W, p(xs8[k]), 3, None, *COLOUR, st)), n8, 9 * H * W)
    n16 = count(12 * H * W)
    xs16 = [torch.empty((H, W, 3), dtype=torch.float16, device="cuda") for _ in range(n16)]
    for depth in (10, 16):
        pic = _pictures16(H, W, depth)
        srcs = [pic.clone() for _ in range(n16)]
        keep.append(srcs)
        calls["u16_%d" % depth] = (lambda k, srcs=srcs, depth=depth: _lib.check(
            f_to_x16(p(srcs[k]), 3 * W, 3, 1, depth, H, W, p(xs16[k]), 3, None, *COLOUR, st)), n16, 12 * H * W)
    res["to_x"] = _rounds(calls, batch, reps, rounds)
    x0 = xs16[0].clone()
    del calls, keep, src8, xs8, xs16
    torch.cuda.empty_cache()

    # from x: 6 Hp Wp in; 6 HW (fp16 planes) + 3 HW (u8) or 12 HW (fp32 planes) + 6 HW (u16) out
    xh = torch.zeros((Hp, Wp, 3), dtype=torch.float16, device="cuda")
    xh[:H, :W] = x0
    b8, b16 = 6 * Hp * Wp + 9 * H * W, 6 * Hp * Wp + 18 * H * W
    n8, n16 = count(b8), count(b16)
    xhs = [xh.clone() for _ in range(max(n8, n16))]
    r16 = [torch.empty((3, H, W), dtype=torch.float16, device="cuda") for _ in range(n8)]
    r8 = [torch.empty((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(n8)]
    d32 = [torch.empty((3, H, W), dtype=torch.float32, device="cuda") for _ in range(n16)]
    o16 = [torch.empty((H, W, 3), dtype=torch.int16, device="cuda") for _ in range(n16)]
    calls = {"u8": (lambda k: _lib.check(f_to_rgb8(p(xhs[k]), Wp, H, W, p(r16[k]), p(r8[k]), *COLOUR, st)), n8, b8)}
    for depth in (10, 16):
        calls["u16_%d" % depth] = (lambda k, depth=depth: _lib.check(
            f_to_rgb16(p(xhs[k]), Wp, H, W, depth, p(d32[k]), p(o16[k]), *COLOUR, st)), n16, b16)
    res["from_x"] = _rounds(calls, batch, reps, rounds)
    return res


def time_tool(pictures):
    H, W = 1080, 1920
    m = models.DMCI()
    m.load_state_dict(synthetic.synthetic_state_dict(arch.dmci_spec(), 0))
    m.update(0.15)
    pics = [p for p, _, _ in _rgb_pictures(H, W, pictures)]
    res = {"pictures": pictures, "stream": "1080p intra, synthetic weights, qp 32; rgb48 = the rgb24 pictures * 257 at 16 bits"}
    with tempfile.TemporaryDirectory() as d:
        j = lambda *a: os.path.join(d, *a)
        with open(j("in.rgb24"), "wb") as f8, open(j("in.rgb48"), "wb") as f16:
            for pic in pics:
                f8.write(pic.tobytes())
                f16.write((pic.astype(np.uint16) * 257).astype("<u2").tobytes())
        export_weights.write_dcvw(j("i.dcvw"), "dmci", m, 0.15)
        run = lambda a: subprocess.run([TOOL] + a, check=True, capture_output=True, text=True, timeout=600).stdout
        rate = lambda s: float(re.search(r"([0-9.]+) pictures/s", s).group(1))
        base = ["--intra", j("i.dcvw"), "-W", str(W), "-H", str(H)]
        enc = lambda t: ["encode"] + base + ["--src-type", t, "-i", j("in." + t), "--qp-i", "32", "-o", j(t + ".bin")]
        dec = lambda t: ["decode"] + base + ["--src-type", t, "-i", j(t + ".bin"), "--ref", j("in." + t), "--json", j(t + ".json")]
        modes = ("rgb24", "rgb48")
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
            res[t]["stream_bytes"] = os.path.getsize(j(t + ".bin"))
        for k in ("encode", "decode_ref_json"):
            res["rgb48"][k + "_vs_rgb24"] = res["rgb48"][k + "_median"] / res["rgb24"][k + "_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pictures", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgb16_bench needs the GPU")
    res = {"what": "dcvc_rgb16_to_x_cs / dcvc_x_to_rgb16_cs per picture at 10 and 16 bits next to dcvc_rgb_to_x_cs / dcvc_x_to_rgb_cs in "
                   "one run (HIP events, batches of back-to-back calls over > 512 MB of buffers, the variants taking turns), "
                   "times_floor = median / HBM floor of the bytes moved; dcvc encode / decode pictures/s, rgb48 against rgb24",
           "device": torch.cuda.get_device_name(0), "hbm_tbps": HBM_TBPS, "batch": a.batch, "reps": a.reps, "rounds": a.rounds,
           "1920x1080": time_kernels(1080, 1920, a.batch, a.reps, a.rounds),
           "3840x2160": time_kernels(2160, 3840, a.batch, a.reps, a.rounds),
           "tool": time_tool(a.pictures)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
