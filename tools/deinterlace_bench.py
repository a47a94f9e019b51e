"""What the deinterlacer costs, on one MI355X.

The kernel: microseconds per YUV420 picture (two dcvc_deinterlace_planes calls: Y, then U and V) with history at threshold 10,
for 1920x1080 and 3840x2160, u8 and 10-bit u16 - device events around --pictures pictures after --warmup on one stream, the two
input frames and the two parities taking turns as in the tool's field mode - and the bytes it has to move (two pictures read,
one written) per second. Beside each figure, from the same run: the time of plain hipMemcpyAsync device-to-device copies that
move the same bytes (one copy of 1.5 pictures reads 1.5 and writes 1.5), the floor the kernel is held against. Kernel and copy
take turns --repeats times; the table holds the median of each. The spatial-only launch (no history: one picture's kept rows
read, one picture written) is timed the same way beside them.

The tool: pictures/s of dcvc encode - its own figure, file I/O included - for a 1080p synthetic yuv420 clip woven from twice as
many pictures, LD with seeded synthetic weights at a constant q_index, with and without --deinterlace frame, one warm-up each and
then --repeats rounds in turn; and the kernel's share of an encode step. Nothing here is a target.

    python tools/deinterlace_bench.py [--pictures 200] [--warmup 20] [--repeats 5] [--clip 97] [--out profiles/deinterlace_bench.json]
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
SIZES = [(1080, 1920), (2160, 3840)]
KINDS = [("u8", 8), ("u16 10-bit", 10)]
THRESHOLD = 10


def _frame(np, H, W, bits, seed):
    """one picture [H * W * 3 / 2] of a smooth scene plus Gaussian noise of sigma 2 (8-bit code values)"""
    rng = np.random.default_rng(seed)
    s = 1 << (bits - 8)
    planes = []
    for hh, ww in ((H, W), (H // 2, W // 2), (H // 2, W // 2)):
        yy, xx = np.mgrid[0:hh, 0:ww]
        clean = (128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)) * s
        planes.append(np.clip(np.rint(clean + rng.normal(0, 2 * s, clean.shape)), 0, (1 << bits) - 1).ravel())
    return np.concatenate(planes).astype(np.uint8 if bits == 8 else np.int16)


def _kernel_bench(a, res):
    import numpy as np
    import torch
    from dcvc_amd import deinterlace
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    D2D = 3
    stream = torch.cuda.current_stream()
    res["kernel"] = []
    for H, W in SIZES:
        for name, bits in KINDS:
            es = 1 if bits == 8 else 2
            n = H * W * 3 // 2
            src = [torch.from_numpy(_frame(np, H, W, bits, seed)).cuda() for seed in (1, 2)]
            dst = torch.empty_like(src[0])
            ny = H * W
            # the C entry itself with its arguments made beforehand, as the tool calls it: the wrapper's checks would add host
            # time between the launches of a picture
            fn, vp = deinterlace._fn(), ctypes.c_void_p
            dt = 0 if bits == 8 else 3                              # DCVC_SAMPLE_U8 / DCVC_SAMPLE_U16
            st = vp(stream.cuda_stream)

            def calls_for(history):
                calls = []
                for t in (0, 1):                                    # picture t: frame t against frame t ^ 1, keep t, weave t ^ 1
                    c, p, o = src[t].data_ptr(), src[t ^ 1].data_ptr() if history else 0, dst.data_ptr()
                    pv = (lambda off: vp(p + off)) if history else (lambda off: None)
                    calls.append(((vp(c), W, ny, pv(0), W, ny, vp(o), W, ny, dt, bits, H, W, 1, t, t ^ 1, THRESHOLD, st),
                                  (vp(c + ny * es), W // 2, ny // 4, pv(ny * es), W // 2, ny // 4, vp(o + ny * es), W // 2, ny // 4, dt, bits,
                                   H // 2, W // 2, 2, t, t ^ 1, THRESHOLD, st)))
                return calls

            with_history, spatial_only = calls_for(True), calls_for(False)

            def picture(i, calls=with_history):
                for args in calls[i & 1]:
                    rc = fn(*args)
                    assert rc == 0, rc

            def bob(i):
                picture(i, spatial_only)

            half = n * es * 3 // 2                                  # bytes of 1.5 pictures
            cs, cd = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
            cs.zero_()

            def copy(i):
                rc = hip.hipMemcpyAsync(cd.data_ptr(), cs.data_ptr(), half, D2D, stream.cuda_stream)
                assert rc == 0, rc

            def timed(f):
                for i in range(a.warmup):
                    f(i)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for i in range(a.pictures):
                    f(i)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) * 1000.0 / a.pictures     # microseconds per picture

            k, c, b = [], [], []
            for _ in range(a.repeats):
                k.append(timed(picture))
                c.append(timed(copy))
                b.append(timed(bob))
            traffic = 3 * n * es
            row = {"size": "%dx%d" % (W, H), "samples": name, "bytes_moved": traffic, "kernel_us": k, "copy_us": c, "spatial_only_us": b,
                   "kernel_us_median": float(np.median(k)), "copy_us_median": float(np.median(c)),
                   "spatial_only_us_median": float(np.median(b)), "spatial_only_bytes_moved": n * es * 3 // 2}
            row["kernel_gb_s"] = traffic / row["kernel_us_median"] / 1e3
            row["copy_gb_s"] = traffic / row["copy_us_median"] / 1e3
            row["kernel_over_copy"] = row["kernel_us_median"] / row["copy_us_median"]
            res["kernel"].append(row)
            print("%-10s %-11s kernel %8.1f us (%7.1f GB/s)  copy %8.1f us (%7.1f GB/s)  kernel / copy %.2f  spatial only %8.1f us"
                  % (row["size"], name, row["kernel_us_median"], row["kernel_gb_s"], row["copy_us_median"], row["copy_gb_s"],
                     row["kernel_over_copy"], row["spatial_only_us_median"]), flush=True)


def _run(args):
    r = subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=900)
    return float(re.search(r"([0-9.]+) pictures/s", r.stdout).group(1))


def _tool_bench(a, res):
    import numpy as np
    from dcvc_amd import arch, export_weights, models, synthetic
    H, W = SIZES[0]
    with tempfile.TemporaryDirectory() as d:
        j = lambda *p: os.path.join(d, *p)      # noqa: E731
        with open(j("in.yuv"), "wb") as f:
            for i in range(a.clip):
                # a frame woven from two pictures of the sequence, top field first; chroma rows alternate as luma rows do
                (ya, ca), (yb, cb) = (synthetic.synthetic_frame_yuv420(H, W, index=2 * i + k, seed=3) for k in (0, 1))
                for p, q in ((ya, yb), (ca, cb)):
                    wv = np.array(p, copy=True)
                    wv[..., 1::2, :] = q[..., 1::2, :]
                    f.write(wv.astype(np.uint8).tobytes())
        for name, cls, spec in (("i", models.DMCI, arch.dmci_spec()), ("ld", models.DMC, arch.dmc_ld_spec())):
            m = cls()
            m.load_state_dict(synthetic.synthetic_state_dict(spec, 0))
            m.update(0.15)
            export_weights.write_dcvw(j(name + ".dcvw"), "dmci" if name == "i" else "ld", m, 0.15)
        base = ["encode", "--intra", j("i.dcvw"), "--inter", j("ld.dcvw"), "-i", j("in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "40"]
        variants = {"plain": lambda: _run(base + ["-o", j("a.bin")]),
                    "deinterlace_frame": lambda: _run(base + ["--deinterlace", "frame", "-o", j("b.bin")])}
        runs = {v: [] for v in variants}
        for run in variants.values():          # warm-up
            run()
        for _ in range(a.repeats):             # alternating
            for v, run in variants.items():
                runs[v].append(run())
        tool = {"what": "dcvc encode pictures/s (the tool's own figure, file I/O included), %dx%d yuv420 8-bit synthetic clip woven top field "
                        "first from %d pictures, %d frames, LD, synthetic weights, qp 40" % (W, H, 2 * a.clip, a.clip)}
        for v in variants:
            tool[v] = {"pictures_per_s": runs[v], "median": float(np.median(runs[v])), "min": min(runs[v]), "max": max(runs[v])}
            print("%-18s median %7.2f  min %7.2f  max %7.2f pictures/s" % (v, tool[v]["median"], tool[v]["min"], tool[v]["max"]), flush=True)
        tool["deinterlace_vs_plain"] = tool["deinterlace_frame"]["median"] / tool["plain"]["median"]
        tool["plain_spread"] = (tool["plain"]["max"] - tool["plain"]["min"]) / tool["plain"]["median"]
        kernel_us = next(r["kernel_us_median"] for r in res["kernel"] if r["size"] == "%dx%d" % (W, H) and r["samples"] == "u8")
        tool["kernel_share_of_a_step"] = kernel_us * 1e-6 * tool["deinterlace_frame"]["median"]
        res["tool"] = tool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clip", type=int, default=97)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("deinterlace_bench needs the GPU: a time from anywhere else says nothing")
    res = {"what": "dcvc_deinterlace_planes at threshold %d with history, microseconds per yuv420 picture (Y call + U, V call) between "
                   "device events over %d pictures after %d warm-up pictures, beside hipMemcpyAsync device-to-device copies moving the "
                   "same bytes (1.5 pictures copied = 3 pictures of traffic) and the spatial-only launch (no history); medians of %d "
                   "alternating rounds" % (THRESHOLD, a.pictures, a.warmup, a.repeats),
           "device": torch.cuda.get_device_name(0), "pictures": a.pictures, "warmup": a.warmup, "repeats": a.repeats}
    _kernel_bench(a, res)
    _tool_bench(a, res)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
