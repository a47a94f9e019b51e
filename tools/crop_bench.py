"""What black-bar cropping costs and gives, on one MI355X.

The kernels: microseconds per YUV420 picture, 1920x1080 and 3840x2160, u8 and 10-bit u16, letterboxed to 2.40:1 (1920x800,
3840x1600): dcvc_crop_stats on the luma plane alone (two launches); the two dcvc_window_planes calls of a crop (Y, then U and V:
the window out of the full picture); the two calls of a pad (the window back into a full picture, bars filled). Device events
around --pictures pictures after --warmup on one stream, two input pictures taking turns. Beside each figure, from the same
run: the time of a plain hipMemcpyAsync device-to-device copy of the bytes it moves (the measurement reads one luma plane: half
a plane is copied, which reads and writes a plane's worth; the crop reads and writes the window: the window's bytes are copied;
the pad reads the window and writes the full picture: their mean is copied), the floor the kernels are held against. The
variants take turns --repeats times; the table holds the median of each. The copy of the words to the host and the wait for
it, which the tool's probe needs, are not in these figures; the tool's figures below hold them.

The tool: pictures/s of dcvc encode - its own figure, file I/O included - for a 1080p synthetic yuv420 clip, LD with seeded
synthetic weights at a constant q_index: the clip letterboxed to 1920x800 without the flag and with --crop auto (what dropping
26 % of the samples gives), and the same clip without bars without the flag and with --crop auto (what the probe costs when it
finds nothing); one warm-up each and then --repeats rounds in turn. Nothing here is a target.

    python tools/crop_bench.py [--pictures 200] [--warmup 20] [--repeats 5] [--clip 48] [--out profiles/crop_bench.json]
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
SIZES = [(1080, 1920, 800), (2160, 3840, 1600)]          # H, W, the letterboxed height
KINDS = [("u8", 8), ("u16 10-bit", 10)]
LIMIT = 24


def _frame(np, H, W, inner, bits, seed):
    """one letterboxed picture [H * W * 3 / 2]: a smooth scene plus Gaussian noise of sigma 2 (8-bit code values) between bars"""
    rng = np.random.default_rng(seed)
    s = 1 << (bits - 8)
    planes = []
    for hh, ww, bar, black in ((H, W, (H - inner) // 2, 16), (H // 2, W // 2, (H - inner) // 4, 128), (H // 2, W // 2, (H - inner) // 4, 128)):
        yy, xx = np.mgrid[0:hh, 0:ww]
        clean = (128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)) * s
        clean[:bar], clean[hh - bar:] = black * s, black * s
        planes.append(np.clip(np.rint(clean + rng.normal(0, 2 * s, clean.shape)), 0, (1 << bits) - 1).ravel())
    return np.concatenate(planes).astype(np.uint8 if bits == 8 else np.int16)


def _kernel_bench(a, res):
    import numpy as np
    import torch
    from dcvc_amd import _lib
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    D2D = 3
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    stats_fn = _lib.fn("dcvc_crop_stats", ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp])
    window_fn = _lib.fn("dcvc_window_planes", ci, [vp, ci, ll, ci, ci, vp, ci, ll, ci, ci, ci, ci, ci, ci, ctypes.POINTER(ci), vp])
    stream = torch.cuda.current_stream()
    res["kernel"] = []
    for H, W, inner in SIZES:
        for name, bits in KINDS:
            es = 1 if bits == 8 else 2
            ny, nyi, bar = H * W, inner * W, (H - inner) // 2
            src = [torch.from_numpy(_frame(np, H, W, inner, bits, seed)).cuda() for seed in (1, 2)]
            small = torch.empty(nyi * 3 // 2, dtype=src[0].dtype, device="cuda")
            full = torch.empty_like(src[0])
            words = torch.empty(H + W, dtype=torch.int32, device="cuda")
            dt = 0 if bits == 8 else 3                              # DCVC_SAMPLE_U8 / DCVC_SAMPLE_U16
            st = vp(stream.cuda_stream)
            fy, fc = (ci * 1)(16 << (bits - 8)), (ci * 2)(128 << (bits - 8), 128 << (bits - 8))
            # the C entries themselves with their arguments made beforehand, as the tool calls them
            stats_calls, crop_calls = [], []
            for t in (0, 1):
                p, o = src[t].data_ptr(), small.data_ptr()
                stats_calls.append((vp(p), W, dt, bits, H, W, LIMIT, vp(words.data_ptr()), st))
                crop_calls.append(((vp(p), W, ny, H, W, vp(o), W, nyi, inner, W, dt, 1, 0, bar, fy, st),
                                   (vp(p + ny * es), W // 2, ny // 4, H // 2, W // 2, vp(o + nyi * es), W // 2, nyi // 4, inner // 2, W // 2, dt, 2, 0,
                                    bar // 2, fc, st)))
            o, p = small.data_ptr(), full.data_ptr()
            pad_calls = ((vp(o), W, nyi, inner, W, vp(p), W, ny, H, W, dt, 1, 0, -bar, fy, st),
                         (vp(o + nyi * es), W // 2, nyi // 4, inner // 2, W // 2, vp(p + ny * es), W // 2, ny // 4, H // 2, W // 2, dt, 2, 0,
                          -(bar // 2), fc, st))

            def stats(i):
                rc = stats_fn(*stats_calls[i & 1])
                assert rc == 0, rc

            def crop(i):
                for args in crop_calls[i & 1]:
                    rc = window_fn(*args)
                    assert rc == 0, rc

            def pad(i):
                for args in pad_calls:
                    rc = window_fn(*args)
                    assert rc == 0, rc

            crop(0)
            traffic = {"crop_stats": ny * es, "crop": 2 * (nyi * 3 // 2) * es, "pad": (nyi * 3 // 2 + ny * 3 // 2) * es}
            cs, cd = (torch.empty(max(traffic.values()) // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
            cs.zero_()

            def copy_of(nbytes):
                def copy(i):
                    rc = hip.hipMemcpyAsync(cd.data_ptr(), cs.data_ptr(), nbytes // 2, D2D, stream.cuda_stream)
                    assert rc == 0, rc
                return copy

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

            variants = {"crop_stats": stats, "crop": crop, "pad": pad}
            times = {k: [] for k in variants}
            copies = {k: [] for k in variants}
            for _ in range(a.repeats):
                for k, f in variants.items():
                    times[k].append(timed(f))
                    copies[k].append(timed(copy_of(traffic[k])))
            row = {"size": "%dx%d" % (W, H), "window": "%dx%d" % (W, inner), "samples": name}
            for k in variants:
                us, cu = float(np.median(times[k])), float(np.median(copies[k]))
                row[k] = {"bytes_moved": traffic[k], "us": times[k], "copy_us": copies[k], "us_median": us, "copy_us_median": cu,
                          "gb_s": traffic[k] / us / 1e3, "copy_gb_s": traffic[k] / cu / 1e3, "over_copy": us / cu}
            res["kernel"].append(row)
            print("%-10s %-11s " % (row["size"], name) + "  ".join("%s %7.1f us (%6.1f GB/s; copy %7.1f us, ratio %.2f)" % (
                k, row[k]["us_median"], row[k]["gb_s"], row[k]["copy_us_median"], row[k]["over_copy"]) for k in variants), flush=True)


def _run(args):
    r = subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=900)
    return float(re.search(r"([0-9.]+) pictures/s", r.stdout).group(1)), r.stdout


def _tool_bench(a, res):
    import numpy as np
    from dcvc_amd import arch, export_weights, models, synthetic
    H, W, inner = SIZES[0]
    bar = (H - inner) // 2
    with tempfile.TemporaryDirectory() as d:
        j = lambda *p: os.path.join(d, *p)      # noqa: E731
        with open(j("box.yuv"), "wb") as fb, open(j("full.yuv"), "wb") as ff:
            for i in range(a.clip):
                y, c = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=3)
                y, c = np.maximum(np.array(y, copy=True), 40).astype(np.uint8), np.array(c, copy=True).astype(np.uint8)
                ff.write(y.tobytes() + c.tobytes())
                y[:bar], y[H - bar:] = 16, 16
                c[:, :bar // 2], c[:, H // 2 - bar // 2:] = 128, 128
                fb.write(y.tobytes() + c.tobytes())
        for name, cls, spec in (("i", models.DMCI, arch.dmci_spec()), ("ld", models.DMC, arch.dmc_ld_spec())):
            m = cls()
            m.load_state_dict(synthetic.synthetic_state_dict(spec, 0))
            m.update(0.15)
            export_weights.write_dcvw(j(name + ".dcvw"), "dmci" if name == "i" else "ld", m, 0.15)
        base = ["encode", "--intra", j("i.dcvw"), "--inter", j("ld.dcvw"), "-W", str(W), "-H", str(H), "--qp-i", "40"]
        variants = {"letterboxed_plain": lambda: _run(base + ["-i", j("box.yuv"), "-o", j("a.bin")]),
                    "letterboxed_crop_auto": lambda: _run(base + ["-i", j("box.yuv"), "--crop", "auto", "-o", j("b.bin")]),
                    "no_bars_plain": lambda: _run(base + ["-i", j("full.yuv"), "-o", j("c.bin")]),
                    "no_bars_crop_auto": lambda: _run(base + ["-i", j("full.yuv"), "--crop", "auto", "-o", j("e.bin")])}
        runs = {v: [] for v in variants}
        summaries = {}
        for v, run in variants.items():        # warm-up
            m = re.search(r"crop: [^\n]*", run()[1])
            summaries[v] = m.group(0) if m else None
        for _ in range(a.repeats):             # alternating
            for v, run in variants.items():
                runs[v].append(run()[0])
        tool = {"what": "dcvc encode pictures/s (the tool's own figure, file I/O and the probe included), %dx%d yuv420 8-bit synthetic clip of %d "
                        "pictures, letterboxed to %dx%d and without bars, LD, synthetic weights, qp 40" % (W, H, a.clip, W, inner),
                "summaries": summaries, "bytes": {v: os.path.getsize(j(n)) for v, n in zip(variants, ("a.bin", "b.bin", "c.bin", "e.bin"))}}
        for v in variants:
            tool[v] = {"pictures_per_s": runs[v], "median": float(np.median(runs[v])), "min": min(runs[v]), "max": max(runs[v])}
            print("%-24s median %7.2f  min %7.2f  max %7.2f pictures/s" % (v, tool[v]["median"], tool[v]["min"], tool[v]["max"]), flush=True)
        tool["crop_vs_plain_letterboxed"] = tool["letterboxed_crop_auto"]["median"] / tool["letterboxed_plain"]["median"]
        tool["crop_vs_plain_no_bars"] = tool["no_bars_crop_auto"]["median"] / tool["no_bars_plain"]["median"]
        tool["samples_kept"] = inner / H
        tool["plain_spread"] = (tool["letterboxed_plain"]["max"] - tool["letterboxed_plain"]["min"]) / tool["letterboxed_plain"]["median"]
        res["tool"] = tool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clip", type=int, default=48)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("crop_bench needs the GPU: a time from anywhere else says nothing")
    res = {"what": "dcvc_crop_stats (limit %d) on the luma plane, the two dcvc_window_planes calls of a crop and the two of a pad, microseconds "
                   "per letterboxed yuv420 picture between device events over %d pictures after %d warm-up pictures, each beside a "
                   "hipMemcpyAsync device-to-device copy of the bytes it moves; medians of %d alternating rounds" % (LIMIT, a.pictures, a.warmup,
                                                                                                                   a.repeats),
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
