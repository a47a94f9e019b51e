"""What film grain costs, on one MI355X.

The kernels: microseconds per YUV420 picture of the two dcvc_grain_apply calls (Y, then U and V against the ungrained luma, into
a buffer of their own, as the decoder calls them) and of the two dcvc_grain_stats calls (Y, then U and V, accumulating, as the
encoder calls them), for 1920x1080 and 3840x2160, u8 and 10-bit u16 - device events around --pictures pictures after --warmup on
one stream. Beside each figure, from the same run: the time of a plain hipMemcpyAsync device-to-device copy of one picture, which
moves the bytes either pair of calls has to move (apply reads a picture and writes one; stats reads two), the floor they are held
against - the chroma calls' second read of the luma plane comes on top. The three take turns --repeats times; the table holds
the median of each.

The tool: pictures/s of dcvc - its own figure, file I/O included - for a 1080p synthetic yuv420 clip with seeded noise, LD with
seeded synthetic weights at a constant q_index: decode -o with and without --film-grain, encode --denoise 8 with and without
--grain-log, one warm-up each and then --repeats rounds in turn. Nothing here is a target.

    python tools/grain_bench.py [--pictures 200] [--warmup 20] [--repeats 5] [--clip 49] [--out profiles/grain_bench.json]
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


def _noisy(np, H, W, bits, seed):
    """one picture [H * W * 3 / 2] of a smooth scene plus Gaussian noise of sigma 3 (8-bit code values)"""
    rng = np.random.default_rng(seed)
    s = 1 << (bits - 8)
    planes = []
    for hh, ww in ((H, W), (H // 2, W // 2), (H // 2, W // 2)):
        yy, xx = np.mgrid[0:hh, 0:ww]
        clean = (128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)) * s
        planes.append(np.clip(np.rint(clean + rng.normal(0, 3 * s, clean.shape)), 0, (1 << bits) - 1).ravel())
    return np.concatenate(planes).astype(np.uint8 if bits == 8 else np.int16)


def _kernel_bench(a, res):
    import numpy as np
    import torch
    from dcvc_amd import denoise, grain
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    D2D = 3
    stream = torch.cuda.current_stream()
    vp, ci, ll, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint32
    apply_fn = grain._fn("dcvc_grain_apply", [vp, ci, ll, vp, ci, ci, ci, vp, ci, ll, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, ctypes.c_char_p,
                                              u32, u32, vp])
    stats_fn = grain._fn("dcvc_grain_stats", [vp, ci, ll, vp, ci, ll, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp])
    tpl = torch.tensor([grain.grain_template(1, p, 12) for p in range(3)], dtype=torch.int16).cuda()
    tp = [vp(tpl[p].data_ptr()) for p in range(3)]
    lut = bytes([16, 20, 24, 28, 32, 28, 24, 20, 16] * 3)
    res["kernel"] = []
    for H, W in SIZES:
        for name, bits in KINDS:
            es = 1 if bits == 8 else 2
            n, ny = H * W * 3 // 2, H * W
            dt = 0 if bits == 8 else 3                              # DCVC_SAMPLE_U8 / DCVC_SAMPLE_U16
            src = torch.from_numpy(_noisy(np, H, W, bits, 1)).cuda()
            den = torch.empty_like(src)
            denoise.denoise_planes(src[:ny].view(1, H, W), None, 8, 8, bits, out=den[:ny].view(1, H, W))
            denoise.denoise_planes(src[ny:].view(2, H // 2, W // 2), None, 8, 8, bits, out=den[ny:].view(2, H // 2, W // 2))
            out = torch.empty_like(src)
            words = torch.zeros(48, dtype=torch.int64, device="cuda")
            st = vp(stream.cuda_stream)
            r, d, o, s = den.data_ptr(), den.data_ptr(), out.data_ptr(), src.data_ptr()
            # the C entries themselves with their arguments made beforehand, as the tool calls them

            def apply(i):
                rc = apply_fn(vp(r), W, ny, vp(r), W, H, W, vp(o), W, ny, dt, bits, H, W, 1, 0, 0, 0, tp[0], tp[1], tp[2], lut, 1, i, st)
                rc |= apply_fn(vp(r + ny * es), W // 2, ny // 4, vp(r), W, H, W, vp(o + ny * es), W // 2, ny // 4, dt, bits, H // 2, W // 2, 2, 1,
                               1, 1, tp[0], tp[1], tp[2], lut, 1, i, st)
                assert rc == 0, rc

            def stats(i):
                acc = 1 if i % 8 else 0
                rc = stats_fn(vp(s), W, ny, vp(d), W, ny, vp(d), W, H, W, dt, bits, H, W, 1, 0, 0, 4, acc, vp(words.data_ptr()), st)
                rc |= stats_fn(vp(s + ny * es), W // 2, ny // 4, vp(d + ny * es), W // 2, ny // 4, vp(d), W, H, W, dt, bits, H // 2, W // 2, 2, 1, 1,
                               4, acc, vp(words.data_ptr() + 128), st)
                assert rc == 0, rc

            cd = torch.empty(n * es, dtype=torch.uint8, device="cuda")

            def copy(i):
                rc = hip.hipMemcpyAsync(cd.data_ptr(), s, n * es, D2D, stream.cuda_stream)
                assert rc == 0, rc

            def timed(fn):
                for i in range(a.warmup):
                    fn(i)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for i in range(a.pictures):
                    fn(i)
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) * 1000.0 / a.pictures     # microseconds per picture

            t = {"apply": [], "stats": [], "copy": []}
            for _ in range(a.repeats):
                t["apply"].append(timed(apply))
                t["stats"].append(timed(stats))
                t["copy"].append(timed(copy))
            traffic = 2 * n * es
            row = {"size": "%dx%d" % (W, H), "samples": name, "bytes_moved": traffic, "apply_us": t["apply"], "stats_us": t["stats"],
                   "copy_us": t["copy"]}
            for k in t:
                row[k + "_us_median"] = float(np.median(t[k]))
                row[k + "_gb_s"] = traffic / row[k + "_us_median"] / 1e3
            row["apply_over_copy"] = row["apply_us_median"] / row["copy_us_median"]
            row["stats_over_copy"] = row["stats_us_median"] / row["copy_us_median"]
            res["kernel"].append(row)
            print("%-10s %-11s apply %8.1f us (%7.1f GB/s)  stats %8.1f us (%7.1f GB/s)  copy %8.1f us (%7.1f GB/s)  apply / copy %.2f  "
                  "stats / copy %.2f" % (row["size"], name, row["apply_us_median"], row["apply_gb_s"], row["stats_us_median"], row["stats_gb_s"],
                                         row["copy_us_median"], row["copy_gb_s"], row["apply_over_copy"], row["stats_over_copy"]), flush=True)


def _run(args):
    r = subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=900)
    return float(re.search(r"([0-9.]+) pictures/s", r.stdout).group(1))


def _tool_bench(a, res):
    import numpy as np
    from dcvc_amd import arch, export_weights, models, synthetic
    H, W = SIZES[0]
    with tempfile.TemporaryDirectory() as d:
        j = lambda *p: os.path.join(d, *p)      # noqa: E731
        rng = np.random.default_rng(3)
        with open(j("in.yuv"), "wb") as f:
            for i in range(a.clip):
                y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=3)
                for p in (y, uv):
                    f.write(np.clip(np.rint(p + rng.normal(0, 3, p.shape)), 0, 255).astype(np.uint8).tobytes())
        for name, cls, spec in (("i", models.DMCI, arch.dmci_spec()), ("ld", models.DMC, arch.dmc_ld_spec())):
            m = cls()
            m.load_state_dict(synthetic.synthetic_state_dict(spec, 0))
            m.update(0.15)
            export_weights.write_dcvw(j(name + ".dcvw"), "dmci" if name == "i" else "ld", m, 0.15)
        mdl = ["--intra", j("i.dcvw"), "--inter", j("ld.dcvw")]
        enc = ["encode"] + mdl + ["-i", j("in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "40", "--denoise", "8"]
        dec = ["decode"] + mdl + ["-i", j("s.bin")]
        _run(enc + ["-o", j("s.bin"), "--grain-log", j("g.json")])
        variants = {"decode_plain": lambda: _run(dec + ["-o", j("a.yuv")]),
                    "decode_film_grain": lambda: _run(dec + ["--film-grain", j("g.json"), "-o", j("b.yuv")]),
                    "encode_denoise": lambda: _run(enc + ["-o", j("a.bin")]),
                    "encode_grain_log": lambda: _run(enc + ["--grain-log", j("h.json"), "-o", j("b.bin")])}
        runs = {v: [] for v in variants}
        for run in variants.values():          # warm-up
            run()
        for _ in range(a.repeats):             # alternating
            for v, run in variants.items():
                runs[v].append(run())
        tool = {"what": "dcvc pictures/s (the tool's own figure, file I/O included), %dx%d yuv420 8-bit synthetic clip plus noise of sigma 3, "
                        "%d pictures, LD, synthetic weights, qp 40; decode writes -o in both variants, encode runs --denoise 8 in both"
                        % (W, H, a.clip)}
        for v in variants:
            tool[v] = {"pictures_per_s": runs[v], "median": float(np.median(runs[v])), "min": min(runs[v]), "max": max(runs[v])}
            print("%-18s median %7.2f  min %7.2f  max %7.2f pictures/s" % (v, tool[v]["median"], tool[v]["min"], tool[v]["max"]), flush=True)
        for flagged, plain, key in (("decode_film_grain", "decode_plain", "decode"), ("encode_grain_log", "encode_denoise", "encode")):
            tool[key + "_flagged_vs_plain"] = tool[flagged]["median"] / tool[plain]["median"]
            tool[key + "_plain_spread"] = (tool[plain]["max"] - tool[plain]["min"]) / tool[plain]["median"]
        with open(j("g.json")) as f:
            tool["fitted_luma_table"] = json.load(f)["records"][0]["y"]
        res["tool"] = tool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clip", type=int, default=49)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("grain_bench needs the GPU: a time from anywhere else says nothing")
    res = {"what": "dcvc_grain_apply and dcvc_grain_stats, microseconds per yuv420 picture (Y call + U, V call each) between device events "
                   "over %d pictures after %d warm-up pictures, beside a hipMemcpyAsync device-to-device copy of one picture (the bytes "
                   "either pair has to move); medians of %d alternating rounds" % (a.pictures, a.warmup, a.repeats),
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
