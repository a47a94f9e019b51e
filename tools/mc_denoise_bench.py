"""What motion-compensated denoising costs, on one MI355X.

The kernels: microseconds per YUV420 picture for 1920x1080 and 3840x2160, u8 and 10-bit u16, of each part of what
dcvc encode --denoise 8 --denoise-mc 7 adds and runs - the search (dcvc_motion_search at range 7, lambda 4: two launches), the
two dcvc_motion_compensate_planes calls (Y; U and V), the two dcvc_denoise_planes calls at 8:8 reading the compensated picture,
and the five calls together - between device events around --pictures pictures after --warmup on one stream, the C entries with
their arguments made beforehand, as the tool calls them. Beside them, timed in the same run: a hipMemcpyAsync device-to-device
copy of one picture. The parts take turns --repeats times; the table holds the median, the smallest and the largest of each.
The pictures are a smooth scene panning by (3, 1) samples plus noise, so the vectors are not all zero.

The tool: pictures/s of dcvc encode - its own figure, file I/O included - for a 1080p synthetic yuv420 clip (a pan of (4, 2) a
picture) with seeded noise, LD with seeded synthetic weights at a constant q_index, with --denoise 8 alone and with
--denoise-mc 7 beside it, and - with --parent-tool - the dcvc binary of the parent commit with --denoise 8; one warm-up each and
then --repeats rounds in turn. Nothing here is a target.

    python tools/mc_denoise_bench.py [--pictures 100] [--warmup 10] [--repeats 5] [--clip 49] [--parent-tool PATH]
                                     [--out profiles/mc_denoise_bench.json]
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
RANGE, LAMBDA = 7, 4


def _noisy(np, H, W, bits, index, seed):
    """picture `index` [H * W * 3 / 2] of a smooth scene panning by (3, 1) samples a picture plus Gaussian noise of sigma 3"""
    rng = np.random.default_rng(seed)
    s = 1 << (bits - 8)
    planes = []
    for hh, ww, sub in ((H, W, 1), (H // 2, W // 2, 2), (H // 2, W // 2, 2)):
        yy, xx = np.mgrid[0:hh, 0:ww]
        yy, xx = yy + index * 1.0 / sub, xx + index * 3.0 / sub
        clean = (128 + 60 * np.sin(xx * sub / 9.0) * np.cos(yy * sub / 7.0) + 40 * (((xx * sub) // 16 + (yy * sub) // 16) % 2)) * s
        planes.append(np.clip(np.rint(clean + rng.normal(0, 3 * s, clean.shape)), 0, (1 << bits) - 1).ravel())
    return np.concatenate(planes).astype(np.uint8 if bits == 8 else np.int16)


def _kernel_bench(a, res):
    import numpy as np
    import torch
    from dcvc_amd import denoise, motion
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    D2D = 3
    stream = torch.cuda.current_stream()
    vp = ctypes.c_void_p
    st = vp(stream.cuda_stream)
    res["kernel"] = []
    for H, W in SIZES:
        for name, bits in KINDS:
            es = 1 if bits == 8 else 2
            n, ny = H * W * 3 // 2, H * W
            src = [torch.from_numpy(_noisy(np, H, W, bits, i, seed=i + 1)).cuda() for i in (0, 1)]
            hist = [torch.empty_like(src[0]) for _ in range(2)]
            comp = torch.empty_like(src[0])
            Bh, Bw = motion.grid(H, W)
            mv = torch.zeros((Bh, Bw, 2), dtype=torch.int16, device="cuda")
            sad = torch.zeros((Bh, Bw), dtype=torch.int32, device="cuda")
            moved = torch.zeros(1, dtype=torch.int32, device="cuda")
            need = motion._fn("dcvc_motion_search_workspace_bytes")(H, W)
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            f_search, f_comp, f_dn = motion._fn("dcvc_motion_search"), motion._fn("dcvc_motion_compensate_planes"), denoise._fn()
            dt = 0 if bits == 8 else 3                              # DCVC_SAMPLE_U8 / DCVC_SAMPLE_U16
            m, c = mv.data_ptr(), comp.data_ptr()
            parts = []
            for t in (0, 1):
                s, p, o = src[t].data_ptr(), hist[t ^ 1].data_ptr(), hist[t].data_ptr()
                parts.append({
                    "search": [(f_search, (vp(s), W, vp(p), W, dt, bits, H, W, RANGE, LAMBDA, vp(m), Bh, Bw, vp(sad.data_ptr()),
                                           vp(moved.data_ptr()), vp(ws.data_ptr()), need, st))],
                    "compensate": [(f_comp, (vp(p), W, ny, vp(c), W, ny, dt, H, W, 1, 0, 0, vp(m), Bh, Bw, st)),
                                   (f_comp, (vp(p + ny * es), W // 2, ny // 4, vp(c + ny * es), W // 2, ny // 4, dt, H // 2, W // 2, 2, 1, 1,
                                             vp(m), Bh, Bw, st))],
                    "denoise": [(f_dn, (vp(s), W, ny, vp(c), W, ny, vp(o), W, ny, dt, bits, H, W, 1, 8, 8, st)),
                                (f_dn, (vp(s + ny * es), W // 2, ny // 4, vp(c + ny * es), W // 2, ny // 4, vp(o + ny * es), W // 2, ny // 4, dt,
                                        bits, H // 2, W // 2, 2, 8, 8, st))]})
            hist[1].copy_(src[1])                                   # the first picture's history
            cs, cd = (torch.empty(n * es, dtype=torch.uint8, device="cuda") for _ in range(2))
            cs.zero_()

            def part(names):
                def run(i):
                    for k in names:
                        for fn, args in parts[i & 1][k]:
                            rc = fn(*args)
                            assert rc == 0, rc
                return run

            def copy(i):
                rc = hip.hipMemcpyAsync(cd.data_ptr(), cs.data_ptr(), n * es, D2D, stream.cuda_stream)
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

            what = {"search": part(["search"]), "compensate": part(["compensate"]), "denoise": part(["denoise"]),
                    "all": part(["search", "compensate", "denoise"]), "copy": copy}
            part(["search", "compensate", "denoise"])(0)            # the vectors and the compensated picture of the parts run alone
            times = {k: [] for k in what}
            for _ in range(a.repeats):
                for k, fn in what.items():
                    times[k].append(timed(fn))
            stream.synchronize()
            v = mv.cpu().numpy()
            row = {"size": "%dx%d" % (W, H), "samples": name, "picture_bytes": n * es, "blocks": Bh * Bw,
                   "blocks_moved": int(v.any(axis=-1).sum())}
            for k in what:
                row[k + "_us"] = times[k]
                row[k + "_us_median"] = float(np.median(times[k]))
            row["copy_gb_s"] = 2 * n * es / row["copy_us_median"] / 1e3
            row["search_over_copy"] = row["search_us_median"] / row["copy_us_median"]
            row["all_over_denoise"] = row["all_us_median"] / row["denoise_us_median"]
            res["kernel"].append(row)
            print("%-10s %-11s search %7.1f (%.1f..%.1f)  compensate %7.1f  denoise %7.1f  all %7.1f  copy %7.1f us (%6.1f GB/s)  moved %d / %d"
                  % (row["size"], name, row["search_us_median"], min(times["search"]), max(times["search"]), row["compensate_us_median"],
                     row["denoise_us_median"], row["all_us_median"], row["copy_us_median"], row["copy_gb_s"], row["blocks_moved"], Bh * Bw),
                  flush=True)


def _run(tool, args):
    r = subprocess.run([tool] + args, check=True, capture_output=True, text=True, timeout=900)
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
        base = ["encode", "--intra", j("i.dcvw"), "--inter", j("ld.dcvw"), "-i", j("in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "40"]
        variants = {"denoise_8": lambda: _run(TOOL, base + ["--denoise", "8", "-o", j("a.bin")]),
                    "denoise_8_mc_7": lambda: _run(TOOL, base + ["--denoise", "8", "--denoise-mc", str(RANGE), "-o", j("b.bin")])}
        if a.parent_tool:
            variants["parent_denoise_8"] = lambda: _run(a.parent_tool, base + ["--denoise", "8", "-o", j("c.bin")])
        runs = {v: [] for v in variants}
        for run in variants.values():          # warm-up
            run()
        for _ in range(a.repeats):             # taking turns
            for v, run in variants.items():
                runs[v].append(run())
        tool = {"what": "dcvc encode pictures/s (the tool's own figure, file I/O included), %dx%d yuv420 8-bit synthetic clip panning by "
                        "(4, 2) a picture plus noise of sigma 3, %d pictures, LD, synthetic weights, qp 40" % (W, H, a.clip)}
        for v in variants:
            tool[v] = {"pictures_per_s": runs[v], "median": float(np.median(runs[v])), "min": min(runs[v]), "max": max(runs[v])}
            print("%-17s median %7.2f  min %7.2f  max %7.2f pictures/s" % (v, tool[v]["median"], tool[v]["min"], tool[v]["max"]), flush=True)
        tool["mc_vs_denoise"] = tool["denoise_8_mc_7"]["median"] / tool["denoise_8"]["median"]
        if a.parent_tool:
            tool["denoise_vs_parent"] = tool["denoise_8"]["median"] / tool["parent_denoise_8"]["median"]
        tool["denoise_spread"] = (tool["denoise_8"]["max"] - tool["denoise_8"]["min"]) / tool["denoise_8"]["median"]
        res["tool"] = tool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clip", type=int, default=49)
    ap.add_argument("--parent-tool", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mc_denoise_bench needs the GPU: a time from anywhere else says nothing")
    res = {"what": "dcvc_motion_search (range %d, lambda %d), dcvc_motion_compensate_planes (Y call + U, V call) and dcvc_denoise_planes at 8:8 "
                   "on the compensated picture (Y call + U, V call), microseconds per yuv420 picture between device events over %d pictures "
                   "after %d warm-up pictures, beside a hipMemcpyAsync device-to-device copy of one picture; %d rounds taking turns"
                   % (RANGE, LAMBDA, a.pictures, a.warmup, a.repeats),
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
