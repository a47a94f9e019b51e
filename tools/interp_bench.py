"""What frame-rate conversion costs, on one MI355X.

The kernels: microseconds per YUV420 picture for 1920x1080 and 3840x2160, u8 and 10-bit u16, of each part of what
dcvc decode --interpolate 2 runs per in-between picture - the search (dcvc_motion_search at range 7, lambda 4: two launches, once
a pair of pictures), one dcvc_interp_select at limit 8, the two dcvc_interp_planes calls (Y; U and V) with the picture rule's
counter, and the four calls together - between device events around --pictures pictures after --warmup on one stream, the C
entries with their arguments made beforehand, as the tool calls them. Beside them, timed in the same run: a hipMemcpyAsync
device-to-device copy of one picture. The parts take turns --repeats times; the table holds the median, the smallest and the
largest of each. The pictures are a smooth scene panning by (6, 2) samples plus noise, so the vectors are not zero and the blocks
agree.

The tool: pictures/s of dcvc decode - its own figure over decoded pictures, file I/O included - for a 1080p synthetic yuv420
clip (a pan of (4, 2) a picture), LD with seeded synthetic weights at a constant q_index, without the flag and with
--interpolate 2, both writing -o, and - with --parent-tool - the dcvc binary of the parent commit without the flag; one warm-up
each and then --repeats rounds in turn. Nothing here is a target.

    python tools/interp_bench.py [--pictures 100] [--warmup 10] [--repeats 5] [--clip 49] [--parent-tool PATH]
                                 [--out profiles/interp_bench.json]
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
RANGE, LAMBDA, LIMIT, N, K = 7, 4, 8, 2, 1


def _noisy(np, H, W, bits, index, seed):
    """picture `index` [H * W * 3 / 2] of a smooth scene panning by (6, 2) samples a picture plus Gaussian noise of sigma 2"""
    rng = np.random.default_rng(seed)
    s = 1 << (bits - 8)
    planes = []
    for hh, ww, sub in ((H, W, 1), (H // 2, W // 2, 2), (H // 2, W // 2, 2)):
        yy, xx = np.mgrid[0:hh, 0:ww]
        yy, xx = yy + index * 2.0 / sub, xx + index * 6.0 / sub
        clean = (128 + 60 * np.sin(xx * sub / 9.0) * np.cos(yy * sub / 7.0) + 40 * (((xx * sub) // 16 + (yy * sub) // 16) % 2)) * s
        planes.append(np.clip(np.rint(clean + rng.normal(0, 2 * s, clean.shape)), 0, (1 << bits) - 1).ravel())
    return np.concatenate(planes).astype(np.uint8 if bits == 8 else np.int16)


def _kernel_bench(a, res):
    import numpy as np
    import torch
    from dcvc_amd import interp, motion
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
            pa, pb = (torch.from_numpy(_noisy(np, H, W, bits, i, seed=i + 1)).cuda() for i in (0, 1))
            mid = torch.empty_like(pa)
            Bh, Bw = motion.grid(H, W)
            mv = torch.zeros((Bh, Bw, 2), dtype=torch.int16, device="cuda")
            plan = torch.zeros((Bh, Bw, 4), dtype=torch.int16, device="cuda")
            wb = torch.zeros((Bh, Bw), dtype=torch.uint8, device="cuda")
            fallen = torch.zeros(1, dtype=torch.int32, device="cuda")
            need = motion._fn("dcvc_motion_search_workspace_bytes")(H, W)
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            f_search, f_select, f_planes = motion._fn("dcvc_motion_search"), interp._fn("dcvc_interp_select"), interp._fn("dcvc_interp_planes")
            dt = 0 if bits == 8 else 3                              # DCVC_SAMPLE_U8 / DCVC_SAMPLE_U16
            A, B, M = pa.data_ptr(), pb.data_ptr(), mid.data_ptr()
            p, w_, f = vp(plan.data_ptr()), vp(wb.data_ptr()), vp(fallen.data_ptr())
            parts = {
                "search": [(f_search, (vp(B), W, vp(A), W, dt, bits, H, W, RANGE, LAMBDA, vp(mv.data_ptr()), Bh, Bw, None, None,
                                       vp(ws.data_ptr()), need, st))],
                "select": [(f_select, (vp(A), W, vp(B), W, dt, bits, H, W, vp(mv.data_ptr()), Bh, Bw, K, N, LIMIT, p, w_, Bh, Bw, None, f, st))],
                "interp": [(f_planes, (vp(A), W, ny, vp(B), W, ny, vp(M), W, ny, dt, H, W, 1, 0, 0, p, w_, Bh, Bw, K, N, f, Bh * Bw, st)),
                           (f_planes, (vp(A + ny * es), W // 2, ny // 4, vp(B + ny * es), W // 2, ny // 4, vp(M + ny * es), W // 2, ny // 4, dt,
                                       H // 2, W // 2, 2, 1, 1, p, w_, Bh, Bw, K, N, f, Bh * Bw, st))]}
            cs, cd = (torch.empty(n * es, dtype=torch.uint8, device="cuda") for _ in range(2))
            cs.zero_()

            def part(names):
                def run(i):
                    for k in names:
                        if k == "select":
                            fallen.zero_()                          # the tool's hipMemsetAsync of the counter
                        for fn, args in parts[k]:
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

            what = {"search": part(["search"]), "select": part(["select"]), "interp": part(["interp"]),
                    "all": part(["search", "select", "interp"]), "copy": copy}
            part(["search", "select", "interp"])(0)                 # the vectors and the plan of the parts run alone
            times = {k: [] for k in what}
            for _ in range(a.repeats):
                for k, fn in what.items():
                    times[k].append(timed(fn))
            stream.synchronize()
            v = mv.cpu().numpy()
            row = {"size": "%dx%d" % (W, H), "samples": name, "picture_bytes": n * es, "blocks": Bh * Bw,
                   "blocks_moved": int(v.any(axis=-1).sum()), "blocks_fallen": int(fallen.item())}
            for k in what:
                row[k + "_us"] = times[k]
                row[k + "_us_median"] = float(np.median(times[k]))
            row["copy_gb_s"] = 2 * n * es / row["copy_us_median"] / 1e3
            row["interp_over_copy"] = row["interp_us_median"] / row["copy_us_median"]
            row["select_over_search"] = row["select_us_median"] / row["search_us_median"]
            res["kernel"].append(row)
            print("%-10s %-11s search %7.1f (%.1f..%.1f)  select %7.1f  interp %7.1f  all %7.1f  copy %7.1f us (%6.1f GB/s)  moved %d, fallen %d / %d"
                  % (row["size"], name, row["search_us_median"], min(times["search"]), max(times["search"]), row["select_us_median"],
                     row["interp_us_median"], row["all_us_median"], row["copy_us_median"], row["copy_gb_s"], row["blocks_moved"],
                     row["blocks_fallen"], Bh * Bw), flush=True)


def _run(tool, args):
    r = subprocess.run([tool] + args, check=True, capture_output=True, text=True, timeout=900)
    return float(re.search(r"([0-9.]+) pictures/s", r.stdout).group(1))


def _tool_bench(a, res):
    import numpy as np
    from dcvc_amd import arch, export_weights, models, synthetic
    H, W = SIZES[0]
    with tempfile.TemporaryDirectory() as d:
        j = lambda *p: os.path.join(d, *p)      # noqa: E731
        with open(j("in.yuv"), "wb") as f:
            for i in range(a.clip):
                y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=3)
                for p in (y, uv):
                    f.write(p.astype(np.uint8).tobytes())
        for name, cls, spec in (("i", models.DMCI, arch.dmci_spec()), ("ld", models.DMC, arch.dmc_ld_spec())):
            m = cls()
            m.load_state_dict(synthetic.synthetic_state_dict(spec, 0))
            m.update(0.15)
            export_weights.write_dcvw(j(name + ".dcvw"), "dmci" if name == "i" else "ld", m, 0.15)
        model = ["--intra", j("i.dcvw"), "--inter", j("ld.dcvw")]
        subprocess.run([TOOL, "encode"] + model + ["-i", j("in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "40", "-o", j("s.bin")], check=True,
                       capture_output=True, timeout=900)
        base = ["decode"] + model + ["-i", j("s.bin")]
        variants = {"plain": lambda: _run(TOOL, base + ["-o", j("a.yuv")]),
                    "interpolate_2": lambda: _run(TOOL, base + ["--interpolate", str(N), "-o", j("b.yuv")])}
        if a.parent_tool:
            variants["parent_plain"] = lambda: _run(a.parent_tool, base + ["-o", j("c.yuv")])
        runs = {v: [] for v in variants}
        for run in variants.values():          # warm-up
            run()
        for _ in range(a.repeats):             # taking turns
            for v, run in variants.items():
                runs[v].append(run())
        tool = {"what": "dcvc decode pictures/s over decoded pictures (the tool's own figure, file I/O included; --interpolate 2 writes twice "
                        "the pictures less one), %dx%d yuv420 8-bit synthetic clip panning by (4, 2) a picture, %d pictures, LD, synthetic "
                        "weights, qp 40, -o to a file" % (W, H, a.clip)}
        for v in variants:
            tool[v] = {"pictures_per_s": runs[v], "median": float(np.median(runs[v])), "min": min(runs[v]), "max": max(runs[v])}
            print("%-14s median %7.2f  min %7.2f  max %7.2f pictures/s" % (v, tool[v]["median"], tool[v]["min"], tool[v]["max"]), flush=True)
        tool["interpolate_vs_plain"] = tool["interpolate_2"]["median"] / tool["plain"]["median"]
        if a.parent_tool:
            tool["plain_vs_parent"] = tool["plain"]["median"] / tool["parent_plain"]["median"]
        tool["plain_spread"] = (tool["plain"]["max"] - tool["plain"]["min"]) / tool["plain"]["median"]
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
        raise SystemExit("interp_bench needs the GPU: a time from anywhere else says nothing")
    res = {"what": "dcvc_motion_search (range %d, lambda %d), dcvc_interp_select (k %d of n %d, limit %d) and dcvc_interp_planes (Y call + U, V "
                   "call, with the counter), microseconds per yuv420 picture between device events over %d pictures after %d warm-up "
                   "pictures, beside a hipMemcpyAsync device-to-device copy of one picture; %d rounds taking turns"
                   % (RANGE, LAMBDA, K, N, LIMIT, a.pictures, a.warmup, a.repeats),
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
