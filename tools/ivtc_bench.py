"""What inverse telecine costs, on one MI355X.

The kernels: microseconds per YUV420 picture of what the tool enqueues for a frame that is not combed - dcvc_field_match on the
luma planes of two frames (two launches), then dcvc_weave_fields for Y and for U, V - for 1920x1080 and 3840x2160, u8 and 10-bit
u16: device events around --pictures pictures after --warmup on one stream, the two input frames, the two parities and the two
matches taking turns. Beside each figure, from the same run: the time of a plain hipMemcpyAsync device-to-device copy that moves
the same bytes (the measurement reads two luma planes, the weave reads 1.5 planes' worth and writes 1.5: 5 luma planes of
traffic, so 2.5 are copied), the floor the kernels are held against; and the measurement alone and the weave alone. The three
take turns --repeats times; the table holds the median of each. The copy of the words to the host and the wait for it, which
the tool needs before it can decide, are not in these figures; the tool's figures below hold them.

The tool: pictures/s of dcvc encode - its own figure, file I/O included - for a 1080p synthetic yuv420 clip carried by 2:3
pulldown, LD with seeded synthetic weights at a constant q_index, without the flag (every woven frame coded) and with --ivtc
film (four pictures from five frames), one warm-up each and then --repeats rounds in turn; and frames/s read, which is what a
capture pipeline has to keep up with. Nothing here is a target.

    python tools/ivtc_bench.py [--pictures 200] [--warmup 20] [--repeats 5] [--clip 100] [--out profiles/ivtc_bench.json]
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
CTHRESH = 9


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
    from dcvc_amd import _lib
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    D2D = 3
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    match_fn = _lib.fn("dcvc_field_match", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp])
    weave_fn = _lib.fn("dcvc_weave_fields", ci, [vp, ci, ll, vp, ci, ll, vp, ci, ll, ci, ci, ci, ci, ci, vp])
    stream = torch.cuda.current_stream()
    res["kernel"] = []
    for H, W in SIZES:
        for name, bits in KINDS:
            es = 1 if bits == 8 else 2
            n, ny = H * W * 3 // 2, H * W
            src = [torch.from_numpy(_frame(np, H, W, bits, seed)).cuda() for seed in (1, 2)]
            dst = torch.empty_like(src[0])
            words = torch.empty(8, dtype=torch.int64, device="cuda")
            dt = 0 if bits == 8 else 3                              # DCVC_SAMPLE_U8 / DCVC_SAMPLE_U16
            st = vp(stream.cuda_stream)
            # the C entries themselves with their arguments made beforehand, as the tool calls them
            match_calls, weave_calls = [], []
            for t in (0, 1):                                        # picture t: frame t against frame t ^ 1, first t, match c / p
                c, p, o = src[t].data_ptr(), src[t ^ 1].data_ptr(), dst.data_ptr()
                second = p if t else c
                match_calls.append((vp(c), W, vp(p), W, dt, bits, H, W, t, CTHRESH, vp(words.data_ptr()), st))
                weave_calls.append(((vp(c), W, ny, vp(second), W, ny, vp(o), W, ny, dt, H, W, 1, t, st),
                                    (vp(c + ny * es), W // 2, ny // 4, vp(second + ny * es), W // 2, ny // 4, vp(o + ny * es), W // 2, ny // 4, dt,
                                     H // 2, W // 2, 2, t, st)))

            def measure(i):
                rc = match_fn(*match_calls[i & 1])
                assert rc == 0, rc

            def weave(i):
                for args in weave_calls[i & 1]:
                    rc = weave_fn(*args)
                    assert rc == 0, rc

            def picture(i):
                measure(i)
                weave(i)

            traffic = (2 * ny + 2 * n) * es                         # two luma planes read; 1.5 planes read and 1.5 written
            half = traffic // 2
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

            k, c, m, w = [], [], [], []
            for _ in range(a.repeats):
                k.append(timed(picture))
                c.append(timed(copy))
                m.append(timed(measure))
                w.append(timed(weave))
            row = {"size": "%dx%d" % (W, H), "samples": name, "bytes_moved": traffic, "kernels_us": k, "copy_us": c, "field_match_us": m,
                   "weave_us": w, "kernels_us_median": float(np.median(k)), "copy_us_median": float(np.median(c)),
                   "field_match_us_median": float(np.median(m)), "weave_us_median": float(np.median(w))}
            row["kernels_gb_s"] = traffic / row["kernels_us_median"] / 1e3
            row["copy_gb_s"] = traffic / row["copy_us_median"] / 1e3
            row["kernels_over_copy"] = row["kernels_us_median"] / row["copy_us_median"]
            res["kernel"].append(row)
            print("%-10s %-11s match + weave %8.1f us (%7.1f GB/s)  copy %8.1f us (%7.1f GB/s)  ratio %.2f  match alone %8.1f us  weave alone %8.1f us"
                  % (row["size"], name, row["kernels_us_median"], row["kernels_gb_s"], row["copy_us_median"], row["copy_gb_s"],
                     row["kernels_over_copy"], row["field_match_us_median"], row["weave_us_median"]), flush=True)


def _run(args):
    r = subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=900)
    return float(re.search(r"([0-9.]+) pictures/s", r.stdout).group(1)), r.stdout


def _tool_bench(a, res):
    import numpy as np
    from dcvc_amd import arch, export_weights, models, synthetic
    H, W = SIZES[0]
    with tempfile.TemporaryDirectory() as d:
        j = lambda *p: os.path.join(d, *p)      # noqa: E731
        # 2:3 pulldown, top field first: film picture k shows its fields 2, 3, 2, 3, ... times
        fields = []
        parity, k = 0, 0
        while len(fields) < 2 * a.clip:
            for _ in range(2 if k % 2 == 0 else 3):
                fields.append((k, parity))
                parity ^= 1
            k += 1
        with open(j("in.yuv"), "wb") as f:
            for i in range(a.clip):
                (ka, _), (kb, _) = fields[2 * i], fields[2 * i + 1]
                (ya, ca), (yb, cb) = synthetic.synthetic_frame_yuv420(H, W, index=ka, seed=3), synthetic.synthetic_frame_yuv420(H, W, index=kb, seed=3)
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
                    "ivtc_film": lambda: _run(base + ["--ivtc", "film", "-o", j("b.bin")])}
        runs = {v: [] for v in variants}
        summary = ""
        for run in variants.values():          # warm-up
            summary = run()[1]
        for _ in range(a.repeats):             # alternating
            for v, run in variants.items():
                runs[v].append(run()[0])
        tool = {"what": "dcvc encode pictures/s (the tool's own figure, file I/O included), %dx%d yuv420 8-bit synthetic clip, %d frames carrying "
                        "%d film pictures by 2:3 pulldown top field first, LD, synthetic weights, qp 40" % (W, H, a.clip, fields[2 * a.clip - 1][0] + 1),
                "summary": re.search(r"ivtc: [^\n]*", summary).group(0)}
        pictures = int(re.search(r"(\d+) pictures from", tool["summary"]).group(1))
        for v in variants:
            tool[v] = {"pictures_per_s": runs[v], "median": float(np.median(runs[v])), "min": min(runs[v]), "max": max(runs[v])}
            print("%-18s median %7.2f  min %7.2f  max %7.2f pictures/s" % (v, tool[v]["median"], tool[v]["min"], tool[v]["max"]), flush=True)
        tool["ivtc_vs_plain_pictures_per_s"] = tool["ivtc_film"]["median"] / tool["plain"]["median"]
        # source frames a second: what a capture pipeline has to keep up with
        tool["ivtc_frames_per_s"] = tool["ivtc_film"]["median"] * a.clip / pictures
        tool["ivtc_vs_plain_frames_per_s"] = tool["ivtc_frames_per_s"] / tool["plain"]["median"]
        tool["plain_spread"] = (tool["plain"]["max"] - tool["plain"]["min"]) / tool["plain"]["median"]
        kernel_us = next(r["kernels_us_median"] for r in res["kernel"] if r["size"] == "%dx%d" % (W, H) and r["samples"] == "u8")
        tool["kernels_share_of_a_step"] = kernel_us * 1e-6 * tool["ivtc_film"]["median"]
        res["tool"] = tool


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clip", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ivtc_bench needs the GPU: a time from anywhere else says nothing")
    res = {"what": "dcvc_field_match (cthresh %d, with prev) + dcvc_weave_fields (Y call + U, V call), microseconds per yuv420 picture between "
                   "device events over %d pictures after %d warm-up pictures, beside a hipMemcpyAsync device-to-device copy moving the "
                   "same bytes (2.5 luma planes copied = 5 of traffic), the measurement alone and the weave alone; medians of %d "
                   "alternating rounds" % (CTHRESH, a.pictures, a.warmup, a.repeats),
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
