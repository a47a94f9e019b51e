"""Intra batches: pictures/s of the sequential compress-then-decompress loop (bench.py's definition of `value`)
for N pictures per DMCI call, on the seeded synthetic model with skip_thres 0.15 and q 0 / 32 / 63 in turn, as bench.py runs.

Per point: pictures/s, the gain over N = 1 and the host's entropy time per call, encode and decode (from DCVC_TIMING's lines
on stderr). Each point runs in a process of its own.

    python tools/intra_batch_bench.py [--steps 12] [--warmup 3] [--out profiles/intra_batch_bench.json] [--sizes 240x416,...]
"""
import argparse
import copy
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

POINTS = {(240, 416): (1, 2, 4, 8), (480, 832): (1, 2, 4, 8), (1080, 1920): (1, 2, 4, 8), (2160, 3840): (1, 2)}
QPS = (0, 32, 63)


def run_point(h, w, n, steps, warmup):
    import numpy as np
    import torch
    from codec_util import dmci_model, picture
    g = copy.deepcopy(dmci_model(skip_thres=0.15)).half().cuda()
    g.proxy = None
    p = g._ensure_proxy()
    x = torch.from_numpy(np.stack([picture(h, w, index=i) for i in range(n)])).permute(0, 3, 1, 2).cuda()
    x = x.contiguous(memory_format=torch.channels_last)
    pb, pr = (h + 15) // 16 * 16 - h, (w + 15) // 16 * 16 - w

    def step(i):
        qp = QPS[i % len(QPS)]
        if n == 1:
            bs, _, ec = p.compress(x, qp, pb, pr)
            p.decompress(bs, qp, h, w, ec)
        else:
            got = p.compress_batch(x, qp, pb, pr)
            p.decompress_batch([r[0] for r in got], qp, h, w, [r[2] for r in got])

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return steps * n / dt


def child(args):
    """one point per process (fresh device memory); DCVC_TIMING lines on stderr give the host entropy time"""
    h, w = map(int, args.point.split("x"))
    print(json.dumps({"pictures_per_s": run_point(h, w, args.n, args.steps, args.warmup)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intra_batch_bench.json"))
    ap.add_argument("--sizes", default="")
    ap.add_argument("--point", default="")
    ap.add_argument("--n", type=int, default=1)
    args = ap.parse_args()
    if args.point:
        return child(args)
    sizes = [tuple(map(int, s.split("x"))) for s in args.sizes.split(",")] if args.sizes else list(POINTS)
    rows = []
    for (h, w) in sizes:
        base = None
        for n in POINTS.get((h, w), (1, 2, 4, 8)):
            env = dict(os.environ, DCVC_TIMING="1")
            r = subprocess.run([sys.executable, __file__, "--point", "%dx%d" % (h, w), "--n", str(n), "--steps", str(args.steps),
                                "--warmup", str(args.warmup)], capture_output=True, text=True, env=env, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-3000:])
                raise SystemExit("point %dx%d N=%d failed (exit %d)" % (h, w, n, r.returncode))
            fps = json.loads(r.stdout.strip().splitlines()[-1])["pictures_per_s"]
            enc = [float(v) for v in re.findall(r"compress host entropy coding of \d+ pictures (\d+) us", r.stderr)]
            dec = [float(v) for v in re.findall(r"entropy decoding (\d+) us", r.stderr)]
            base = fps if n == 1 else base
            row = {"height": h, "width": w, "n": n, "pictures_per_s": round(fps, 1), "x_over_n1": round(fps / base, 2),
                   "host_entropy_decode_ms_per_call": round(sum(dec) / len(dec) / 1e3, 2) if dec else None,
                   "host_entropy_encode_ms_per_call": round(sum(enc) / len(enc) / 1e3, 2) if enc else None}
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"workload": "DMCI compress + decompress loop, synthetic seed 0, skip_thres 0.15, q 0/32/63",
                   "steps": args.steps, "warmup": args.warmup, "points": rows}, f, indent=1)


if __name__ == "__main__":
    main()
