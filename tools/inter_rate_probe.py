"""The size probe of the inter codecs against compress: milliseconds per call of estimate_bits and of
compress on the same unit and q_index for LD, HT-S and HT-L, medians after warm-up, on the seeded synthetic models with
skip_thres 0.15; the prediction next to the stream each compress wrote; and, with --intra 1, the same for the intra codec.

compress advances the temporal state, the probe does not. The state both are timed against is that of a running GOP -
add_ref and one P unit - exported once and imported again, outside the timed span, before every compress: a seeded
synthetic model that codes one unit again and again against its own output leaves the range pictures give it.

    python tools/inter_rate_probe.py [--size 1080x1920] [--models ld,hts,htl] [--qps 21,42] [--calls 16] [--warmup 4]
                                     [--intra 1] [--out FILE.json]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--models", default="ld,hts,htl")
    ap.add_argument("--qps", default="21,42")
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--intra", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from codec_util import chunk, dmc_ht_model, dmc_ld_model, dmci_model, picture, to_device_input
    from dcvc_amd import rate_control as rc
    h, w = map(int, args.size.split("x"))
    pb, pr = -h % 16, -w % 16
    qps = [int(q) for q in args.qps.split(",")]

    def timed(fn, setup=None):
        for _ in range(args.warmup):
            if setup is not None:
                setup()
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.calls):
            if setup is not None:
                setup()
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()          # compress returns with its last stage still running: count it
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms)

    def proxy_of(model):
        g = copy.deepcopy(model).half().cuda()
        g.proxy = None
        return g._ensure_proxy()

    rows = []

    def report(kind, qp, t_compress, t_probe, est, stream):
        y_units, z_units, symbols = est
        predicted = rc.predicted_stream_bytes(y_units, z_units, rc.ec_parallel_for(symbols))
        rows.append({"model": kind, "height": h, "width": w, "qp": qp, "compress_ms": t_compress, "estimate_bits_ms": t_probe,
                     "probe_over_compress": t_probe / t_compress, "symbols": symbols, "predicted_bytes": predicted,
                     "stream_bytes": int(len(stream)), "ideal_bits": (y_units + z_units) / rc.CODE_LENGTH_UNIT})
        print("%-4s %dx%d q %2d: compress %7.3f ms, estimate_bits %7.3f ms (%.2f of compress); %d symbols, predicted %d bytes, "
              "stream %d bytes" % (kind, w, h, qp, t_compress, t_probe, t_probe / t_compress, symbols, predicted, len(stream)),
              flush=True)

    for kind in [k for k in args.models.split(",") if k]:
        p = proxy_of(dmc_ld_model(skip_thres=0.15) if kind == "ld" else dmc_ht_model(kind, skip_thres=0.15))
        ref = to_device_input(np.pad(picture(h, w, index=0), ((0, pb), (0, pr), (0, 0)), mode="edge"))
        step = 1 if kind == "ld" else 8
        x0, x = (to_device_input(picture(h, w, index=i) if kind == "ld" else chunk(h, w, i)) for i in (1, 1 + step))
        p.add_ref_feature_from_frame(ref, True)
        p.compress(x0, 30, False, pb, pr)
        state = p.export_state()
        rewind = lambda: p.import_state(state, h, w)                  # noqa: E731
        for qp in qps:
            t_compress = timed(lambda: p.compress(x, qp, False, pb, pr), rewind)
            rewind()
            t_probe = timed(lambda: p.estimate_bits(x, qp, pb, pr))
            est = p.estimate_bits(x, qp, pb, pr)
            report(kind, qp, t_compress, t_probe, est, p.compress(x, qp, False, pb, pr)[0])
        del p
    if args.intra:
        p = proxy_of(dmci_model(skip_thres=0.15))
        x = to_device_input(picture(h, w, index=1))
        for qp in qps:
            t_compress = timed(lambda: p.compress(x, qp, pb, pr))
            t_probe = timed(lambda: p.estimate_bits(x, qp, pb, pr))
            est = p.estimate_bits(x, qp, pb, pr)
            report("dmci", qp, t_compress, t_probe, est, p.compress(x, qp, pb, pr)[0])
    for kind in sorted({r["model"] for r in rows}):
        ratios = [r["probe_over_compress"] for r in rows if r["model"] == kind]
        print("%-4s estimate_bits / compress: median %.2f over %d q_indexes" % (kind, statistics.median(ratios), len(ratios)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"calls": args.calls, "warmup": args.warmup, "points": rows}, f, indent=1)


if __name__ == "__main__":
    main()
