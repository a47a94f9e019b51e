"""The size probe against compress: milliseconds per call of DMCIProxy.estimate_bits and of
DMCIProxy.compress on the same picture and q_index, medians after warm-up, on the seeded synthetic model with skip_thres
0.15; and the prediction next to the stream each compress wrote.

    python tools/intra_rate_probe.py [--size 1080x1920] [--qps 0,21,42,63] [--calls 24] [--warmup 4] [--out FILE.json]
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
    ap.add_argument("--qps", default="0,21,42,63")
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from codec_util import dmci_model, picture
    from dcvc_amd import rate_control as rc
    h, w = map(int, args.size.split("x"))
    g = copy.deepcopy(dmci_model(skip_thres=0.15)).half().cuda()
    g.proxy = None
    p = g._ensure_proxy()
    x = torch.from_numpy(picture(h, w, index=1)).permute(2, 0, 1)[None].cuda().contiguous(memory_format=torch.channels_last)
    pb, pr = (h + 15) // 16 * 16 - h, (w + 15) // 16 * 16 - w

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()          # compress returns with its reconstruction still running: count it
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms)

    rows = []
    for qp in [int(q) for q in args.qps.split(",")]:
        t_compress = timed(lambda: p.compress(x, qp, pb, pr))
        t_probe = timed(lambda: p.estimate_bits(x, qp, pb, pr))
        y_units, z_units, symbols = p.estimate_bits(x, qp, pb, pr)
        stream = p.compress(x, qp, pb, pr)[0]
        predicted = rc.predicted_stream_bytes(y_units, z_units, rc.ec_parallel_for(symbols))
        row = {"height": h, "width": w, "qp": qp, "compress_ms": t_compress, "estimate_bits_ms": t_probe,
               "probe_over_compress": t_probe / t_compress, "symbols": symbols, "predicted_bytes": predicted,
               "stream_bytes": int(len(stream)), "ideal_bits": (y_units + z_units) / rc.CODE_LENGTH_UNIT}
        rows.append(row)
        print("%dx%d q %2d: compress %7.3f ms, estimate_bits %7.3f ms (%.2f of compress); %d symbols, predicted %d bytes, "
              "stream %d bytes" % (w, h, qp, t_compress, t_probe, t_probe / t_compress, symbols, predicted, len(stream)), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"calls": args.calls, "warmup": args.warmup, "points": rows}, f, indent=1)


if __name__ == "__main__":
    main()
