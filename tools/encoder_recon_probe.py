"""What a trial coding of dcvc encode --target-psnr costs: milliseconds per call of compress, of reconstruct
and of export_state + import_state on the same unit for LD, HT-S and HT-L, medians after warm-up, each timed to the end of
the device's work, on the seeded synthetic models with skip_thres 0.15.

A trial of a P unit is import_state (not before the first), compress, reconstruct and the measurement; export_state runs once
per unit. The state everything is timed against is that of a running GOP - add_ref and one P unit - exported once and
imported again, outside the timed span, before every compress (tools/inter_rate_probe.py has the reason).

    python tools/encoder_recon_probe.py [--size 1080x1920] [--models ld,hts,htl] [--qp 32] [--calls 16] [--warmup 4]
                                        [--out profiles/encoder_recon_probe.json]
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
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_recon_probe.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from codec_util import chunk, dmc_ht_model, dmc_ld_model, picture, to_device_input
    h, w = map(int, args.size.split("x"))
    pb, pr = -h % 16, -w % 16

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
            torch.cuda.synchronize()          # the calls return with device work still running: count it
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms)

    rows = []
    for kind in [k for k in args.models.split(",") if k]:
        g = copy.deepcopy(dmc_ld_model(skip_thres=0.15) if kind == "ld" else dmc_ht_model(kind, skip_thres=0.15)).half().cuda()
        g.proxy = None
        p = g._ensure_proxy()
        ref = to_device_input(np.pad(picture(h, w, index=0), ((0, pb), (0, pr), (0, 0)), mode="edge"))
        step = 1 if kind == "ld" else 8
        x0, x = (to_device_input(picture(h, w, index=i) if kind == "ld" else chunk(h, w, i)) for i in (1, 1 + step))
        p.add_ref_feature_from_frame(ref, True)
        p.compress(x0, 30, False, pb, pr)
        state = p.export_state()
        rewind = lambda: p.import_state(state, h, w)                  # noqa: E731
        t_compress = timed(lambda: p.compress(x, args.qp, False, pb, pr), rewind)
        t_recon = timed(lambda: p.reconstruct(h, w))
        t_export = timed(p.export_state)
        t_import = timed(rewind)
        row = {"model": kind, "height": h, "width": w, "qp": args.qp, "compress_ms": t_compress, "reconstruct_ms": t_recon,
               "export_state_ms": t_export, "import_state_ms": t_import, "state_bytes": int(state.numel()),
               "reconstruct_over_compress": t_recon / t_compress,
               "export_import_over_compress": (t_export + t_import) / t_compress}
        # in compress calls: a unit of k trials = one export, k compress + reconstruct, k - 1 imports (the measurement aside)
        for k in (2, 12):
            row["unit_of_%d_trials_in_compress_calls" % k] = (t_export + k * (t_compress + t_recon) + (k - 1) * t_import) / t_compress
        rows.append(row)
        print("%-4s %dx%d q %2d: compress %7.3f ms, reconstruct %7.3f ms (%.2f of compress), export_state %6.3f ms + import_state "
              "%6.3f ms (%.2f of compress); a unit of 2 trials %.2f, of 12 trials %.2f compress calls"
              % (kind, w, h, args.qp, t_compress, t_recon, row["reconstruct_over_compress"], t_export, t_import,
                 row["export_import_over_compress"], row["unit_of_2_trials_in_compress_calls"], row["unit_of_12_trials_in_compress_calls"]),
              flush=True)
        del p, g
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"calls": args.calls, "warmup": args.warmup, "points": rows}, f, indent=1)


if __name__ == "__main__":
    main()
