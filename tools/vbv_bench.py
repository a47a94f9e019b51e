"""What the decoder-buffer cap costs dcvc encode: pictures/s of the tool - its own figure, the host clock from the
first read to the last write - on one MI355X for a 1080p synthetic yuv420 clip, LD with seeded synthetic weights at a constant
q_index, in three variants that take turns:

    a  without the flags
    b  --vbv-maxrate / --vbv-bufsize with a bucket that never binds (ten times a's mean P-unit bits per period, 100 periods):
       one state export per P unit, no probe, a's stream byte for byte
    c  a bucket that binds: maxrate = 0.98 of a's mean P-unit bits per picture and pixel, 1 period. The clip's P units are of one
       size, so this lowers every one of them (32 of 32 measured, by one q_index each: the slack a lowered unit leaves is
       smaller than the 2 % it would take to let the next one through); a clip of which half the units are lowered pays about
       half of c's distance from a

Every variant runs once to warm up, then --repeats rounds of a, b, c in turn; the table holds each variant's runs, median,
minimum and maximum, and c's counts of lowered units, probes and recodes from its --vbv-log. Nothing here is a target.

    python tools/vbv_bench.py [--pictures 33] [--repeats 3] [--out profiles/vbv_bench.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W = 1080, 1920


def _run(args):
    r = subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=900)
    return float(re.search(r"([0-9.]+) pictures/s", r.stdout).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=33)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dcvc_amd import arch, export_weights, models, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("vbv_bench needs the GPU: a time from anywhere else says nothing")
    res = {"what": "dcvc encode pictures/s (the tool's own figure, file I/O included), %dx%d yuv420 8-bit synthetic clip, LD, synthetic "
                   "weights, qp 40; variants a no cap, b a bucket that never binds, c a bucket of one period at 0.98 of the mean P unit; one warm-up each, "
                   "then rounds of a, b, c in turn" % (W, H),
           "device": torch.cuda.get_device_name(0), "pictures": a.pictures, "repeats": a.repeats}
    with tempfile.TemporaryDirectory() as d:
        j = lambda *p: os.path.join(d, *p)      # noqa: E731
        with open(j("in.yuv"), "wb") as f:
            for i in range(a.pictures):
                y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=3)
                f.write(y.tobytes() + uv.tobytes())
        for name, cls, spec in (("i", models.DMCI, arch.dmci_spec()), ("ld", models.DMC, arch.dmc_ld_spec())):
            m = cls()
            m.load_state_dict(synthetic.synthetic_state_dict(spec, 0))
            m.update(0.15)
            export_weights.write_dcvw(j(name + ".dcvw"), "dmci" if name == "i" else "ld", m, 0.15)
        base = ["encode", "--intra", j("i.dcvw"), "--inter", j("ld.dcvw"), "-i", j("in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "40"]
        # the bucket comes from the plain run's units
        _run(base + ["-o", j("a.bin"), "--latency-log", j("lat.json")])
        units = json.load(open(j("lat.json")))["units"]
        p_bits = [8 * u["bytes"] / u["pictures"] for u in units if u["type"] == "P"]
        loose = ["--vbv-maxrate", repr(10 * float(np.mean(p_bits)) / (H * W)), "--vbv-bufsize", "100"]
        tight = ["--vbv-maxrate", repr(0.98 * float(np.mean(p_bits)) / (H * W)), "--vbv-bufsize", "1"]
        variants = {"a": lambda: _run(base + ["-o", j("a.bin")]),
                    "b": lambda: _run(base + loose + ["-o", j("b.bin"), "--vbv-log", j("b.json")]),
                    "c": lambda: _run(base + tight + ["-o", j("c.bin"), "--vbv-log", j("c.json")])}
        runs = {v: [] for v in variants}
        for v, run in variants.items():        # warm-up; makes the streams
            run()
        for _ in range(a.repeats):             # alternating
            for v, run in variants.items():
                runs[v].append(run())
        assert open(j("b.bin"), "rb").read() == open(j("a.bin"), "rb").read(), "the bucket that never binds changed the stream"
        for v in variants:
            res[v] = {"pictures_per_s": runs[v], "median": float(np.median(runs[v])), "min": min(runs[v]), "max": max(runs[v])}
            print("%s  median %7.2f  min %7.2f  max %7.2f pictures/s" % (v, res[v]["median"], res[v]["min"], res[v]["max"]), flush=True)
        for v in ("b", "c"):
            log = json.load(open(j(v + ".json")))
            res[v].update(units=len(log["units"]), lowered=log["lowered"], recodes=log["recodes"], violations=log["violations"],
                          probes=sum(u["probes"] for u in log["units"]))
        res["b_vs_a"] = res["b"]["median"] / res["a"]["median"]
        res["c_vs_a"] = res["c"]["median"] / res["a"]["median"]
        res["a_spread"] = (res["a"]["max"] - res["a"]["min"]) / res["a"]["median"]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
