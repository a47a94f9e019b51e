"""What reading from a pipe costs dcvc encode, and what --read-ahead gives back: pictures/s of the tool - its own
figure, the host clock from the first read to the last write, behind a device synchronise - on one MI355X for a 1080p synthetic
yuv420 clip, all-intra and LD, in four variants that take turns:

    a  this build, -i a regular file                     c  this build, -i - (stdin), --read-ahead 0
    b  another build of the tool (--parent-tool: the     d  this build, -i - (stdin), --read-ahead 2
       parent commit's), the same file

Every variant runs once to warm up (code objects, the file cache), then --repeats rounds of a, b, c, d in turn; the table holds
each variant's runs, median, minimum and maximum. stdin is a pipe fed by this process from memory in 1 MiB writes; -o is a
regular file in every variant, and every variant's stream is compared with a's. Nothing here is a target.

    python tools/pipe_bench.py [--pictures 60] [--repeats 3] [--parent-tool PATH] [--out profiles/pipe_bench.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W = 1080, 1920


def _rate(text):
    return float(re.search(r"([0-9.]+) pictures/s", text).group(1))


def _run_file(tool, args):
    r = subprocess.run([tool] + args, check=True, capture_output=True, text=True, timeout=900)
    return _rate(r.stdout)


def _run_stdin(tool, args, data):
    proc = subprocess.Popen([tool] + args, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, bufsize=0)
    stdin, proc.stdin = proc.stdin, None

    def feed():
        try:
            mv = memoryview(data)
            for at in range(0, len(mv), 1 << 20):
                piece = mv[at:at + (1 << 20)]
                while len(piece):
                    piece = piece[stdin.write(piece):]
        except OSError:
            pass
        finally:
            stdin.close()

    t = threading.Thread(target=feed, daemon=True)
    t.start()
    try:
        out, err = proc.communicate(timeout=900)
    finally:
        proc.kill()
        proc.wait()
        t.join(10)
    if proc.returncode != 0:
        raise SystemExit("dcvc failed: " + err.decode("utf-8", "replace"))
    return _rate(out.decode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pictures", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-tool", default="", help="the dcvc binary of another build, next to its own libdcvc_amd.so (variant b)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dcvc_amd import arch, export_weights, models, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("pipe_bench needs the GPU: a time from anywhere else says nothing")
    res = {"what": "dcvc encode pictures/s (the tool's own figure, file I/O included), %dx%d yuv420 8-bit synthetic clip, synthetic weights, "
                   "qp 32; variants a file, b another build's tool on the same file, c stdin --read-ahead 0, d stdin --read-ahead 2; "
                   "one warm-up each, then rounds of a, b, c, d in turn" % (W, H),
           "device": torch.cuda.get_device_name(0), "pictures": a.pictures, "repeats": a.repeats, "parent_tool": bool(a.parent_tool)}
    with tempfile.TemporaryDirectory() as d:
        j = lambda *p: os.path.join(d, *p)
        clip = bytearray()
        for i in range(a.pictures):
            y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=3)
            clip += y.tobytes() + uv.tobytes()
        clip = bytes(clip)
        with open(j("in.yuv"), "wb") as f:
            f.write(clip)
        for name, cls, spec in (("i", models.DMCI, arch.dmci_spec()), ("ld", models.DMC, arch.dmc_ld_spec())):
            m = cls()
            m.load_state_dict(synthetic.synthetic_state_dict(spec, 0))
            m.update(0.15)
            export_weights.write_dcvw(j(name + ".dcvw"), "dmci" if name == "i" else "ld", m, 0.15)
        for mode in ("intra", "ld"):
            base = ["encode", "--intra", j("i.dcvw")] + (["--inter", j("ld.dcvw")] if mode == "ld" else []) + \
                   ["-W", str(W), "-H", str(H), "--qp-i", "32"]
            out = lambda v: j("%s_%s.bin" % (mode, v))
            variants = {"a": lambda: _run_file(TOOL, base + ["-i", j("in.yuv"), "-o", out("a")])}
            if a.parent_tool:
                variants["b"] = lambda: _run_file(a.parent_tool, base + ["-i", j("in.yuv"), "-o", out("b")])
            variants["c"] = lambda: _run_stdin(TOOL, base + ["-i", "-", "--read-ahead", "0", "-o", out("c")], clip)
            variants["d"] = lambda: _run_stdin(TOOL, base + ["-i", "-", "--read-ahead", "2", "-o", out("d")], clip)
            runs = {v: [] for v in variants}
            for v, run in variants.items():        # warm-up; makes the streams
                run()
            for _ in range(a.repeats):             # alternating
                for v, run in variants.items():
                    runs[v].append(run())
            ref = open(out("a"), "rb").read()
            table = {"stream_bytes": len(ref)}
            for v in variants:
                assert open(out(v), "rb").read() == ref, "variant %s wrote another stream" % v
                table[v] = {"pictures_per_s": runs[v], "median": float(np.median(runs[v])), "min": min(runs[v]), "max": max(runs[v])}
                print("%-5s %s  median %7.2f  min %7.2f  max %7.2f pictures/s" % (mode, v, table[v]["median"], table[v]["min"], table[v]["max"]),
                      flush=True)
            if "b" in table:
                table["a_vs_b"] = table["a"]["median"] / table["b"]["median"]
                table["a_median_below_b_min"] = table["a"]["median"] < table["b"]["min"]
            table["d_vs_c"] = table["d"]["median"] / table["c"]["median"]
            res[mode] = table
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
