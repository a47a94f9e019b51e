"""What the scene-cut measurement costs: microseconds per dcvc_luma_sad call, timed with HIP events around
a run of calls on one stream, at 1920x1080 and 3840x2160, for ldx 3 (one picture, 16-byte loads) and ldx 24 (a slot of an
8-picture chunk, the strided path), and the rate that implies over the H W (2 ldx + 2) bytes of the pixels' extent and
the two luma planes.

Two figures per shape: "warm" - the same x and planes every call, which is what the tool sees (convert has just written x,
and a 1080p picture stays in the 256 MiB last-level cache) - and "cold" - the calls walk over enough copies of x and
of the planes that every call's operands have left that cache, which is the HBM rate.

    python tools/scene_cut_probe.py [--sizes 1080x1920,2160x3840] [--ldx 3,24] [--calls 200] [--warmup 20] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLD_FOOTPRINT = 1 << 30      # bytes the cold walk covers: four times the last-level cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--ldx", default="3,24")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from dcvc_amd import _lib
    assert torch.cuda.is_available(), "scene_cut_probe needs the GPU: a time from anywhere else says nothing"
    vp, ci = ctypes.c_void_p, ctypes.c_int
    fn = _lib.fn("dcvc_luma_sad", ci, [vp, ci, ci, ci, vp, vp, vp, vp])
    stream = torch.cuda.Stream()
    rows = []
    for size in args.sizes.split(","):
        h, w = map(int, size.split("x"))
        for ldx in (int(v) for v in args.ldx.split(",")):
            nbytes = h * w * (2 * ldx + 2)
            for mode in ("warm", "cold"):
                copies = 1 if mode == "warm" else max(2, -(-COLD_FOOTPRINT // nbytes))
                xs = [torch.rand(h * w * ldx, device="cuda").sub_(0.5).half() for _ in range(copies)]
                planes = [torch.randint(0, 256, (h, w), dtype=torch.uint8, device="cuda") for _ in range(copies + 1)]
                sad = torch.zeros(1, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()

                def run(calls):
                    for k in range(calls):
                        # the previous call's luma is this call's prev, as in the tool
                        _lib.check(fn(vp(xs[k % copies].data_ptr()), ldx, h, w, vp(planes[k % (copies + 1)].data_ptr()),
                                      vp(planes[(k + 1) % (copies + 1)].data_ptr()), vp(sad.data_ptr()), vp(stream.cuda_stream)))

                run(args.warmup)
                stream.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                run(args.calls)
                t1.record(stream)
                stream.synchronize()
                us = 1e3 * t0.elapsed_time(t1) / args.calls
                rows.append({"height": h, "width": w, "ldx": ldx, "mode": mode, "copies": copies, "calls": args.calls,
                             "us_per_call": us, "bytes": nbytes, "gb_per_s": nbytes / us / 1e3})
                print("%dx%d ldx %2d %s: %8.2f us per call, %7.1f GB/s over %d bytes (%d calls, %d operand sets)"
                      % (w, h, ldx, mode, us, nbytes / us / 1e3, nbytes, args.calls, copies), flush=True)
                del xs, planes
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"warmup": args.warmup, "points": rows}, f, indent=1)


if __name__ == "__main__":
    main()
