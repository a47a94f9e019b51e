"""What converting a wire picture costs: microseconds per dcvc_wire_unpack / dcvc_wire_pack call and the rate
over the bytes read + written, for every wire format at 1920x1080 and 3840x2160, timed with HIP events on one stream.

The yardstick is a device-to-device copy (hipMemcpyAsync, issued through torch's copy_ of one contiguous uint8 tensor to
another) of (bytes read + bytes written) / 2 bytes - a copy reads and writes every byte, so it moves the same total - timed in
the same loop: the timed calls run in rounds of --round calls of the kernel, then as many copies, each run of calls between two
events, so that whatever else the machine does falls on both. The operands are the same every call, as in the tool, where the
upload has just written the picture: they sit in the 256 MiB last-level cache, so the rates are not HBM rates.

    python tools/wire_bench.py [--sizes 1080x1920,2160x3840] [--calls 200] [--warmup 20] [--round 20] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [("nv21", 8), ("nv16", 8), ("nv16", 10), ("uyvy", 8), ("yuy2", 8), ("yuy2", 10), ("v210", 10)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--round", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from dcvc_amd import _lib, pixfmt, wirefmt
    assert torch.cuda.is_available(), "wire_bench needs the GPU: a time from anywhere else says nothing"
    assert args.calls % args.round == 0, "--calls must be a multiple of --round"
    vp = ctypes.c_void_p
    stream = torch.cuda.Stream()
    rows = []
    for size in args.sizes.split(","):
        H, W = map(int, size.split("x"))
        for name, bits in CASES:
            wire = wirefmt.WIRE[name]
            wbytes = wirefmt.picture_bytes(wire, bits, H, W)
            cbytes = pixfmt.picture_samples(wirefmt.carrier(wire), H, W) * (1 if bits == 8 else 2)
            moved = wbytes + cbytes                                      # either direction reads one picture and writes the other
            wire_t = torch.randint(0, 256, (wbytes,), device="cuda").to(torch.uint8)
            carrier_t = torch.zeros(cbytes, dtype=torch.uint8, device="cuda")
            a, b = (torch.zeros(moved // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
            for op in ("unpack", "pack"):
                fn = wirefmt._fn("dcvc_wire_" + op)
                src, dst = (wire_t, carrier_t) if op == "unpack" else (carrier_t, wire_t)

                def kernel(calls):
                    for _ in range(calls):
                        _lib.check(fn(vp(src.data_ptr()), wire, bits, H, W, vp(dst.data_ptr()), vp(stream.cuda_stream)))

                def copy(calls):
                    with torch.cuda.stream(stream):
                        for _ in range(calls):
                            b.copy_(a, non_blocking=True)

                kernel(args.warmup)
                copy(args.warmup)
                stream.synchronize()
                ms = {"kernel": 0.0, "copy": 0.0}
                for _ in range(args.calls // args.round):
                    for what, run in (("kernel", kernel), ("copy", copy)):
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record(stream)
                        run(args.round)
                        t1.record(stream)
                        stream.synchronize()
                        ms[what] += t0.elapsed_time(t1)
                us, copy_us = (1e3 * ms[k] / args.calls for k in ("kernel", "copy"))
                rows.append({"size": [H, W], "format": name, "bit_depth": bits, "op": op, "calls": args.calls, "us_per_call": us,
                             "bytes": moved, "gb_per_s": moved / us / 1e3, "copy_bytes": moved // 2, "copy_us": copy_us,
                             "ratio_to_copy": us / copy_us})
                print("| %dx%d | %s %d | %s | %.2f | %.0f | %.2f | %.2f |" % (W, H, name, bits, op, us, moved / us / 1e3, copy_us, us / copy_us),
                      flush=True)
            del wire_t, carrier_t, a, b
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"warmup": args.warmup, "round": args.round, "points": rows}, f, indent=1)


if __name__ == "__main__":
    main()
