"""What resampling a picture costs: microseconds per picture - one dcvc_resample_planes call for Y plus one
for U and V, four launches - timed with HIP events around a run of pictures on one stream, for 3840x2160 -> 1920x1080 and
1920x1080 -> 3840x2160, u8 and 10-bit u16 samples, and the rate that implies over the bytes a picture moves: the source
planes read, the intermediate planes written and read, the output planes written.

The operands are the same every call, as in the tool, where the upload has just written the planes: a picture and its
intermediate plane stay in the 256 MiB last-level cache, so the rate is not an HBM rate.

    python tools/resample_bench.py [--cases 2160x3840:1080x1920,1080x1920:2160x3840] [--calls 200] [--warmup 20] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2160x3840:1080x1920,1080x1920:2160x3840")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from dcvc_amd import _lib, resample
    from dcvc_amd.yuv16 import DCVC_SAMPLE_U8, DCVC_SAMPLE_U16
    assert torch.cuda.is_available(), "resample_bench needs the GPU: a time from anywhere else says nothing"
    vp = ctypes.c_void_p
    fn = resample._fn("dcvc_resample_planes")
    stream = torch.cuda.Stream()
    rows = []
    for case in args.cases.split(","):
        (H, W), (h, w) = (tuple(map(int, s.split("x"))) for s in case.split(":"))
        plan_y, plan_c = resample.Plan(H, W, h, w), resample.Plan(H // 2, W // 2, h // 2, w // 2)
        for name, dtype, code, max_val, es in (("u8", torch.uint8, DCVC_SAMPLE_U8, 255, 1), ("u16", torch.int16, DCVC_SAMPLE_U16, 1023, 2)):
            src = torch.randint(0, max_val + 1, (H * W * 3 // 2,), device="cuda").to(dtype)
            dst = torch.empty(h * w * 3 // 2, dtype=dtype, device="cuda")
            ws = torch.empty(max(plan_y.workspace_bytes(1), plan_c.workspace_bytes(2)), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def run(calls):
                for _ in range(calls):
                    _lib.check(fn(plan_y._p, vp(src.data_ptr()), code, W, H * W, vp(dst.data_ptr()), code, w, h * w, 1, max_val,
                                  vp(ws.data_ptr()), ws.numel(), vp(stream.cuda_stream)))
                    _lib.check(fn(plan_c._p, vp(src.data_ptr() + H * W * es), code, W // 2, H * W // 4, vp(dst.data_ptr() + h * w * es),
                                  code, w // 2, h * w // 4, 2, max_val, vp(ws.data_ptr()), ws.numel(), vp(stream.cuda_stream)))

            run(args.warmup)
            stream.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            run(args.calls)
            t1.record(stream)
            stream.synchronize()
            us = 1e3 * t0.elapsed_time(t1) / args.calls
            # source read + intermediate [H][w] written and read + output written, Y and the two chroma planes (3/2 of Y)
            nbytes = (H * W + 2 * H * w + h * w) * 3 // 2 * es
            rows.append({"from": [H, W], "to": [h, w], "samples": name, "calls": args.calls, "us_per_picture": us, "launches": 4,
                         "bytes": nbytes, "gb_per_s": nbytes / us / 1e3})
            print("%dx%d -> %dx%d %-3s: %8.2f us per picture (Y + U,V: 4 launches), %7.1f GB/s over %d bytes (%d pictures)"
                  % (W, H, w, h, name, us, nbytes / us / 1e3, nbytes, args.calls), flush=True)
            del src, dst, ws
        plan_y.close()
        plan_c.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"warmup": args.warmup, "points": rows}, f, indent=1)


if __name__ == "__main__":
    main()
