"""What hashing a picture costs: microseconds per dcvc_crc32_segments call over the three planes of a YUV420
picture - two launches - timed with HIP events around a run of calls on one stream (tools/resample_bench.py's conventions),
at 1920x1080 and 3840x2160, 8-bit and 16-bit samples, and the GB/s that implies over the picture's bytes:

  warm   the same picture every call, as in the tool, where the conversion kernel has just written it: it stays in the
         256 MiB last-level cache, so the rate is not an HBM rate;
  cold   rotating over > 512 MB of distinct pictures, so that the bytes come from HBM; the time as a multiple of the HBM
         floor at 6.3 TB/s (the yardstick of tools/pixfmt_bench.py for the same pictures).

In the same run, what the kernel replaces: the device-to-host copy of that picture into pinned memory plus zlib.crc32 of it on
the host (a host clock around copy, synchronise and hash; the two parts are given too). Every CRC is checked against zlib's.

    python tools/crc_bench.py [--sizes 1080x1920,2160x3840] [--calls 200] [--warmup 20] [--host-reps 10] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from dcvc_amd import _lib, picture_hash
    assert torch.cuda.is_available(), "crc_bench needs the GPU: a time from anywhere else says nothing"
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    fn = picture_hash._fn("dcvc_crc32_segments")
    stream = torch.cuda.Stream()
    rows = []
    for size in args.sizes.split(","):
        H, W = map(int, size.split("x"))
        for name, es in (("u8", 1), ("u16", 2)):
            hw = H * W
            nbytes = hw * 3 // 2 * es
            offsets = (ll * 3)(0, hw * es, (hw + hw // 4) * es)
            lengths = (ll * 3)(hw * es, hw // 4 * es, hw // 4 * es)
            n_pics = max(2, -(-(512 << 20) // nbytes))
            pics = torch.randint(0, 256, (n_pics, nbytes), dtype=torch.uint8, device="cuda")
            out = torch.empty(3, dtype=torch.int32, device="cuda")
            pinned = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            torch.cuda.synchronize()

            def run(calls, rotate):
                for k in range(calls):
                    at = pics.data_ptr() + (k % n_pics if rotate else 0) * nbytes
                    _lib.check(fn(vp(at), offsets, lengths, 3, vp(out.data_ptr()), vp(stream.cuda_stream)))

            row = {"size": [H, W], "samples": name, "bytes": nbytes, "calls": args.calls, "launches": 2,
                   "hbm_floor_us": nbytes / HBM_BYTES_PER_S * 1e6}
            for label, rotate in (("warm", False), ("cold", True)):
                run(args.warmup, rotate)
                stream.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                run(args.calls, rotate)
                t1.record(stream)
                stream.synchronize()
                us = 1e3 * t0.elapsed_time(t1) / args.calls
                row[label + "_us"] = us
                row[label + "_gb_per_s"] = nbytes / us / 1e3
            row["cold_times_hbm_floor"] = row["cold_us"] / row["hbm_floor_us"]
            # the result is zlib's (the last cold call hashed picture (calls - 1) % n_pics)
            last = (args.calls - 1) % n_pics
            host = pics[last].cpu().numpy().tobytes()
            got = [int(v) & 0xFFFFFFFF for v in out.tolist()]
            want = [zlib.crc32(host[offsets[k]:offsets[k] + lengths[k]]) for k in range(3)]
            assert got == want, (got, want)
            # what it replaces: the picture to pinned host memory, then zlib.crc32 there
            copy_s, hash_s, both_s = [], [], []
            with torch.cuda.stream(stream):
                for k in range(args.host_reps + 2):
                    t_a = time.perf_counter()
                    pinned.copy_(pics[k % n_pics], non_blocking=True)
                    stream.synchronize()
                    t_b = time.perf_counter()
                    zlib.crc32(memoryview(pinned.numpy()))
                    t_c = time.perf_counter()
                    if k >= 2:
                        copy_s.append(t_b - t_a); hash_s.append(t_c - t_b); both_s.append(t_c - t_a)
            med = lambda v: sorted(v)[len(v) // 2] * 1e6
            row.update({"copy_to_host_us": med(copy_s), "host_zlib_us": med(hash_s), "copy_plus_host_crc_us": med(both_s)})
            row["host_path_over_kernel_warm"] = row["copy_plus_host_crc_us"] / row["warm_us"]
            rows.append(row)
            print("%dx%d %-3s: warm %8.2f us (%7.1f GB/s), cold %8.2f us (%7.1f GB/s, %.2f x the HBM floor of %.2f us); "
                  "copy to host + zlib.crc32 %9.1f us (copy %.1f, zlib %.1f): %.0f x the warm call"
                  % (W, H, name, row["warm_us"], row["warm_gb_per_s"], row["cold_us"], row["cold_gb_per_s"], row["cold_times_hbm_floor"],
                     row["hbm_floor_us"], row["copy_plus_host_crc_us"], row["copy_to_host_us"], row["host_zlib_us"],
                     row["host_path_over_kernel_warm"]), flush=True)
            del pics, out, pinned
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S, "points": rows},
                      f, indent=1)


if __name__ == "__main__":
    main()
