"""Generates tests/golden/msssim_golden.npz from the REFERENCE's metric (run in the build container, where /root/reference
exists): src/utils/metrics.py calc_msssim / calc_msssim_rgb on smooth synthetic planes.

Each case stores <name>_src (u8), <name>_rec (fp16 holding 0..255, or u8) and <name>_value (the reference's result):
  l5_240x416   5 levels                     l4_120x208   4 levels
  min_88x88    the smallest accepted size   odd_175x301  odd sides, 4 levels
  odd_176x177  5 levels, odd width          same_120x128 rec == src: exactly 1.0
  inv_120x128  rec = 255 - src: NaN         u8_144x200   rec as u8
  rgb_96x128   3 x 96 x 128 through calc_msssim_rgb

Usage: python tests/golden/make_msssim_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, "/root/reference")
from src.utils.metrics import calc_msssim, calc_msssim_rgb  # noqa: E402


def smooth(rng, h, w, amp):
    """a few random sinusoids plus a little pixel noise: compresses well, and has structure on every pyramid level"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = np.zeros((h, w))
    for _ in range(6):
        fy, fx = rng.uniform(0.005, 0.12, 2)
        v += rng.uniform(0.3, 1.0) * np.sin(fy * yy + fx * xx + rng.uniform(0, 2 * np.pi))
    return amp * v / 6 + rng.normal(0, 1.5, (h, w))


def pair(rng, h, w, rec_u8=False):
    src = np.clip(np.round(128 + smooth(rng, h, w, 200)), 0, 255).astype(np.uint8)
    rec = np.clip(src + smooth(rng, h, w, 12), 0, 255)
    return src, (np.round(rec).astype(np.uint8) if rec_u8 else rec.astype(np.float16))


def main():
    rng = np.random.default_rng(2024)
    out = {}

    def add(name, src, rec, value):
        out[name + "_src"], out[name + "_rec"], out[name + "_value"] = src, rec, np.float64(value)
        print("%-14s %-10s %-8s %.17g" % (name, "x".join(map(str, src.shape)), rec.dtype, value))

    for name, h, w in [("l5_240x416", 240, 416), ("l4_120x208", 120, 208), ("min_88x88", 88, 88),
                       ("odd_175x301", 175, 301), ("odd_176x177", 176, 177)]:
        s, r = pair(rng, h, w)
        add(name, s, r, calc_msssim(s, r.astype(np.float64)))
    s, _ = pair(rng, 120, 128)
    add("same_120x128", s, s.astype(np.float16), calc_msssim(s, s))
    with np.errstate(invalid="ignore"):
        add("inv_120x128", s, (255 - s).astype(np.uint8), calc_msssim(s, 255 - s))
    s, r = pair(rng, 144, 200, rec_u8=True)
    add("u8_144x200", s, r, calc_msssim(s, r))
    planes = [pair(rng, 96, 128) for _ in range(3)]
    s = np.stack([p[0] for p in planes])
    r = np.stack([p[1] for p in planes])
    add("rgb_96x128", s, r, calc_msssim_rgb(s, r.astype(np.float64)))
    path = os.path.join(ROOT, "tests", "golden", "msssim_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
