"""Generates tests/golden/yuv16_golden.npz: the high-bit-depth YUV420 reader and writer evaluated as torch ops on the CPU, an
implementation independent of the numpy restatement (tests/yuv16_np.py) that the fixture pins.

  * reader (DCVC-FM video_reader.py:130-183 YUVReader on DCVC-UF's get_src_frame, test_video.py:69-123): 10-bit samples
    (every code in Y, random U / V) -> torch.from_numpy(v.astype(float32) / max_val), .half() - 0.5, nearest chroma ->
    x [H, W, 3] fp16;
  * writer (test_video.py:32-45 before its * 255, then video_writer.py:86-130 YUVWriter at 10 and 16 bits): random fp16 x_hat
    [Hp, Wp, 3] with values past both clamps, cropped to H x W -> fp32 distortion planes clamp(t * max_val, 0, max_val) and
    their torch.round (half to even) as uint16.

Usage: python tests/golden/make_yuv16_golden.py
"""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def reader(y, uv, bit_depth):
    m = (1 << bit_depth) - 1
    yf = torch.from_numpy(y.astype(np.float32) / np.float32(m))
    uvf = torch.from_numpy(uv.astype(np.float32) / np.float32(m))
    up = uvf.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    x = torch.cat((yf[None], up), dim=0).half() - 0.5
    return x.permute(1, 2, 0).numpy()


def writer(x_hat, H, W, bit_depth):
    m = float((1 << bit_depth) - 1)
    t = torch.from_numpy(x_hat).permute(2, 0, 1)[:, :H, :W] + 0.5                       # fp16
    c = t[1:].float()
    s = ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + c[:, 1::2, 0::2]) + c[:, 1::2, 1::2]
    tuv = (s * 0.25).half()
    dist_y = torch.clamp(t[0].float() * m, 0, m)
    dist_uv = torch.clamp(tuv.float() * m, 0, m)
    return (dist_y.numpy(), dist_uv.numpy(), torch.round(dist_y).to(torch.int32).numpy().astype(np.uint16),
            torch.round(dist_uv).to(torch.int32).numpy().astype(np.uint16))


def main():
    rng = np.random.default_rng(10)
    out = {}
    H, W = 4, 256                                                   # 1024 luma samples: every 10-bit code once
    y = np.arange(H * W, dtype=np.uint16).reshape(H, W)
    uv = rng.integers(0, 1024, (2, H // 2, W // 2), dtype=np.uint16)
    out["y10"], out["uv10"], out["x10"] = y, uv, reader(y, uv, 10)

    Hc, Wc, Hp, Wp = 30, 44, 32, 48
    x_hat = rng.uniform(-0.75, 0.75, (Hp, Wp, 3)).astype(np.float16)
    x_hat[0, :12] = np.array([-0.5, 0.5, -0.6, 0.6, -0.501, 0.499, 0.0, -0.25, 0.25, 0.75, -0.75, 0.4999], np.float16)[:, None]
    out["x_hat"] = x_hat
    out["crop"] = np.array([Hc, Wc], dtype=np.int64)
    for b in (10, 16):
        dy, duv, y16, uv16 = writer(x_hat, Hc, Wc, b)
        out["dist_y%d" % b], out["dist_uv%d" % b], out["y16_%d" % b], out["uv16_%d" % b] = dy, duv, y16, uv16
    path = os.path.join(ROOT, "tests", "golden", "yuv16_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
