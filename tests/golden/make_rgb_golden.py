"""Generates tests/golden/rgb_golden.npz from the REFERENCE's colour transforms (run in the build container, where
/root/reference exists): src/utils/transforms.py rgb2ycbcr / ycbcr2rgb with the tensor op chains of test_video.py:87-122
(get_src_frame, png branch), :55-64 (get_distortion, png branch) and :366-370 (the PNG writer), on CPU torch.

CPU torch divides a tensor by a scalar with a true division; the GPU kernels follow torch on a GPU (a * (1 / b)), so this
fixture pins the numpy restatement (tests/rgb_np.py, div="true") and the op chain, not the kernels.

  * x: every u8 value on each channel (rows 0-2), 2048 random colours (rows 3-10) -> the model input [H, W, 3] fp16;
  * x_hat: random fp16 [Hp, Wp, 3] with values past both clamps, cropped to H x W (padded rows) -> rgb16 [3, H, W] fp16
    (the distortion planes) and rgb8 [H, W, 3] u8 (the writer's pixels).

Usage: python tests/golden/make_rgb_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, "/root/reference")
from src.utils.transforms import rgb2ycbcr, ycbcr2rgb  # noqa: E402


def main():
    rng = np.random.default_rng(5)
    H, W = 11, 256
    rgb = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    for c in range(3):
        rgb[c, c] = np.arange(256, dtype=np.uint8)           # channel c sweeps 0..255, the others random
    x = torch.from_numpy(rgb).unsqueeze(0)
    x = x.float() / 255.0
    x = rgb2ycbcr(x)
    x = x.half() - 0.5
    out = {"rgb": rgb, "x": x[0].permute(1, 2, 0).numpy()}

    Hc, Wc, Hp, Wp = 30, 44, 32, 48
    x_hat = rng.uniform(-0.75, 0.75, (Hp, Wp, 3)).astype(np.float16)
    x_hat[0, :12] = np.array([-0.5, 0.5, -0.6, 0.6, -0.501, 0.499, 0.0, -0.25, 0.25, 0.75, -0.75, 0.4999], np.float16)[:, None]
    t = torch.from_numpy(x_hat).permute(2, 0, 1).unsqueeze(0)[:, :, :Hc, :Wc]
    rec = ycbcr2rgb(t + 0.5)
    rgb16 = torch.clamp(rec * 255, 0, 255)
    out["x_hat"] = x_hat
    out["crop"] = np.array([Hc, Wc], dtype=np.int64)
    out["rgb16"] = rgb16[0].numpy()
    out["rgb8"] = rgb16.round().byte()[0].permute(1, 2, 0).numpy()
    path = os.path.join(ROOT, "tests", "golden", "rgb_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
