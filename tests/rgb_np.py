"""numpy restatement of the reference's RGB picture path (BT.709, src/utils/transforms.py:17-27 rgb2ycbcr and :53-66
ycbcr2rgb, with the tensor op chains of test_video.py:87-122 get_src_frame, :55-64 get_distortion and :366-370 the writer).

Written from the formulas: every torch op rounds on its own, so every step here is one fp32 (or fp16) numpy op on arrays, and
each Python-double constant (or constant expression such as 1 - Kb) becomes fp32 when it meets the array.

div selects how a tensor divided by a scalar is evaluated:
  "true"  - a / b, as CPU torch computes it;
  "recip" - a * (1 / b) with the reciprocal taken in fp32, as torch's GPU true-division kernel computes it when the divisor
            is a CPU scalar.
"""
import numpy as np

KR, KG, KB = 0.2126, 0.7152, 0.0722
f32, f16 = np.float32, np.float16


def _div(a, b, div):
    if div == "true":
        return a / f32(b)
    if div == "recip":
        return a * (f32(1.0) / f32(b))
    raise ValueError(div)


def _clamp(a, lo, hi):
    # torch.clamp: NaN passes through
    return np.where(np.isnan(a), a, np.minimum(np.maximum(a, a.dtype.type(lo)), a.dtype.type(hi)))


def rgb2ycbcr(r, g, b, div):
    """fp32 planes in 0..1 -> clamped fp32 (y, cb, cr)"""
    y = (f32(KR) * r + f32(KG) * g) + f32(KB) * b
    cb = _div(f32(0.5) * (b - y), 1 - KB, div) + f32(0.5)
    cr = _div(f32(0.5) * (r - y), 1 - KR, div) + f32(0.5)
    return tuple(_clamp(c, 0.0, 1.0) for c in (y, cb, cr))


def rgb_to_x(rgb, div):
    """[3, H, W] u8 -> [H, W, 3] fp16 model input (x.float() / 255, rgb2ycbcr, .half(), - 0.5)"""
    f = _div(rgb.astype(f32), 255.0, div)
    ycc = rgb2ycbcr(f[0], f[1], f[2], div)
    return np.stack([(c.astype(f16).astype(f32) - f32(0.5)).astype(f16) for c in ycc], axis=-1)


def ycbcr2rgb(y, cb, cr, div):
    """fp32 (y, cb, cr) -> clamped fp32 (r, g, b)"""
    r = y + f32(2 - 2 * KR) * (cr - f32(0.5))
    b = y + f32(2 - 2 * KB) * (cb - f32(0.5))
    g = _div((y - f32(KR) * r) - f32(KB) * b, KG, div)
    return tuple(_clamp(c, 0.0, 1.0) for c in (r, g, b))


def x_to_rgb(x_hat, H, W, div):
    """[Hp, Wp, 3] fp16 x_hat -> ([3, H, W] fp16 distortion planes, [H, W, 3] u8 writer pixels)"""
    xh = (x_hat[:H, :W].astype(f32) + f32(0.5)).astype(f16).astype(f32)
    rgb = ycbcr2rgb(xh[..., 0], xh[..., 1], xh[..., 2], div)
    rgb16 = np.stack([_clamp((c.astype(f16).astype(f32) * f32(255.0)).astype(f16), 0.0, 255.0) for c in rgb])
    rgb8 = np.rint(rgb16.astype(f32)).astype(np.uint8).transpose(1, 2, 0)
    return rgb16, np.ascontiguousarray(rgb8)


def all_colours():
    """[3, 4096, 4096] u8 holding each of the 2^24 colours once (r = i >> 16, g = (i >> 8) & 255, b = i & 255)"""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255]).astype(np.uint8).reshape(3, 4096, 4096)


def psnr(sse, n):
    """metrics.py:10-24 calc_psnr from the fp64 sum of squared differences over n samples"""
    mse = sse / n
    if np.isnan(mse) or np.isinf(mse):
        return -999.9
    p = 10 * np.log10(255.0 * 255.0 / mse) if mse > 1e-10 else 999.9
    return min(p, 99.9)
