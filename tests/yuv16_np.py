"""numpy restatement of the high-bit-depth YUV420 path (bit depth 9..16, uint16 samples): DCVC-FM's YUVReader / YUVWriter
scale (video_reader.py:130-183, video_writer.py:86-130) on DCVC-UF's picture chain (test_video.py:32-45, 69-123).

Written from the arithmetic stated in DESIGN.md ("High-bit-depth YUV420 sources"), one fp32 / fp16 numpy op per step:
  reader: d = fp16(fp32(v) / fp32(max_val)) (a true, correctly rounded division), x = fp16(fp32(d) - 0.5), chroma repeated
          over its 2 x 2 block;
  writer: t = fp16(x_hat + 0.5) (Y), fp16(fp32 sum of the 2 x 2 block of fp16(x_hat + 0.5), in the order (0, 0), (0, 1),
          (1, 0), (1, 1), * 0.25) (U, V); dist = clamp(fp32(t) * max_val, 0, max_val) in fp32; samples rint(dist), half to
          even, on all three planes.
"""
import numpy as np

f32, f16 = np.float32, np.float16


def max_val(bit_depth):
    assert 9 <= bit_depth <= 16
    return (1 << bit_depth) - 1


def read_picture(b, H, W):
    """one picture of a yuv420p<b>le file's bytes -> (y [H, W], uv [2, H/2, W/2]) uint16"""
    s = np.frombuffer(b, "<u2")
    return s[:H * W].reshape(H, W), s[H * W:].reshape(2, H // 2, W // 2)


def reader_scale(samples, bit_depth):
    """the reader's fp32 picture: fp32(v) / max_val"""
    return samples.astype(f32) / f32(max_val(bit_depth))


def yuv420p16_to_x(y, uv, bit_depth):
    """y [H, W], uv [2, H/2, W/2] uint16 -> the model input x [H, W, 3] fp16"""
    H, W = y.shape
    up = np.repeat(np.repeat(uv, 2, axis=1), 2, axis=2)[:, :H, :W]
    planes = [y, up[0], up[1]]
    return np.stack([(reader_scale(p, bit_depth).astype(f16).astype(f32) - f32(0.5)).astype(f16) for p in planes], axis=-1)


def _clamp(a, hi):
    # fmaxf / fminf: NaN becomes 0
    return np.fmin(np.fmax(a, f32(0)), f32(hi))


def x_to_yuv420p16(x_hat, H, W, bit_depth):
    """x_hat [Hp, Wp, 3] fp16 -> (dist_y [H, W] fp32, dist_uv [2, H/2, W/2] fp32, y16 [H, W] u16, uv16 [2, H/2, W/2] u16)"""
    m = f32(max_val(bit_depth))
    t = (x_hat[:H, :W].astype(f32) + f32(0.5)).astype(f16)
    dist_y = _clamp(t[..., 0].astype(f32) * m, m)
    c = t[..., 1:].astype(f32).transpose(2, 0, 1)
    s = ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + c[:, 1::2, 0::2]) + c[:, 1::2, 1::2]
    dist_uv = _clamp((s * f32(0.25)).astype(f16).astype(f32) * m, m)
    return dist_y, dist_uv, np.rint(dist_y).astype(np.uint16), np.rint(dist_uv).astype(np.uint16)


def sse(a, b):
    """fp64 sum of squared differences of two planes"""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float((d * d).sum())


def psnr(total, n, bit_depth):
    """metrics.py:10-24 calc_psnr at data range max_val from the fp64 sum of squares over n samples"""
    mse = total / n
    if np.isnan(mse) or np.isinf(mse):
        return -999.9
    peak = float(max_val(bit_depth))
    p = 10 * np.log10(peak * peak / mse) if mse > 1e-10 else 999.9
    return min(p, 99.9)


def psnr_yuv420(y, uv, dist_y, dist_uv, bit_depth):
    """[(6 y + u + v) / 8, y, u, v]"""
    py = psnr(sse(y, dist_y), y.size, bit_depth)
    pu = psnr(sse(uv[0], dist_uv[0]), uv[0].size, bit_depth)
    pv = psnr(sse(uv[1], dist_uv[1]), uv[1].size, bit_depth)
    return [(6 * py + pu + pv) / 8, py, pu, pv]


def all_codes(bit_depth, W=512):
    """(y, uv) uint16 holding every code 0..max_val at least once in Y and in each chroma plane (H W >= 4 * 2^b)"""
    n = 1 << bit_depth
    H = max(2, (4 * n + 2 * W - 1) // (2 * W) * 2)
    y = (np.arange(H * W, dtype=np.uint32) % n).astype(np.uint16).reshape(H, W)
    c = (H // 2) * (W // 2)
    uv = ((np.arange(2 * c, dtype=np.uint32) + 7) % n).astype(np.uint16).reshape(2, H // 2, W // 2)
    return y, uv
