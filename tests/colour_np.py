"""numpy restatement of dcvc_rgb_to_x_cs / dcvc_x_to_rgb_cs (include/dcvc_amd_ops.h): RGB <-> the codec's x with
a chosen colour matrix (bt601, bt709, bt2020) and range (full, limited at a YUV bit depth).

Written from the two sequences in the header, after rgb_np.py: every step is one fp32 (or fp16) numpy op on arrays, every
constant the fp32 value of the double expression it stands for. At bt709 / full the sequences are rgb_np's with
div="recip", operation for operation.
"""
import numpy as np

MATRICES = {"bt601": (0.299, 0.587, 0.114), "bt709": (0.2126, 0.7152, 0.0722), "bt2020": (0.2627, 0.6780, 0.0593)}
MATRIX_CODE = {"bt601": 0, "bt709": 1, "bt2020": 2}
RANGE_CODE = {"full": 0, "limited": 1}
f32, f16 = np.float32, np.float16


def levels(depth):
    """(lo, ry, mid, rc, iy, ic) of limited range at a YUV bit depth: one division in double each, then fp32"""
    s, m = float(1 << (depth - 8)), float((1 << depth) - 1)
    return tuple(f32(v) for v in (16 * s / m, 219 * s / m, 128 * s / m, 224 * s / m, m / (219 * s), m / (224 * s)))


def _clamp(a, lo, hi):
    # torch.clamp: NaN passes through
    return np.where(np.isnan(a), a, np.minimum(np.maximum(a, a.dtype.type(lo)), a.dtype.type(hi)))


def rgb_to_x(rgb, matrix="bt709", range="full", depth=8):
    """[3, H, W] u8 -> [H, W, 3] fp16 x"""
    kr, kg, kb = MATRICES[matrix]
    f = rgb.astype(f32) * (f32(1.0) / f32(255.0))
    r, g, b = f[0], f[1], f[2]
    y = (f32(kr) * r + f32(kg) * g) + f32(kb) * b
    pb = (f32(0.5) * (b - y)) * (f32(1.0) / f32(1 - kb))
    pr = (f32(0.5) * (r - y)) * (f32(1.0) / f32(1 - kr))
    if range == "limited":
        lo, ry, mid, rc, _, _ = levels(depth)
        ycc = (y * ry + lo, pb * rc + mid, pr * rc + mid)
    elif range == "full":
        ycc = (y, pb + f32(0.5), pr + f32(0.5))
    else:
        raise ValueError(range)
    return np.stack([(_clamp(c, 0.0, 1.0).astype(f16).astype(f32) - f32(0.5)).astype(f16) for c in ycc], axis=-1)


def x_to_rgb(x_hat, H, W, matrix="bt709", range="full", depth=8):
    """[Hp, Wp, 3] fp16 x_hat -> ([3, H, W] fp16 distortion planes in 0..255, [H, W, 3] u8 pixels; NaN -> 0)"""
    kr, kg, kb = MATRICES[matrix]
    with np.errstate(invalid="ignore", over="ignore"):
        xh = (x_hat[:H, :W].astype(f32) + f32(0.5)).astype(f16).astype(f32)
        y, cb, cr = xh[..., 0], xh[..., 1], xh[..., 2]
        if range == "limited":
            lo, _, mid, _, iy, ic = levels(depth)
            y, pb, pr = (y - lo) * iy, (cb - mid) * ic, (cr - mid) * ic
        elif range == "full":
            pb, pr = cb - f32(0.5), cr - f32(0.5)
        else:
            raise ValueError(range)
        r = y + f32(2 - 2 * kr) * pr
        b = y + f32(2 - 2 * kb) * pb
        g = ((y - f32(kr) * r) - f32(kb) * b) * (f32(1.0) / f32(kg))
        rgb16 = np.stack([_clamp((_clamp(c, 0.0, 1.0).astype(f16).astype(f32) * f32(255.0)).astype(f16), 0.0, 255.0)
                          for c in (r, g, b)])
        v = rgb16.astype(f32)
        rgb8 = np.rint(np.where(np.isnan(v), f32(0), v)).astype(np.uint8).transpose(1, 2, 0)
    return rgb16, np.ascontiguousarray(rgb8)


def exact_ycc(rgb, matrix, range, depth):
    """the matrix in closed form in float64, independent of the sequences above: [3, H, W] u8 -> (Y, Cb, Cr) on x's scale
    before the - 0.5 (sample value / (2^depth - 1))"""
    kr, kg, kb = MATRICES[matrix]
    r, g, b = (rgb[k].astype(np.float64) / 255.0 for k in (0, 1, 2))
    y = kr * r + kg * g + kb * b
    cb, cr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    if range == "full":
        return y, cb + 0.5, cr + 0.5
    s, m = float(1 << (depth - 8)), float((1 << depth) - 1)
    return (16 + 219 * y) * s / m, (128 + 224 * cb) * s / m, (128 + 224 * cr) * s / m
