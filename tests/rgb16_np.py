"""numpy restatement of dcvc_rgb16_to_x_cs / dcvc_x_to_rgb16_cs (include/dcvc_amd_ops.h): 9..16-bit RGB <-> the
codec's x with a chosen colour matrix and range.

Written from the two sequences in the header, after colour_np.py, whose constants (MATRICES, levels) and clamp it shares: every
step is one fp32 (or fp16) numpy op on arrays. The unit value is a true fp32 division, fp32(v) / fp32(max_val) (numpy's
float32 division is correctly rounded), where the 8-bit pair multiplies by fp32(1 / 255); the distortion planes are fp32.
"""
import numpy as np

from colour_np import MATRICES, _clamp, levels

f32, f16 = np.float32, np.float16


def max_val(bit_depth):
    assert 9 <= bit_depth <= 16
    return (1 << bit_depth) - 1


def rgb16_to_x(rgb, bit_depth, matrix="bt709", range="full", depth=8):
    """[3, H, W] u16 -> [H, W, 3] fp16 x; samples above max_val are neither masked nor checked"""
    kr, kg, kb = MATRICES[matrix]
    f = rgb.astype(f32) / f32(max_val(bit_depth))
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


def x_to_rgb16(x_hat, H, W, bit_depth, matrix="bt709", range="full", depth=8):
    """[Hp, Wp, 3] fp16 x_hat -> ([3, H, W] fp32 distortion planes in 0..max_val (NaN passes through), [H, W, 3] u16 pixels;
    NaN -> 0)"""
    kr, kg, kb = MATRICES[matrix]
    m = f32(max_val(bit_depth))
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
        dist = np.stack([_clamp(_clamp(c, 0.0, 1.0).astype(f16).astype(f32) * m, 0.0, m) for c in (r, g, b)])
        out = np.rint(np.where(np.isnan(dist), f32(0), dist)).astype(np.uint16).transpose(1, 2, 0)
    return dist, np.ascontiguousarray(out)


def exact_ycc(rgb, bit_depth, matrix, range, depth):
    """the matrix in closed form in float64, independent of the sequences above: [3, H, W] u16 -> (Y, Cb, Cr) on x's scale
    before the - 0.5"""
    kr, kg, kb = MATRICES[matrix]
    r, g, b = (rgb[k].astype(np.float64) / float(max_val(bit_depth)) for k in (0, 1, 2))
    y = kr * r + kg * g + kb * b
    cb, cr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    if range == "full":
        return y, cb + 0.5, cr + 0.5
    s, m = float(1 << (depth - 8)), float((1 << depth) - 1)
    return (16 + 219 * y) * s / m, (128 + 224 * cb) * s / m, (128 + 224 * cr) * s / m


def exact_rgb(x_hat, bit_depth, matrix, range, depth):
    """the inverse in closed form in float64 from fp16 x_hat [..., 3]: (r, g, b) on the sample scale 0..max_val, clamped"""
    kr, kg, kb = MATRICES[matrix]
    v = x_hat.astype(np.float64) + 0.5
    y, cb, cr = v[..., 0], v[..., 1], v[..., 2]
    if range == "limited":
        s, m = float(1 << (depth - 8)), float((1 << depth) - 1)
        y, pb, pr = (y * m / s - 16) / 219, (cb * m / s - 128) / 224, (cr * m / s - 128) / 224
    else:
        pb, pr = cb - 0.5, cr - 0.5
    r = y + (2 - 2 * kr) * pr
    b = y + (2 - 2 * kb) * pb
    g = (y - kr * r - kb * b) / kg
    return tuple(np.clip(c, 0.0, 1.0) * max_val(bit_depth) for c in (r, g, b))
