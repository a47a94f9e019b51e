"""numpy restatement of the picture I/O for 4:2:0, 4:2:2, 4:4:4 planar and NV12 / P010 pictures of 8..16 bits, written from
the arithmetic stated in DESIGN.md ("Other chroma formats and Y4M"), one fp32 / fp16 numpy op per step:

  layout: Y [H][W], then Cb, Cr as planes [2][Hc][Wc] or, for NV12, interleaved [Hc][Wc][2]; Hc = H (H / 2 for 4:2:0 and
          NV12), Wc = W (W / 2 for all but 4:4:4). u8 at 8 bits, u16 at 9..16: LSB-aligned, NV12 in the high b bits.
  reader: v = sample (NV12 above 8 bits: v >> (16 - b)); d = fp16(fp32(v) / fp32(max_val)), x = fp16(fp32(d) - 0.5); chroma
          repeated over its 1, 2 or 2 x 2 luma positions.
  writer: t = fp16(fp32(x_hat) + 0.5); chroma t: the same (4:4:4), fp16((fp32(t_left) + fp32(t_right)) * 0.5) (4:2:2),
          fp16((((t00 + t01) + t10) + t11) * 0.25) in fp32 (4:2:0, NV12). dist: 8 bits fp32(clamp(fp16(fp32(t) * 255), 0,
          255)), 9..16 bits clamp(fp32(t) * max_val, 0, max_val) in fp32, NaN -> 0. samples: rint(dist), half to even, except
          Cb / Cr of the two 4:2:0 layouts at 8 bits, which truncate; NV12 above 8 bits stores s << (16 - b).
"""
import numpy as np

f32, f16 = np.float32, np.float16

YUV420P, YUV422P, YUV444P, NV12 = 0, 1, 2, 3
FORMATS = (YUV420P, YUV422P, YUV444P, NV12)


def max_val(bit_depth):
    assert 8 <= bit_depth <= 16
    return (1 << bit_depth) - 1


def sub(fmt):
    """(sub_h, sub_w): the shifts from a luma position to its chroma sample"""
    return (1 if fmt in (YUV420P, NV12) else 0), (0 if fmt == YUV444P else 1)


def plane_shapes(fmt, H, W):
    sh, sw = sub(fmt)
    return (H, W), (H >> sh, W >> sw)


def picture_samples(fmt, H, W):
    (_, _), (hc, wc) = plane_shapes(fmt, H, W)
    return H * W + 2 * hc * wc


def dtype(bit_depth):
    return np.uint8 if bit_depth == 8 else np.uint16


def shift(fmt, bit_depth):
    return 16 - bit_depth if fmt == NV12 and bit_depth > 8 else 0


def pack(y, cbcr, fmt, bit_depth):
    """LSB-aligned planes y [H, W], cbcr [2, Hc, Wc] -> one flat picture in file layout"""
    s = shift(fmt, bit_depth)
    dt = dtype(bit_depth)
    c = cbcr.transpose(1, 2, 0) if fmt == NV12 else cbcr
    return np.concatenate([(y.astype(np.uint32) << s).astype(dt).ravel(), (c.astype(np.uint32) << s).astype(dt).ravel()])


def unpack(pic, fmt, bit_depth, H, W):
    """one flat picture in file layout -> LSB-aligned planes (y [H, W], cbcr [2, Hc, Wc]); P010's low bits are dropped"""
    (_, _), (hc, wc) = plane_shapes(fmt, H, W)
    s = shift(fmt, bit_depth)
    y = pic[:H * W].reshape(H, W) >> s
    c = pic[H * W:]
    c = c.reshape(hc, wc, 2).transpose(2, 0, 1) if fmt == NV12 else c.reshape(2, hc, wc)
    return y, np.ascontiguousarray(c >> s)


def planar(pic, fmt, bit_depth, H, W):
    """the picture as flat LSB-aligned planar samples (Y, Cb, Cr)"""
    y, c = unpack(pic, fmt, bit_depth, H, W)
    return np.concatenate([y.ravel(), c.ravel()]).astype(dtype(bit_depth))


def to_x(pic, fmt, bit_depth, H, W):
    """one flat picture -> the model input x [H, W, 3] fp16"""
    y, c = unpack(pic, fmt, bit_depth, H, W)
    sh, sw = sub(fmt)
    up = np.repeat(np.repeat(c, 1 << sh, axis=1), 1 << sw, axis=2)
    m = f32(max_val(bit_depth))
    planes = [y, up[0], up[1]]
    return np.stack([((p.astype(f32) / m).astype(f16).astype(f32) - f32(0.5)).astype(f16) for p in planes], axis=-1)


def _clamp(a, hi):
    # fmaxf / fminf: NaN becomes 0
    return np.fmin(np.fmax(a, f32(0)), f32(hi))


def chroma_t(t, fmt):
    """t [H, W, 3] fp16 (x_hat + 0.5) -> the chroma planes' t [2, Hc, Wc] fp16"""
    c = t[..., 1:].astype(f32).transpose(2, 0, 1)
    sh, sw = sub(fmt)
    with np.errstate(invalid="ignore", over="ignore"):
        if sh:
            s = ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2]) + c[:, 1::2, 0::2]) + c[:, 1::2, 1::2]
            return (s * f32(0.25)).astype(f16)
        if sw:
            return ((c[:, :, 0::2] + c[:, :, 1::2]) * f32(0.5)).astype(f16)
    return np.ascontiguousarray(c).astype(f16)


def from_x(x_hat, H, W, fmt, bit_depth):
    """x_hat [Hp, Wp, 3] fp16 -> (dist32: flat fp32 planar Y, Cb, Cr; samples: one flat picture in file layout)"""
    m = f32(max_val(bit_depth))
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x_hat[:H, :W].astype(f32) + f32(0.5)).astype(f16)
        tc = chroma_t(t, fmt)

        def dist_of(p):
            if bit_depth == 8:
                return _clamp((p.astype(f32) * f32(255)).astype(f16).astype(f32), 255)
            return _clamp(p.astype(f32) * m, m)

        dy, dc = dist_of(t[..., 0]), dist_of(tc)
    truncate = bit_depth == 8 and sub(fmt)[0] == 1
    sy = np.rint(dy).astype(np.uint32)
    sc = (np.trunc(dc) if truncate else np.rint(dc)).astype(np.uint32)
    return np.concatenate([dy.ravel(), dc.ravel()]), pack(sy, sc, fmt, bit_depth)


def all_codes(fmt, bit_depth, H, W, low_bits=0, chroma_start=7):
    """one flat picture holding the codes 0, 1, 2, ... (mod 2^b) in file order in Y and chroma_start, chroma_start + 1, ... in
    the chroma samples, so that a picture of at least 2^b luma and 2^b chroma samples holds every code in Y and in chroma;
    NV12 above 8 bits: `low_bits` ORed below the value"""
    n = picture_samples(fmt, H, W)
    v = np.arange(n, dtype=np.uint32) % (1 << bit_depth)
    v[H * W:] = (np.arange(n - H * W, dtype=np.uint32) + chroma_start) % (1 << bit_depth)
    s = shift(fmt, bit_depth)
    return ((v << s) | (low_bits & ((1 << s) - 1))).astype(dtype(bit_depth))


def all_halfs():
    """every fp16 bit pattern (NaN and the infinities included) as x_hat [256, 256, 3]: channel c holds the patterns rotated
    by 21845 c, so that every channel sees all of them"""
    bits = np.arange(65536, dtype=np.uint32)
    return np.stack([((bits + 21845 * c) % 65536).astype(np.uint16).view(f16).reshape(256, 256) for c in range(3)], axis=-1)
