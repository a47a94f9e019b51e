"""numpy restatement of the wire formats, written from the table of layouts; it imports nothing of the library.

One picture, little-endian, as a flat uint8 array of picture_bytes bytes:
  nv21   Y [H][W], then [H/2][W/2][2] as Cr, Cb; 8 bits                                                carrier NV12
  nv16   Y [H][W], then [H][W/2][2] as Cb, Cr; above 8 bits u16 with the value in the high b bits       carrier YUV422P
  uyvy   [H][W/2] x (Cb, Y0, Cr, Y1) bytes; 8 bits                                                      carrier YUV422P
  yuy2   [H][W/2] x (Y0, Cb, Y1, Cr); above 8 bits u16 with the value in the high b bits                carrier YUV422P
  v210   rows of 128 ceil(W / 48) bytes; 6 pixels in four 32-bit words, three 10-bit fields each at bits 0-9, 10-19, 20-29:
         w0 = Cb0 Y0 Cr0, w1 = Y1 Cb2 Y2, w2 = Cr2 Y3 Cb4, w3 = Y4 Cr4 Y5; 10 bits                      carrier YUV422P
The carrier is a flat array in file layout, uint8 at 8 bits and uint16 above: YUV422P = Y [H][W], Cb [H][W/2], Cr [H][W/2],
LSB-aligned; NV12 = Y [H][W], then [H/2][W/2][2] as Cb, Cr.
  unpack: high-aligned samples v >> (16 - b); v210 fields & 1023; low bits, bits 30-31, fields past W, row padding ignored.
  pack:   (s << (16 - b)) & 0xFFFF; v210 fields s & 1023; bits 30-31, fields past W and the row padding zero.
"""
import numpy as np

NV21, NV16, UYVY, YUY2, V210 = 0, 1, 2, 3, 4
NAMES = {"nv21": NV21, "nv16": NV16, "uyvy": UYVY, "yuy2": YUY2, "v210": V210}
PIX_YUV422P, PIX_NV12 = 1, 3
# every (format, depth) the formats have
DEPTHS = {NV21: (8,), NV16: tuple(range(8, 17)), UYVY: (8,), YUY2: tuple(range(8, 17)), V210: (10,)}
# the 12 fields of a v210 group in wire order, as (plane, index in the group): plane 0 Y (6 per group), 1 Cb, 2 Cr (3 each)
V210_FIELDS = [(1, 0), (0, 0), (2, 0), (0, 1), (1, 1), (0, 2), (2, 1), (0, 3), (1, 2), (0, 4), (2, 2), (0, 5)]


def carrier(wire):
    return PIX_NV12 if wire == NV21 else PIX_YUV422P


def dtype(bit_depth):
    return np.uint8 if bit_depth == 8 else np.uint16


def v210_row_bytes(W):
    return 128 * ((W + 47) // 48)


def picture_bytes(wire, bit_depth, H, W):
    assert bit_depth in DEPTHS[wire] and H > 0 and W > 0 and H % 2 == 0 and W % 2 == 0
    if wire == V210:
        return H * v210_row_bytes(W)
    samples = H * W * 3 // 2 if wire == NV21 else 2 * H * W
    return samples * (1 if bit_depth == 8 else 2)


def carrier_samples(wire, H, W):
    return H * W * 3 // 2 if wire == NV21 else 2 * H * W


def _planes(c, wire, H, W):
    """flat carrier -> (y [H, W], cb [Hc, W/2], cr [Hc, W/2]) as uint32"""
    c = c.astype(np.uint32)
    y = c[:H * W].reshape(H, W)
    if wire == NV21:
        uv = c[H * W:].reshape(H // 2, W // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    cb = c[H * W:H * W + H * (W // 2)].reshape(H, W // 2)
    cr = c[H * W + H * (W // 2):].reshape(H, W // 2)
    return y, cb, cr


def _carrier_of(y, cb, cr, wire, bit_depth):
    dt = dtype(bit_depth)
    if wire == NV21:
        return np.concatenate([y.ravel(), np.stack([cb, cr], axis=-1).ravel()]).astype(dt)
    return np.concatenate([y.ravel(), cb.ravel(), cr.ravel()]).astype(dt)


def v210_words(fields):
    """twelve 10-bit fields of one group in wire order -> its four 32-bit words"""
    f = [int(v) & 1023 for v in fields]
    return [f[3 * k] | f[3 * k + 1] << 10 | f[3 * k + 2] << 20 for k in range(4)]


def pack(c, wire, bit_depth, H, W):
    """flat carrier picture -> the wire picture as a flat uint8 array"""
    assert c.size == carrier_samples(wire, H, W)
    y, cb, cr = _planes(np.asarray(c), wire, H, W)
    if wire == V210:
        groups = (W + 5) // 6
        planes = []
        for p, per in ((y, 6), (cb, 3), (cr, 3)):                # zero beyond W, whole groups
            z = np.zeros((H, groups * per), dtype=np.uint32)
            z[:, :p.shape[1]] = p & 1023
            planes.append(z.reshape(H, groups, per))
        f = np.stack([planes[p][:, :, k] for p, k in V210_FIELDS], axis=-1)          # [H, groups, 12]
        words = f[..., 0::3] | f[..., 1::3] << 10 | f[..., 2::3] << 20               # [H, groups, 4]
        rows = np.zeros((H, v210_row_bytes(W) // 4), dtype="<u4")
        rows[:, :groups * 4] = words.reshape(H, groups * 4)
        return rows.view(np.uint8).ravel().copy()
    s = 16 - bit_depth if bit_depth > 8 else 0
    dt = np.dtype(dtype(bit_depth)).newbyteorder("<")
    hi = lambda a: ((a << s) & 0xFFFF).astype(dt) if s else a.astype(dt)
    if wire == NV21:
        out = np.concatenate([hi(y).ravel(), np.stack([hi(cr), hi(cb)], axis=-1).ravel()])
    elif wire == NV16:
        out = np.concatenate([hi(y).ravel(), np.stack([hi(cb), hi(cr)], axis=-1).ravel()])
    else:
        y0, y1 = hi(y[:, 0::2]), hi(y[:, 1::2])
        order = [hi(cb), y0, hi(cr), y1] if wire == UYVY else [y0, hi(cb), y1, hi(cr)]
        out = np.stack(order, axis=-1).ravel()
    return np.ascontiguousarray(out).view(np.uint8).copy()


def unpack(p, wire, bit_depth, H, W):
    """the wire picture (flat uint8 array) -> its flat carrier picture"""
    p = np.asarray(p, dtype=np.uint8)
    assert p.size == picture_bytes(wire, bit_depth, H, W)
    if wire == V210:
        groups = (W + 5) // 6
        words = p.view("<u4").reshape(H, -1)[:, :groups * 4].astype(np.uint32).reshape(H, groups, 4)
        f = np.stack([(words[..., k // 3] >> (10 * (k % 3))) & 1023 for k in range(12)], axis=-1)      # [H, groups, 12]
        planes = [np.zeros((H, groups, per), dtype=np.uint32) for per in (6, 3, 3)]
        for k, (pl, idx) in enumerate(V210_FIELDS):
            planes[pl][:, :, idx] = f[..., k]
        y, cb, cr = (planes[i].reshape(H, -1) for i in range(3))
        return _carrier_of(y[:, :W], cb[:, :W // 2], cr[:, :W // 2], wire, bit_depth)
    s = 16 - bit_depth if bit_depth > 8 else 0
    v = p.view(np.dtype(dtype(bit_depth)).newbyteorder("<")).astype(np.uint32) >> s
    if wire in (NV21, NV16):
        hc = H // 2 if wire == NV21 else H
        y = v[:H * W].reshape(H, W)
        uv = v[H * W:].reshape(hc, W // 2, 2)
        cb, cr = (uv[..., 1], uv[..., 0]) if wire == NV21 else (uv[..., 0], uv[..., 1])
        return _carrier_of(y, cb, cr, wire, bit_depth)
    q = v.reshape(H, W // 2, 4)
    iy0, icb, iy1, icr = (1, 0, 3, 2) if wire == UYVY else (0, 1, 2, 3)
    y = np.stack([q[..., iy0], q[..., iy1]], axis=-1).reshape(H, W)
    return _carrier_of(y, q[..., icb], q[..., icr], wire, bit_depth)


def ignored_mask(wire, bit_depth, H, W):
    """uint8 array of picture_bytes bytes: the bits of the wire picture that unpack ignores and pack writes as zero"""
    n = picture_bytes(wire, bit_depth, H, W)
    if wire == V210:
        rows = np.full((H, v210_row_bytes(W) // 4), 0xFFFFFFFF, dtype="<u4")
        groups = (W + 5) // 6
        live = np.zeros((H, groups, 4), dtype=np.uint32)
        counts = (W, W // 2, W // 2)
        per = (6, 3, 3)
        for g in range(groups):
            for k, (pl, idx) in enumerate(V210_FIELDS):
                if g * per[pl] + idx < counts[pl]:
                    live[:, g, k // 3] |= np.uint32(1023 << (10 * (k % 3)))
        rows[:, :groups * 4] = ~live.reshape(H, groups * 4)
        return rows.view(np.uint8).ravel().copy()
    if bit_depth == 8 or bit_depth == 16:
        return np.zeros(n, dtype=np.uint8)
    return np.full(n // 2, (1 << (16 - bit_depth)) - 1, dtype="<u2").view(np.uint8).copy()


def random_carrier(rng, wire, bit_depth, H, W):
    """seeded samples over the full code range 0 .. 2^b - 1"""
    return rng.integers(0, 1 << bit_depth, carrier_samples(wire, H, W), dtype=np.uint32).astype(dtype(bit_depth))
