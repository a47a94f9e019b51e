"""The denoising prefilter of DESIGN.md 26 (csrc/kernels/denoise.hip, dcvc encode --denoise) restated in numpy, operation for
operation, in signed 32-bit integers: the GPU tests hold the kernel and the tool against it with ==.

Per plane, sh = bit_depth - 8, Ts = spatial << sh, Tt = temporal << sh, indexes clamped to the plane (edge replication):
  spatial:  w_i = max(0, Ts - |n_i - c|) over the 3x3 neighbourhood, num = sum w_i (n_i - c), ws = sum w_i,
            sp = c + floor((2 num + ws) / (2 ws)); spatial == 0: sp = c.
  temporal: no prev or temporal == 0: out = sp. Else m = sum over the 3x3 neighbourhood q of |sp[q] - prev[q]| (sp at a clamped
            index is the sp of the clamped position), L = 9 Tt, k = (192 max(0, L - m)) // L,
            out = sp + ((k (prev - sp) + 128) >> 8).
"""
import numpy as np

I32 = np.int32


def _neighbours(a):
    """the 9 planes a[clamp(y + dy), clamp(x + dx)], dy, dx in -1..1"""
    p = np.pad(a, 1, mode="edge")
    H, W = a.shape
    return [p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]


def _dtype(bit_depth):
    if not 8 <= bit_depth <= 16:
        raise ValueError("bit_depth must be 8..16")
    return np.uint8 if bit_depth == 8 else np.uint16


def spatial_stage(cur, spatial, bit_depth):
    """cur [H, W] integer samples -> sp [H, W] int32"""
    c = np.asarray(cur).astype(I32)
    Ts = I32(int(spatial) << (bit_depth - 8))
    if spatial == 0:
        return c
    num = np.zeros(c.shape, I32)
    ws = np.zeros(c.shape, I32)
    for n in _neighbours(c):
        d = n - c
        w = np.maximum(I32(0), Ts - np.abs(d))
        num = num + w * d
        ws = ws + w
    return c + np.floor_divide(I32(2) * num + ws, I32(2) * ws)


def temporal_stage(sp, prev, temporal, bit_depth):
    """sp [H, W] int32, prev [H, W] integer samples or None -> out [H, W] int32"""
    if prev is None or temporal == 0:
        return sp
    p = np.asarray(prev).astype(I32)
    m = np.zeros(sp.shape, I32)
    for a, b in zip(_neighbours(sp), _neighbours(p)):
        m = m + np.abs(a - b)
    L = I32(9 * (int(temporal) << (bit_depth - 8)))
    k = (I32(192) * np.maximum(I32(0), L - m)) // L
    return sp + ((k * (p - sp) + I32(128)) >> I32(8))


def denoise_plane(cur, prev, spatial, temporal, bit_depth):
    """one plane (uint8 at 8 bits, uint16 above) and the same plane of the previous OUTPUT picture (or None) -> the output"""
    out = temporal_stage(spatial_stage(cur, spatial, bit_depth), prev, temporal, bit_depth)
    assert out.dtype == I32
    return out.astype(_dtype(bit_depth))


def denoise_clip(clip, spatial, temporal, bit_depth):
    """clip: a list of pictures, each a tuple of planes -> the filtered pictures, every plane on its own, in order"""
    out, prev = [], None
    for pic in clip:
        prev = tuple(denoise_plane(p, None if prev is None else prev[i], spatial, temporal, bit_depth) for i, p in enumerate(pic))
        out.append(prev)
    return out
