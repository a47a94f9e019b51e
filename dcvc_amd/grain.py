"""Film grain (no reference counterpart): what ``dcvc encode --denoise`` removes is measured on the GPU and put
back, as statistically equivalent synthetic grain, onto decoded pictures. ``grain_apply`` and ``grain_stats`` are thin wrappers
over ``dcvc_grain_apply`` and ``dcvc_grain_stats`` (include/dcvc_amd_ops.h, csrc/kernels/grain.hip) on
``torch.cuda.current_stream()``; ``grain_template`` and ``grain_fit`` restate the host functions ``dcvc_grain_template`` and
``dcvc_grain_fit`` (include/dcvc_amd_rc.h) operation for operation in Python integers. tests/grain_np.py restates all four in
numpy.

Sample tensors are ``torch.uint8`` (bit depth 8), or 16-bit as yuv16.py takes and returns them (bit depth 9..16).
"""
import ctypes
import math

from . import _lib
from .yuv16 import DCVC_SAMPLE_U8, DCVC_SAMPLE_U16, _u16_dtypes, u16_dtype

MAX_SIZE = 37
MAX_FLAT = 255
MAX_GAIN = 400
_M32 = 0xFFFFFFFF

_vp, _ci, _ll, _u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint32
_fns = {}


def _fn(name, argtypes):
    if name not in _fns:
        _fns[name] = _lib.fn(name, _ci, argtypes)
    return _fns[name]


def grain_template(seed, plane, size):
    """dcvc_grain_template in Python: the 64 x 64 template of (seed, plane 0..2, size 0..37) as 64 lists of 64 ints, a standard
    deviation of about 64 and a lag-1 correlation of about 2ab / (2a^2 + b^2), a = size, b = 128 - 2a."""
    seed, plane, size = int(seed), int(plane), int(size)
    if not 0 <= plane <= 2:
        raise ValueError("grain_template: plane must be in 0..2, got %d" % plane)
    if not 0 <= size <= MAX_SIZE:
        raise ValueError("grain_template: size must be in 0..37, got %d" % size)
    s = (seed * 0x9E3779B1 + plane * 0xC2B2AE3D + 1) & _M32
    w = []
    for _ in range(64):
        row = []
        for _ in range(64):
            t = 0
            for _ in range(4):
                s = (s * 1664525 + 1013904223) & _M32
                t += s >> 24
            row.append(t - 510)
        w.append(row)
    a, b = size, 128 - 2 * size
    h = [[a * r[x - 1] + b * r[x] + a * r[(x + 1) & 63] for x in range(64)] for r in w]
    f = [[a * h[y - 1][x] + b * h[y][x] + a * h[(y + 1) & 63][x] for x in range(64)] for y in range(64)]
    rms = math.isqrt(sum(v * v for r in f for v in r) // 4096)
    if rms == 0:
        raise ValueError("grain_template: the filtered noise is zero")
    T = [[(128 * v + rms) // (2 * rms) for v in r] for r in f]
    if max(abs(v) for r in T for v in r) > 1023:
        raise ValueError("grain_template: a template value is outside -1023..1023")
    return T


def grain_fit(words, bit_depth, gain_percent=100, min_count=256):
    """dcvc_grain_fit in Python. words: three sequences (Y, U, V) of the 16 words of ``grain_stats``, summed over a window of
    pictures -> three tables of nine ints 0..255: the grain's standard deviation in sixteenths of an 8-bit code value at luma
    0, 32, .., 256. A bin below min_count samples takes the nearest valid bin's value (ties: the lower bin); a plane without a
    valid bin gets zeros."""
    bit_depth, gain, min_count = int(bit_depth), int(gain_percent), int(min_count)
    if not 8 <= bit_depth <= 16:
        raise ValueError("grain_fit: bit_depth must be in 8..16, got %d" % bit_depth)
    if not 1 <= gain <= MAX_GAIN:
        raise ValueError("grain_fit: gain_percent must be in 1..400, got %d" % gain)
    if min_count < 1:
        raise ValueError("grain_fit: min_count must be at least 1, got %d" % min_count)
    words = [[int(v) for v in w] for w in words]
    if len(words) != 3 or any(len(w) != 16 for w in words):
        raise ValueError("grain_fit: three times 16 words expected")
    if any(not 0 <= v < 1 << 63 for w in words for v in w):
        raise ValueError("grain_fit: a word is 2^63 or above")
    sh = bit_depth - 8
    luts = []
    for w in words:
        n, S = w[:8], w[8:]
        valid = [n[k] >= min_count for k in range(8)]
        if not any(valid):
            luts.append([0] * 9)
            continue
        bins = [min(255, math.isqrt((256 * S[k] * gain * gain) // ((n[k] * 10000) << (2 * sh)))) if valid[k] else 0 for k in range(8)]
        full = []
        for k in range(8):
            for dist in range(8):                    # the nearest valid bin, the lower one first
                if k - dist >= 0 and valid[k - dist]:
                    full.append(bins[k - dist])
                    break
                if k + dist < 8 and valid[k + dist]:
                    full.append(bins[k + dist])
                    break
        luts.append([full[0]] + [(full[k - 1] + full[k] + 1) >> 1 for k in range(1, 8)] + [full[7]])
    return luts


def _code(t, who):
    import torch
    if t.dtype == torch.uint8:
        return DCVC_SAMPLE_U8, torch.uint8
    if t.dtype in _u16_dtypes():
        return DCVC_SAMPLE_U16, u16_dtype()
    raise TypeError("%s: planes must be uint8 or uint16 / int16 (unsigned samples), got %s" % (who, t.dtype))


def _planes(t, who):
    squeeze = t.dim() == 2
    p = t[None] if squeeze else t
    if p.dim() != 3 or not p.is_cuda:
        raise ValueError("%s: CUDA planes [P, H, W] or [H, W] expected, got %s" % (who, tuple(t.shape)))
    return p, squeeze


def _luma(luma, t, who):
    if luma.dim() != 2 or luma.device != t.device or luma.element_size() != t.element_size() or luma.dtype.is_floating_point:
        raise ValueError("%s: luma must be a plane [Hl, Wl] of the planes' sample width on their device" % who)
    return luma if luma.stride(1) == 1 else luma.contiguous()


def grain_apply(rec, luma, templates, lut, seed, pic, first_plane, bit_depth, sx, sy, out=None):
    """rec: [P, H, W] or [H, W] CUDA samples, planes first_plane .. first_plane + P - 1 of Y, U, V, unit stride along a row (row
    and plane strides may be larger); luma: the UNGRAINED luma plane [Hl, Wl] they share, against which they are subsampled by
    (sx, sy) in {0, 1} - for the luma plane itself pass rec. templates: a CUDA int16 tensor [3, 64, 64] (``grain_template`` of
    planes 0, 1, 2); lut: three tables of nine ints 0..255. out: a tensor of rec's shape to write into (strided likewise; it may
    be rec), else a new contiguous one. Returns out."""
    import torch
    t, squeeze = _planes(rec, "grain_apply")
    code, out_dtype = _code(t, "grain_apply")
    in_place = out is rec
    if t.stride(2) != 1:
        if in_place:
            raise ValueError("grain_apply: rows at unit stride expected in place")
        t = t.contiguous()
    P, H, W = t.shape
    if luma is rec and squeeze:
        y = t[0]
    else:
        y = _luma(luma, t, "grain_apply")
    if (templates.dtype != torch.int16 or tuple(templates.shape) != (3, 64, 64) or templates.device != t.device
            or not templates.is_contiguous()):
        raise ValueError("grain_apply: templates must be a contiguous int16 tensor [3, 64, 64] on rec's device")
    table = [int(v) for row in lut for v in row]
    if len(table) != 27 or any(not 0 <= v <= 255 for v in table):
        raise ValueError("grain_apply: lut must hold three tables of nine values in 0..255")
    if not 0 <= int(seed) <= _M32 or not 0 <= int(pic) <= _M32:
        raise ValueError("grain_apply: seed and pic must fit 32 bits")
    if out is None:
        o = torch.empty((P, H, W), dtype=out_dtype, device=t.device)
    elif in_place:
        o = t
    else:
        o = out[None] if out.dim() == 2 else out
        if (tuple(o.shape) != (P, H, W) or o.device != t.device or o.stride(2) != 1 or o.element_size() != t.element_size()
                or o.dtype.is_floating_point):
            raise ValueError("grain_apply: out must hold [%d, %d, %d] samples of rec's width on rec's device, rows at unit stride" % (P, H, W))
    tp = [_vp(templates[p].data_ptr()) for p in range(3)]
    _lib.check(_fn("dcvc_grain_apply", [_vp, _ci, _ll, _vp, _ci, _ci, _ci, _vp, _ci, _ll, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp,
                                        _vp, ctypes.c_char_p, _u32, _u32, _vp])(
        _vp(t.data_ptr()), t.stride(1), t.stride(0), _vp(y.data_ptr()), y.stride(0), y.shape[0], y.shape[1], _vp(o.data_ptr()),
        o.stride(1), o.stride(0), code, int(bit_depth), H, W, P, int(first_plane), int(sx), int(sy), tp[0], tp[1], tp[2], bytes(table),
        int(seed), int(pic), _vp(torch.cuda.current_stream(t.device).cuda_stream)))
    if out is not None:
        return out
    return o[0] if squeeze else o


def grain_stats(src, den, luma, bit_depth, sx, sy, flat, out=None, accumulate=False):
    """src, den: [P, H, W] or [H, W] CUDA samples (P <= 2) - source planes and the denoiser's output for them - unit stride
    along a row; luma: DEN's luma plane [Hl, Wl] (for the luma plane itself pass den). flat: 0..255 in 8-bit code values. Returns
    a CUDA int64 tensor [P, 16] (or [16]): per plane the counts n[0..7] and the sums S[0..7] of (src - den)^2 of the samples in
    flat surroundings, by luma bin - out, a contiguous one on src's device, when given: zeroed first, or added to with
    accumulate."""
    import torch
    s, squeeze = _planes(src, "grain_stats")
    code, _ = _code(s, "grain_stats")
    if s.stride(2) != 1:
        s = s.contiguous()
    P, H, W = s.shape
    d = den[None] if den.dim() == 2 else den
    if tuple(d.shape) != (P, H, W) or d.device != s.device or d.element_size() != s.element_size() or d.dtype.is_floating_point:
        raise ValueError("grain_stats: den must hold src's planes: [%d, %d, %d] samples of src's width on src's device" % (P, H, W))
    if d.stride(2) != 1:
        d = d.contiguous()
    y = d[0] if (luma is den and squeeze) else _luma(luma, s, "grain_stats")
    shape = (16,) if squeeze else (P, 16)
    if out is None:
        if accumulate:
            raise ValueError("grain_stats: accumulate needs out")
        out = torch.empty(shape, dtype=torch.int64, device=s.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != shape or out.device != s.device or not out.is_contiguous():
        raise ValueError("grain_stats: out must be a contiguous int64 tensor %s on src's device" % (list(shape),))
    _lib.check(_fn("dcvc_grain_stats", [_vp, _ci, _ll, _vp, _ci, _ll, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp,
                                        _vp])(
        _vp(s.data_ptr()), s.stride(1), s.stride(0), _vp(d.data_ptr()), d.stride(1), d.stride(0), _vp(y.data_ptr()), y.stride(0),
        y.shape[0], y.shape[1], code, int(bit_depth), H, W, P, int(sx), int(sy), int(flat), 1 if accumulate else 0,
        _vp(out.data_ptr()), _vp(torch.cuda.current_stream(s.device).cuda_stream)))
    return out


__all__ = ["grain_template", "grain_fit", "grain_apply", "grain_stats", "MAX_SIZE", "MAX_FLAT", "MAX_GAIN"]
