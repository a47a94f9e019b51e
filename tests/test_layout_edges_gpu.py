"""The layout kernels (kernels/layout.hip) and the small elementwise kernels (round_z, int8_to_half, mul_channel,
scale_clamped) at their edges, on a real MI355X (-m gpu), through the C ABI. Every reference is a plain numpy gather or one
fp16 operation per element (oracle/symbols_np.py where the reference defines it), every comparison is on the fp16 bit patterns,
and every output has NaN-payload sentinels around it. No refusal is tried here (tests/test_ops_refusals_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symbol_cases as S  # noqa: E402
from gpu_util import Rows, at, call, guarded, stream, tail_intact  # noqa: E402
from oracle import symbols_np as orc  # noqa: E402

pytestmark = pytest.mark.gpu

F16 = np.float16
XS = (3.0, -0.333, 65504.0, 6e-8)         # the other operand of the multiplies: plain, negative, the largest, a subnormal


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "needs the MI355X"
    from gpu_util import Ops
    return Ops()


def _patterns(shape, seed):
    """random non-NaN fp16 bit patterns: a gather must move any of them unchanged"""
    pat = S.non_nan_patterns()
    return pat[np.random.default_rng(seed).integers(0, pat.size, size=shape)].view(F16)


def _same_bits(got, want):
    return np.array_equal(S.bits(got), S.bits(want))


def _wide(C, wide):
    return C + 24 if wide else C


# ------------------------------------------------------------------------------------------------------------ pad_unshuffle8
def _pad_unshuffle8(x, H8, W8):
    H, W, C3 = x.shape
    hh = np.minimum(np.arange(H8 * 8), H - 1)
    ww = np.minimum(np.arange(W8 * 8), W - 1)
    xp = x[hh][:, ww]                                                      # [H8*8][W8*8][C3], edges replicated
    return xp.reshape(H8, 8, W8, 8, C3).transpose(0, 2, 4, 1, 3).reshape(H8, W8, C3 * 64)     # channel c*64 + dy*8 + dx


@pytest.mark.parametrize("wide", [False, True], ids=["dense", "into_a_wider_row"])
@pytest.mark.parametrize("C3", [3, 24])
@pytest.mark.parametrize("H,W", [(2, 2), (8, 8), (9, 17), (70, 100)])
def test_pad_unshuffle8(ops, H, W, C3, wide):
    H8, W8 = (H + 7) // 8, (W + 7) // 8
    x = _patterns((H, W, C3), 11)
    xd = guarded(x.size, torch.int16)
    xd[:x.size] = torch.from_numpy(x.view(np.int16).reshape(-1)).cuda()
    out = Rows(None, 64 * C3, _wide(64 * C3, wide), fill=(H8 * W8, 7.0))
    if wide:
        call(ops.pad_unshuffle8_ld, at(xd), H, W, C3, out.ptr(), out.ld, H8, W8, stream())
    else:
        call(ops.pad_unshuffle8, at(xd), H, W, C3, out.ptr(), H8, W8, stream())
    torch.cuda.synchronize()
    assert _same_bits(out.get().reshape(H8, W8, 64 * C3), _pad_unshuffle8(x, H8, W8))
    assert out.around_intact()


def test_pad_unshuffle8_ld_at_the_dense_width_is_the_dense_entry(ops):
    H, W, C3 = 9, 17, 3
    x = _patterns((H, W, C3), 12)
    xd = torch.from_numpy(x.view(np.int16).reshape(-1)).cuda()
    out = Rows(None, 192, fill=(2 * 3, 7.0))
    call(ops.pad_unshuffle8_ld, at(xd), H, W, C3, out.ptr(), 192, 2, 3, stream())
    torch.cuda.synchronize()
    assert _same_bits(out.get().reshape(2, 3, 192), _pad_unshuffle8(x, 2, 3)) and out.around_intact()


# ------------------------------------------------------------------------------------------------------------ shuffle8
def _shuffle8(v, clamp):
    H8, W8, C = v.shape
    C3 = C // 64
    if clamp:
        v = np.clip(v, F16(-0.5), F16(0.5))
    return np.ascontiguousarray(v.reshape(H8, W8, C3, 8, 8).transpose(0, 3, 1, 4, 2).reshape(H8 * 8, W8 * 8, C3))


@pytest.mark.parametrize("wide", [False, True], ids=["ldin_64C3", "ldin_wider"])
@pytest.mark.parametrize("clamp", [0, 1], ids=["plain", "clamp"])
@pytest.mark.parametrize("H8,W8,C3", [(19, 18, 3), (2, 3, 24), (1, 1, 3)])
def test_shuffle8(ops, H8, W8, C3, clamp, wide):
    C = 64 * C3
    v = _patterns((H8 * W8 * C,), 21)
    pat = S.non_nan_patterns().view(F16)
    if v.size >= pat.size:
        v[:pat.size] = pat                                    # every non-NaN pattern through the clamp
        want_flat = np.clip(pat, F16(-0.5), F16(0.5))
        for a, b in ((0.5, 0.5), (0.5005, 0.5), (0.4998, 0.4998), (-0.5005, -0.5), (-0.4998, -0.4998), (np.inf, 0.5), (-np.inf, -0.5)):
            assert want_flat[pat == F16(a)][0] == F16(b)      # both sides of +-0.5 and the infinities are in, clipped as expected
        assert S.bit(want_flat[S.bits(pat) == 0x8000][0]) == 0x8000
    v = v.reshape(H8, W8, C)
    src = Rows(v, C, _wide(C, wide))
    n = H8 * W8 * C
    out = guarded(n, torch.int16)
    call(ops.shuffle8, src.ptr(), src.ld, H8, W8, C3, clamp, at(out), stream())
    torch.cuda.synchronize()
    got = out[:n].cpu().numpy().view(F16).reshape(H8 * 8, W8 * 8, C3)
    assert _same_bits(got, _shuffle8(v, clamp))
    assert tail_intact(out, n) and src.around_intact() and _same_bits(src.get().reshape(v.shape), v)


# ------------------------------------------------------------------------------------------------------------ shuffle2 / pad / crop
@pytest.mark.parametrize("C", [8, 512])
@pytest.mark.parametrize("H,W", [(5, 7), (1, 1)])
def test_shuffle2_strided(ops, H, W, C):
    v = _patterns((H, W, 4 * C), 31)
    src = Rows(v, 4 * C, 4 * C + 24)
    out = Rows(None, C, C + 24, fill=(4 * H * W, 7.0))
    call(ops.shuffle2, src.ptr(), src.ld, H, W, C, out.ptr(), out.ld, stream())
    torch.cuda.synchronize()
    want = v.reshape(H, W, C, 2, 2).transpose(0, 3, 1, 4, 2).reshape(2 * H, 2 * W, C)       # in channel c*4 + i*2 + j
    assert _same_bits(out.get().reshape(2 * H, 2 * W, C), want) and out.around_intact()


@pytest.mark.parametrize("C", [8, 512])
@pytest.mark.parametrize("H,W,pad_b,pad_r", [(9, 7, 3, 1), (9, 7, 0, 0), (9, 7, 0, 2), (1, 1, 5, 0)])
def test_replicate_pad_strided(ops, H, W, pad_b, pad_r, C):
    """pad_b = pad_r = 0 is the strided copy of the inter models' state export"""
    v = _patterns((H, W, C), 41)
    src = Rows(v, C, C + 24)
    Ho, Wo = H + pad_b, W + pad_r
    out = Rows(None, C, C + 40, fill=(Ho * Wo, 7.0))
    call(ops.replicate_pad, src.ptr(), src.ld, H, W, C, pad_b, pad_r, out.ptr(), out.ld, stream())
    torch.cuda.synchronize()
    want = v[np.minimum(np.arange(Ho), H - 1)][:, np.minimum(np.arange(Wo), W - 1)]
    assert _same_bits(out.get().reshape(Ho, Wo, C), want) and out.around_intact()


@pytest.mark.parametrize("C", [8, 512])
@pytest.mark.parametrize("Hin,Win,H,W", [(12, 8, 9, 7), (9, 7, 9, 7), (4, 5, 1, 1)])
def test_crop_strided(ops, Hin, Win, H, W, C):
    v = _patterns((Hin, Win, C), 51)
    src = Rows(v, C, C + 40)
    out = Rows(None, C, C + 24, fill=(H * W, 7.0))
    call(ops.crop, src.ptr(), src.ld, Win, out.ptr(), out.ld, H, W, C, stream())
    torch.cuda.synchronize()
    assert _same_bits(out.get().reshape(H, W, C), v[:H, :W]) and out.around_intact()


# ------------------------------------------------------------------------------------------------------------ multiplies
@pytest.fixture(scope="module")
def sweep():
    """q = every non-NaN fp16 pattern against each x of XS"""
    pat = S.non_nan_patterns().view(F16)
    return {"pat": pat, "x": np.repeat(np.array(XS, dtype=F16), pat.size), "q": np.tile(pat, len(XS))}


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("reciprocal", [0, 1], ids=["times_max_q", "times_rcp_max_q"])
def test_scale_clamped_every_q(ops, sweep, reciprocal, inplace):
    """y = x * max(q, 0.5) and y = x * fp16(1 / max(q, 0.5)): three different leading dimensions (in place: x and y are one)"""
    C = 40                                      # five 16-byte vectors per pixel
    assert sweep["x"].size % C == 0
    x = Rows(sweep["x"], C, C + 8)
    q = Rows(sweep["q"], C, C + 16)
    y = x if inplace else Rows(None, C, C + 24, fill=(x.pixels, 7.0))
    call(ops.scale_clamped, x.ptr(), x.ld, q.ptr(), q.ld, y.ptr(), y.ld, x.pixels, C, reciprocal, stream())
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):
        want = orc.divide_with_clamp(sweep["x"], sweep["q"]) if reciprocal else (sweep["x"] * orc.clamp_min_half(sweep["q"])).astype(F16)
    assert not np.isnan(want).any() and np.isinf(want).any() and (want == 0).any()
    assert _same_bits(y.get().reshape(-1), want)
    assert y.around_intact() and q.around_intact() and x.around_intact()
    assert inplace or _same_bits(x.get().reshape(-1), sweep["x"])


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
def test_mul_channel_every_q(ops, sweep, inplace):
    """y[p][c] = x[p][c] * q[c]: one pixel per x of XS, a channel per pattern; out of place between two different leading
    dimensions, in place inside a wider row"""
    pat = sweep["pat"]
    C = (pat.size + 7) // 8 * 8
    q = np.ones(C, F16)
    q[:pat.size] = pat
    xv = np.repeat(np.array(XS, dtype=F16), C).reshape(len(XS), C)
    x = Rows(xv, C, C + 8)
    y = x if inplace else Rows(None, C, C + 24, fill=(len(XS), 7.0))
    qd = guarded(C, torch.int16)
    qd[:C] = torch.from_numpy(q.view(np.int16)).cuda()
    call(ops.mul_channel, x.ptr(), x.ld, at(qd), y.ptr(), y.ld, len(XS), C, stream())
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):
        want = (xv * q[None, :]).astype(F16)
    assert not np.isnan(want).any()
    assert _same_bits(y.get(), want) and y.around_intact() and x.around_intact() and tail_intact(qd, C)


@pytest.mark.parametrize("C,pixels", [(8, 63), (24, 5), (512, 3)])
def test_mul_channel_every_channel_is_multiplied(ops, C, pixels):
    """C / 8 vectors per pixel, C no power of two included: the last 8 channels are not dropped"""
    xv = S.mild((pixels, C), 3.0, 61)
    q = (S.mild((C,), 0.3, 62).astype(np.float32) + 1).astype(F16)
    x = Rows(xv, C, C + 8)
    y = Rows(None, C, C + 24, fill=(pixels, 7.0))
    qd = torch.from_numpy(q.view(np.int16)).cuda()
    call(ops.mul_channel, x.ptr(), x.ld, at(qd), y.ptr(), y.ld, pixels, C, stream())
    torch.cuda.synchronize()
    assert _same_bits(y.get(), (xv * q[None, :]).astype(F16)) and y.around_intact()


# ------------------------------------------------------------------------------------------------------------ round_z / int8_to_half
def test_round_z_every_pattern(ops):
    pat = S.non_nan_patterns().view(F16)
    n = pat.size
    z = torch.from_numpy(pat.view(np.int16).copy()).cuda()
    zh, zi = guarded(n, torch.int16), guarded(n, torch.int8)
    call(ops.round_z, at(z), at(zh), at(zi), n, stream())
    torch.cuda.synchronize()
    wh, wi = orc.round_z(pat)
    assert wi.min() == -64 and wi.max() == 63
    assert np.array_equal(zh[:n].cpu().numpy().view(F16), wh) and not np.isnan(wh).any()
    assert np.array_equal(zi[:n].cpu().numpy(), wi)
    assert tail_intact(zh, n) and tail_intact(zi, n)


def test_int8_to_half_every_value(ops):
    n = 3 * 256 + 5
    v = (np.arange(n) % 256 - 128).astype(np.int8)
    src = torch.from_numpy(v).cuda()
    out = guarded(n, torch.int16)
    call(ops.int8_to_half, at(src), at(out), n, stream())
    torch.cuda.synchronize()
    assert set(v.tolist()) == set(range(-128, 128))
    assert _same_bits(out[:n].cpu().numpy().view(F16), v.astype(F16)) and tail_intact(out, n)
