"""The case builders of tests/symbol_cases.py reach what they claim: proved on the CPU from oracle/symbols_np.py alone, so that
a case that misses its edge fails here and never reaches the MI355X (tests/test_symbols_edges_gpu.py runs them there)."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symbol_cases as S  # noqa: E402
from oracle import symbols_np as orc  # noqa: E402

F16 = np.float16


@pytest.fixture(scope="module")
def scale_sweep():
    return S.scale_sweep()


@pytest.fixture(scope="module")
def quant_sweep():
    return S.quant_sweep()


def test_scale_sweep_holds_every_pattern_for_every_step(scale_sweep):
    c = scale_sweep
    H, W, C = c["H"], c["W"], c["C"]
    every = np.arange(65536)
    for masks in (orc.get_mask_4x(H, W, C), orc.get_mask_2x(H, W, C)):
        for mk in masks:
            seen = np.unique(S.bits(c["scales"][mk]))
            assert np.array_equal(seen, every)


def test_scale_sweep_reaches_every_index_and_every_special_value(scale_sweep):
    p = scale_sweep["patterns"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # the oracle's table is defined on the whole domain
        idx = orc.scale_to_index(p)
    assert idx.min() == 0 and idx.max() == 127 and np.unique(idx).size == 128
    b = S.bits(p)
    assert np.isnan(p).any() and (b == 0x7c00).any() and (b == 0xfc00).any()
    assert (b == 0x0000).any() and (b == 0x8000).any()
    assert ((b & 0x7c00) == 0).sum() == 2 * 1024              # zeros and subnormals of both signs
    assert (p < 0).any()
    # the index of every special value is the first entry or the last
    assert set(idx[np.isnan(p) | (p <= 0)]) == {0} and idx[b == 0x7c00][0] == 127


@pytest.mark.parametrize("thres", S.THRESHOLDS)
def test_scale_sweep_has_both_sides_of_the_threshold(scale_sweep, thres):
    p = scale_sweep["patterns"]
    t = F16(np.float32(thres))
    tb = S.bit(t)
    below = S.from_bits(tb - 1) if tb else S.from_bits(0x8001)      # the neighbour of +0 below it
    above = S.from_bits(tb + 1)
    assert below < t < above
    _, keep = orc.build_index_dec(p, thres)
    b = S.bits(p)
    for v, want in ((below, False), (t, False), (above, True)):
        at = np.flatnonzero(b == S.bit(v))
        assert at.size == 1 and bool(keep[at[0]]) == want


def test_quant_sweep_holds_every_pattern_against_every_mean(quant_sweep):
    c = quant_sweep
    H, W, C = c["H"], c["W"], c["C"]
    pat = S.non_nan_patterns()
    assert pat.size == 63490
    for a in ("y", "means", "q_dec", "scales"):
        assert not np.isnan(c[a]).any(), a
    mk = orc.get_mask_4x(H, W, C)
    for k in range(4):
        y, m = c["y"][mk[k]], c["means"][mk[k]]
        for mean in S.QUANT_MEANS:
            sel = S.bits(m) == S.bit(mean)
            assert np.array_equal(np.unique(S.bits(y[sel])), np.sort(pat)), (k, mean)
    assert F16(6e-8) != 0 and (S.bit(6e-8) & 0x7c00) == 0          # a subnormal mean
    q = c["q_dec"]
    assert (q < 0.5).sum() >= 100 and (q == F16(65504)).sum() >= 1
    assert np.unique(orc.scale_to_index(c["scales"])).size == 128


@pytest.mark.parametrize("thres", S.THRESHOLDS)
def test_quant_sweep_reaches_the_clamp_the_ties_and_the_overflow(quant_sweep, thres):
    c = quant_sweep
    H, W, C = c["H"], c["W"], c["C"]
    masks = orc.get_mask_4x(H, W, C)
    for k in (0, 3):
        with np.errstate(all="ignore"):
            y_q, y_hat, s_hat = orc.process_with_mask(c["y"], c["scales"], c["means"], masks[k], thres)
            comb, keep = orc.build_index_enc(orc.fold4(y_q), orc.fold4(s_hat), thres)
            y_res = (c["y"] - c["means"]).astype(F16)[masks[k]]
        sym = comb.astype(np.int32) >> 8
        assert (sym[keep] == 127).sum() >= 1000 and (sym[keep] == -128).sum() >= 1000
        yk = c["y"][masks[k]]
        assert np.isposinf(yk).any() and np.isneginf(yk).any()
        finite = np.isfinite(y_res)
        frac = np.abs(np.where(finite, y_res, 0).astype(np.float64)) % 1.0
        assert ((frac == 0.5) & finite & (y_res > 0)).sum() >= 100
        assert ((frac == 0.5) & finite & (y_res < 0)).sum() >= 100
        assert (np.isinf(y_res) & np.isfinite(yk)).sum() >= 1                   # y - mean overflows fp16
        assert not np.isnan(y_hat).any() and not np.isnan(y_res).any()


def test_quant_picture_reaches_both_clamps():
    for H, W, C in ((5, 3, 128), (17, 30, 128)):
        p = S.quant_picture(H, W, C)
        st = S.y_steps(p["y"], [p["scales"]] * 4, [p["means"]] * 4, 0.0)
        sym = st[0]["sym"].astype(np.int32) >> 8
        assert (sym == 127).any() and (sym == -128).any()
        assert not np.isnan(st[3]["acc"]).any()


def test_geometry_list_counts_and_blocks():
    from dcvc_amd import _lib
    blocks = _lib.fn("dcvc_symbol_blocks", ctypes.c_int, [ctypes.c_int])
    counts = {}
    for H, W, C, _ in S.GEOMETRIES:
        n = S.geometry_count(H, W, C)
        assert n == H * W * C // 4 and C % 32 == 0 and n % 8 == 0
        assert S.symbol_blocks(n) == (n + 2047) // 2048 == blocks(n)
        counts[(H, W, C)] = n
    assert 2048 in counts.values() and 2048 - 8 in counts.values() and 2048 + 8 in counts.values()
    assert 257 * 2048 + 8 in counts.values() and S.symbol_blocks(257 * 2048 + 8) == 258      # 257 earlier blocks: two passes of 256
    assert {(5, 3), (17, 30), (96, 96)} <= {g[:2] for g in counts}
    assert {32, 128, 256} == {g[2] for g in counts}
    assert max(H * W * C for H, W, C in counts) <= 96 * 96 * 256


@pytest.mark.parametrize("H,W", [(5, 3), (17, 30)])
def test_stacked_pictures_are_not_a_batch(H, W):
    """At an odd height the second picture of a stack starts on an odd row: its masks, and with them its symbols, differ from
    those of the picture on its own. A batched kernel that indexed the batch as one tall picture would show here."""
    C = 128
    pics = [{"y": S.mild((H, W, C), 6.0, 300 + b), "scales": S.mild_scales((H, W, C), 310 + b), "means": S.mild((H, W, C), 2.0, 320 + b)}
            for b in range(2)]
    own = [S.y_steps(p["y"], [p["scales"]] * 4, [p["means"]] * 4, 0.15) for p in pics]
    cat = {a: np.concatenate([p[a] for p in pics]) for a in ("y", "scales", "means")}
    tall = S.y_steps(cat["y"], [cat["scales"]] * 4, [cat["means"]] * 4, 0.15)
    n = S.geometry_count(H, W, C)
    assert np.array_equal(tall[0]["sym"][:n], own[0][0]["sym"])
    assert not np.array_equal(tall[0]["sym"][n:], own[1][0]["sym"])
