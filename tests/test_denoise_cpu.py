"""The denoising prefilter of DESIGN.md 26 without a GPU: the properties of its numpy restatement (tests/denoise_np.py), the
denoising claim on a noisy synthetic clip, and what dcvc encode --denoise / --denoise-out refuse before a model is loaded."""
import os
import subprocess

import numpy as np
import pytest

import denoise_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")

KINDS = [(8, np.uint8), (10, np.uint16), (16, np.uint16)]


def _random(bits, dtype, shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << bits, shape).astype(dtype)


# ------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("bits,dtype", KINDS)
def test_zero_strengths_are_the_identity(bits, dtype):
    a, p = _random(bits, dtype, (37, 53), 1), _random(bits, dtype, (37, 53), 2)
    for prev in (None, p):
        got = denoise_np.denoise_plane(a, prev, 0, 0, bits)
        assert got.dtype == dtype and np.array_equal(got, a)


@pytest.mark.parametrize("bits,dtype", KINDS)
@pytest.mark.parametrize("level", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("strengths", [(8, 8), (64, 64), (1, 0), (0, 1)])
def test_a_constant_plane_stays_constant(bits, dtype, level, strengths):
    v = int(level * ((1 << bits) - 1))
    a = np.full((9, 14), v, dtype)
    for prev in (None, a):
        assert (denoise_np.denoise_plane(a, prev, strengths[0], strengths[1], bits) == v).all()


def _window_min_max(a, radius):
    p = np.pad(a.astype(np.int64), radius, mode="edge")
    H, W = a.shape
    views = [p[dy:dy + H, dx:dx + W] for dy in range(2 * radius + 1) for dx in range(2 * radius + 1)]
    return np.minimum.reduce(views), np.maximum.reduce(views)


@pytest.mark.parametrize("bits,dtype", KINDS)
@pytest.mark.parametrize("strengths", [(8, 0), (64, 0), (0, 8), (8, 8), (64, 64), (3, 64)])
@pytest.mark.parametrize("pattern", ["random", "checkerboard", "near"])
def test_outputs_lie_between_the_samples_they_read(bits, dtype, strengths, pattern):
    m = (1 << bits) - 1
    if pattern == "random":
        a, p = _random(bits, dtype, (21, 34), 3), _random(bits, dtype, (21, 34), 4)
    elif pattern == "checkerboard":
        yy, xx = np.mgrid[0:21, 0:34]
        a = (((yy + xx) & 1) * m).astype(dtype)
        p = (m - a).astype(dtype)
    else:       # samples within the thresholds of each other, so that every weight is positive
        rng = np.random.default_rng(5)
        a = (m // 2 + rng.integers(-3, 4, (21, 34)) * (1 << (bits - 8))).astype(dtype)
        p = (m // 2 + rng.integers(-3, 4, (21, 34)) * (1 << (bits - 8))).astype(dtype)
    S, T = strengths
    # the spatial stage reads the 3x3 neighbourhood
    sp = denoise_np.spatial_stage(a, S, bits)
    lo, hi = _window_min_max(a, 1)
    assert (sp >= lo).all() and (sp <= hi).all()
    # the temporal stage reads sp and prev over 3x3, and gives a value between sp and prev at the centre
    out = denoise_np.denoise_plane(a, p, S, T, bits).astype(np.int64)
    lo, hi = np.minimum(sp, p.astype(np.int64)), np.maximum(sp, p.astype(np.int64))
    assert (out >= lo).all() and (out <= hi).all()
    lo5, hi5 = _window_min_max(a, 2)
    plo, phi = _window_min_max(p, 1)
    assert (out >= np.minimum(lo5, plo)).all() and (out <= np.maximum(hi5, phi)).all()


@pytest.mark.parametrize("bits,dtype", KINDS)
def test_no_history_is_temporal_zero(bits, dtype):
    a = _random(bits, dtype, (19, 23), 6)
    assert np.array_equal(denoise_np.denoise_plane(a, None, 8, 8, bits), denoise_np.denoise_plane(a, None, 8, 0, bits))
    assert np.array_equal(denoise_np.denoise_plane(a, None, 8, 8, bits), denoise_np.denoise_plane(a, a, 8, 0, bits))


def test_the_floor_is_a_true_floor():
    # num is negative wherever the neighbours lie below the centre: the quotient is checked against exact fractions
    from fractions import Fraction
    import math
    rng = np.random.default_rng(7)
    a = (120 + rng.integers(-6, 7, (12, 12))).astype(np.uint8)
    sp = denoise_np.spatial_stage(a, 8, 8)
    p = np.pad(a.astype(int), 1, mode="edge")
    for y in range(12):
        for x in range(12):
            c = int(a[y, x])
            n = [int(p[y + dy, x + dx]) for dy in range(3) for dx in range(3)]
            w = [max(0, 8 - abs(v - c)) for v in n]
            num, ws = sum(wi * (v - c) for wi, v in zip(w, n)), sum(w)
            assert sp[y, x] == c + math.floor(Fraction(2 * num + ws, 2 * ws))


def test_the_accumulator_bound_holds_at_the_largest_strength():
    # the largest term: |n - c| = Ts / 2 in all 8 neighbours, at 16 bits and strength 64
    Ts = 64 << 8
    a = np.full((3, 3), 40000, np.uint16)
    a[1, 1] = 40000 - Ts // 2
    c = a.astype(np.int64)
    d = c - c[1, 1]
    w = np.maximum(0, Ts - np.abs(d))
    assert abs(2 * int((w * d).sum()) + int(w.sum())) < 2 ** 31
    got = denoise_np.spatial_stage(a, 64, 16)[1, 1]
    assert got == c[1, 1] + (2 * int((w * d).sum()) + int(w.sum())) // (2 * int(w.sum()))


# ------------------------------------------------------------------------------------ the denoising claim
def _psnr(a, ref, peak):
    mse = float(((a.astype(np.float64) - ref) ** 2).mean())
    return 10 * np.log10(peak * peak / mse)


@pytest.mark.parametrize("bits", [8, 10])
def test_it_denoises_a_static_scene_and_does_not_hurt_a_pan(bits):
    Hh, Ww = 96, 128
    s = 1 << (bits - 8)
    peak = float((1 << bits) - 1)
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:Hh, 0:Ww + 16]
    wide = (128 + 60 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 40 * ((xx // 16 + yy // 16) & 1)) * s
    shifts = [0, 0, 0, 0, 8, 16]
    clean = [wide[:, d:d + Ww] for d in shifts]
    dtype = np.uint8 if bits == 8 else np.uint16
    noisy = [np.clip(np.rint(c + rng.normal(0, 3 * s, c.shape)), 0, peak).astype(dtype) for c in clean]
    out = denoise_np.denoise_clip([(p,) for p in noisy], 8, 8, bits)
    gain = [_psnr(o[0], c, peak) - _psnr(n, c, peak) for o, n, c in zip(out, noisy, clean)]
    print(bits, [round(g, 2) for g in gain])
    assert gain[3] >= 3.0, gain
    assert gain[4] >= 0.0 and gain[5] >= 0.0, gain


# ------------------------------------------------------------------------------------ the tool
def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.yuv"), "-W", "352", "-H", "288",
                 "-o", str(tmp_path / "o.bin")] + extra)


def _decode(tmp_path, extra):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path / "o.yuv")]
                + extra)


def _refused(r, tmp_path, words):
    assert r.returncode == 2 and words in r.stderr, r.stderr
    assert "missing.dcvw" not in r.stderr, r.stderr          # before a model is loaded
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "o.yuv").exists() and not (tmp_path / "dn.yuv").exists()


@pytest.mark.parametrize("value", ["65", "-1", "8:", "a", "8:65", "", ":8", "8:4:2", "8.5", " 8", "1e1"])
def test_malformed_strengths_are_refused(tmp_path, value):
    _refused(_encode(tmp_path, ["--denoise", value]), tmp_path, "--denoise must be S or S:T with integers in 0..64")


@pytest.mark.parametrize("src_type", ["nv12", "p010", "nv21", "rgb24", "png", "rgb48"])
def test_interleaved_and_rgb_sources_are_refused(tmp_path, src_type):
    _refused(_encode(tmp_path, ["--denoise", "8", "--src-type", src_type]), tmp_path, "sources are not filtered yet")


def test_denoise_out_needs_denoise_and_a_file_name(tmp_path):
    _refused(_encode(tmp_path, ["--denoise-out", str(tmp_path / "dn.yuv")]), tmp_path, "--denoise-out needs --denoise")
    _refused(_encode(tmp_path, ["--denoise", "8", "--denoise-out", "-"]), tmp_path, "--denoise-out needs a file name")


def test_the_flags_are_encoder_flags(tmp_path):
    _refused(_decode(tmp_path, ["--denoise", "8"]), tmp_path, "--denoise is an encoder flag")
    _refused(_decode(tmp_path, ["--denoise-out", str(tmp_path / "dn.yuv")]), tmp_path, "--denoise-out is an encoder flag")


@pytest.mark.parametrize("extra", [["--denoise", "8:4"], ["--denoise", "0"], ["--denoise", "64:0", "--src-type", "yuv444"],
                                   ["--denoise", "8", "--src-type", "v210"], ["--denoise", "8", "--denoise-out", "dn.yuv", "--bit-depth", "10"]])
def test_good_flags_pass_the_flag_checks(tmp_path, extra):
    extra = [str(tmp_path / e) if e == "dn.yuv" else e for e in extra]
    r = _encode(tmp_path, extra)
    assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
    assert not (tmp_path / "dn.yuv").exists()
