"""The search and the budget of dcvc encode --rc-mode probe, on the CPU: rate_control.pick_qp_near,
unit_budget_bits and code_sequence_probed against their native restatements (csrc/codec/rate_control.cpp through
include/dcvc_amd_rc.h) probe for probe, the probe counts and the end condition on every step curve, the probed loop on a
synthetic size model, and the tool's refusals, which come before it loads a model or touches the device."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from dcvc_amd import _lib, rate_control as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")

_vp, _ci, _cd, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64
_ESTIMATE = ctypes.CFUNCTYPE(_i64, _ci, _vp)


def _fn():
    return dict(
        near=_lib.fn("dcvc_rc_pick_qp_near", _ci, [_ESTIMATE, _vp, _i64, _ci, _ci, _ci, ctypes.POINTER(_ci)]),
        budget=_lib.fn("dcvc_rc_unit_budget_bits", _i64, [_cd, _cd, _ci, _i64, _ci, _ci]),
    )


_F = None


def _native_near(curve, budget, start, qp_min, qp_max):
    global _F
    _F = _F or _fn()
    probed = []

    def estimate(qp, user):
        probed.append(qp)
        return int(curve(qp))

    n = _ci(-1)
    qp = _lib.check(_F["near"](_ESTIMATE(estimate), None, int(budget), start, qp_min, qp_max, ctypes.byref(n)))
    assert n.value == len(probed)
    return qp, probed


def _python_near(curve, budget, start, qp_min, qp_max):
    trace = []
    qp = rc.pick_qp_near(curve, budget, start, qp_min, qp_max, trace=trace)
    return qp, [t[0] for t in trace]


def _cap(qp_min, qp_max):
    return 2 * math.ceil(math.log2(qp_max - qp_min + 2)) + 1


def _check_end(qp, probes, fits, qp_min, qp_max):
    """lo fits or is qp_min - 1; lo + 1 was probed and does not fit, or is qp_max + 1; the answer is lo, or qp_min"""
    assert len(set(probes)) == len(probes), probes                     # no q_index twice
    assert all(qp_min <= q <= qp_max for q in probes)
    if qp in probes and fits(qp):
        lo = qp
    else:
        lo = qp_min - 1
        assert qp == qp_min and qp_min in probes and not fits(qp_min)
    assert lo == qp_max or (lo + 1 in probes and not fits(lo + 1)), (qp, probes)


@pytest.mark.parametrize("qp_min,qp_max", [(0, 63), (20, 29), (5, 5), (0, 1), (17, 48)])
def test_every_step_curve_and_start(qp_min, qp_max):
    worst, worst_at_start, worst_near = 0, 0, 0
    for threshold in range(0, 65):                                     # q fits iff q < threshold
        curve = lambda q: 0 if q < threshold else 1                    # noqa: E731
        fits = lambda q: q < threshold                                 # noqa: E731
        want = rc.pick_qp_for_budget(curve, 0, qp_min, qp_max)
        for start in range(0, 64):
            qp_n, probes_n = _native_near(curve, 0, start, qp_min, qp_max)
            qp_p, probes_p = _python_near(curve, 0, start, qp_min, qp_max)
            assert (qp_n, probes_n) == (qp_p, probes_p), (threshold, start)
            assert qp_p == want, (threshold, start)                    # monotone: the bisection's answer
            assert probes_p[0] == min(qp_max, max(qp_min, start))
            _check_end(qp_p, probes_p, fits, qp_min, qp_max)
            worst = max(worst, len(probes_p))
            if qp_min <= start <= qp_max and qp_p == start:
                worst_at_start = max(worst_at_start, len(probes_p))
            if qp_min <= start <= qp_max and abs(qp_p - start) <= 2:
                worst_near = max(worst_near, len(probes_p))
    print("range %d..%d: worst %d probes, %d when the answer is start, %d within 2 of it (cap %d)"
          % (qp_min, qp_max, worst, worst_at_start, worst_near, _cap(qp_min, qp_max)))
    assert worst <= _cap(qp_min, qp_max)
    assert worst_at_start <= 2 and worst_near <= 4
    if (qp_min, qp_max) == (0, 63):
        assert worst == 12 and _cap(0, 63) == 15


@pytest.mark.parametrize("seed", range(10))
def test_non_monotone_curves(seed):
    """30 curves x 4 ranges per seed: a noisy size curve has no "largest q_index that fits", but the search is the same
    in both languages, ends with the same condition, within the same cap"""
    rng = np.random.default_rng(seed)
    for _ in range(30):
        sizes = (1000 * 2.0 ** (0.05 * np.arange(64)) * 2.0 ** rng.normal(0, 0.3, 64)).astype(np.int64)
        curve = lambda q: int(sizes[q])                                # noqa: E731
        budget = int(rng.integers(int(sizes.min()) - 10, int(sizes.max()) + 10))
        for qp_min, qp_max in ((0, 63), (7, 29), (20, 29), (0, 1)):
            start = int(rng.integers(0, 64))
            qp_n, probes_n = _native_near(curve, budget, start, qp_min, qp_max)
            qp_p, probes_p = _python_near(curve, budget, start, qp_min, qp_max)
            assert (qp_n, probes_n) == (qp_p, probes_p)
            assert len(probes_p) <= _cap(qp_min, qp_max)
            _check_end(qp_p, probes_p, lambda q: sizes[q] <= budget, qp_min, qp_max)


def test_exponential_curve_equals_the_bisection():
    curve = lambda q: int(1000 * 2.0 ** (0.049 * q))                    # noqa: E731
    sizes = [curve(q) for q in range(64)]
    for budget in sorted({0, sizes[0] - 1, sizes[63] + 1, 10 ** 9} | set(sizes) | {s - 1 for s in sizes}):
        want = rc.pick_qp_for_budget(curve, budget, 0, 63)
        for start in (0, 5, 31, 32, 62, 63, -4, 90):                    # a start outside the range is clamped
            qp_n, probes_n = _native_near(curve, budget, start, 0, 63)
            assert (qp_n, probes_n) == _python_near(curve, budget, start, 0, 63)
            assert qp_n == want


def test_search_failures():
    f = _fn()["near"]
    assert f(_ESTIMATE(lambda q, u: -1), None, 100, 30, 0, 63, None) < 0      # a failing probe is passed on
    assert f(_ESTIMATE(lambda q, u: 1), None, 100, 8, 9, 8, None) < 0
    with pytest.raises(ValueError):
        rc.pick_qp_near(lambda q: 1, 100, 8, 9, 8)


# ---------------------------------------------------------------- the unit budget
def test_unit_budget_native_equals_python():
    rng = np.random.default_rng(5)
    f = _fn()["budget"]
    floored = 0
    for _ in range(2000):
        bpp, pixels = float(2.0 ** rng.uniform(-8, 1)), int(rng.integers(256, 3840 * 2160))
        coded, horizon, n = int(rng.integers(0, 2000)), int(rng.integers(1, 33)), int(rng.integers(0, 9))
        spent = int(bpp * pixels * coded * 2.0 ** rng.uniform(-1, 1))
        got = f(bpp, pixels, coded, spent, horizon, n)
        assert got == rc.unit_budget_bits(bpp, pixels, coded, spent, horizon, n)
        share = bpp * pixels
        floored += (share * (coded + horizon) - spent) / horizon < share / 64.0
    assert 100 < floored < 1900                                         # both sides of the floor were exercised
    # on target: one picture's share; the quantity TargetBpp.update computes
    assert rc.unit_budget_bits(0.5, 1000, 10, 5000, 8, 1) == 500
    assert rc.unit_budget_bits(0.5, 1000, 10, 5000, 8, 8) == 4000
    assert rc.unit_budget_bits(0.5, 1000, 10, 5400, 8, 1) == 450        # 400 bits over, paid back over 8 pictures
    assert rc.unit_budget_bits(0.5, 1000, 3, 10 ** 6, 8, 8) == 62       # far over: floor(500 / 64 * 8)
    assert f(0.5, 1000.0, 3, 10 ** 6, 8, 8) == 62
    assert f(0.5, 1000.0, 3, 0, 0, 8) < 0
    with pytest.raises(ValueError):
        rc.unit_budget_bits(0.5, 1000, 3, 0, 0, 8)
    ctl = rc.TargetBpp(0.5, 1000, horizon=8)
    ctl.update(5400, 10, False)
    assert rc.unit_budget_bits(0.5, 1000, ctl.pictures, int(ctl.spent), 8, 1) == int(
        max((ctl.target_bits * (ctl.pictures + 8) - ctl.spent) / 8, ctl.target_bits / 64.0))


# ---------------------------------------------------------------- the probed loop
class _Clip:
    """stand-in codec: a picture at q_index q takes complexity * a * 2^(0.049 q) bits; the probe predicts the bits of the
    unit, the coder then writes that many bytes rounded up (the prediction is in bytes too)"""

    def __init__(self, frames, pixels, intra_cost=0.15, inter_cost=0.02, jump_at=None):
        self.frames, self.pixels, self.intra_cost, self.inter_cost, self.jump_at = frames, pixels, intra_cost, inter_cost, jump_at
        self.probes = []

    def _complexity(self, idx):
        return 3.0 if self.jump_at is not None and idx >= self.jump_at else 1.0

    def _bytes(self, idx, n, qp, cost):
        bits = sum(self._complexity(idx + j) * cost * self.pixels * 2.0 ** (0.049 * qp) for j in range(n))
        return int(math.ceil(bits / 8))

    def code_intra(self, idx, qp):
        return b"\0" * self._bytes(idx, 1, qp, self.intra_cost)

    def code_inter(self, idx, n, qp, reset):
        return b"\0" * self._bytes(idx, n, qp, self.inter_cost)

    def probe_inter(self, idx, n, qp):
        self.probes.append((idx, qp))
        return 8 * self._bytes(idx, n, qp, self.inter_cost)


@pytest.mark.parametrize("frames,delay,intra_period,reset_interval,jump_at,bonus", [
    (60, 1, -1, 32, None, 0), (60, 1, -1, 4, 30, 3), (100, 8, -1, 32, 50, 0), (77, 8, 32, 32, 40, -2), (40, 1, 16, 8, 20, 0),
])
def test_probed_loop_on_a_synthetic_size_model(frames, delay, intra_period, reset_interval, jump_at, bonus):
    pixels = 1920 * 1080
    clip = _Clip(frames, pixels, jump_at=jump_at)
    target = 0.02 * 2.0 ** (0.049 * 30) * 1.6                          # about what the P pictures take at q 40
    log = []
    units = rc.code_sequence_probed(frames, delay, clip.code_intra, clip.code_inter, clip.probe_inter, target, pixels,
                                    qp_i=30, horizon=8, intra_bonus=bonus, intra_period=intra_period,
                                    reset_interval=reset_interval, log=log)
    # unit types and reset flags: code_sequence's
    plain = rc.code_sequence(frames, delay, clip.code_intra, clip.code_inter, rc.ConstantQP(30), intra_period=intra_period,
                             reset_interval=reset_interval)
    assert [(u[0], u[2]) for u in units] == [(u[0], u[2]) for u in plain]
    assert len(log) == len(units)
    spent, pictures, start, idx, checked, idxs = 0, 0, 30, 0, 0, []
    for (intra, qp, reset, payload), entry in zip(units, log):
        assert entry["type"] == ("I" if intra else "P") and entry["qp"] == qp
        idxs.append(idx)
        if intra:
            assert qp == min(63, max(0, start + bonus))
            assert entry["probes"] == 0 and entry["predicted_bits"] is None
            n = 1
        else:
            n = min(delay, frames - idx)
            budget = rc.unit_budget_bits(target, pixels, pictures, spent, 8, n)
            assert entry["budget_bits"] == budget
            assert 1 <= entry["probes"] == len(entry["trace"]) <= 12
            assert entry["trace"][0][0] == start
            assert entry["predicted_bits"] == 8 * len(payload)          # the stand-in's probe is exact
            if qp > 0:                                                  # the largest q_index whose predicted bits fit
                assert entry["predicted_bits"] <= budget
                checked += 1
            if qp < 63:
                assert 8 * clip._bytes(idx, n, qp + 1, clip.inter_cost) > budget
            start = qp
        spent += 8 * len(payload)
        pictures += n
        idx += 1 if intra else delay
    assert checked > 0.5 * sum(1 for u in units if not u[0])      # (the rest sit at q 0 behind a costly I picture)
    p_qps = [u[1] for u in units if not u[0]]
    assert len(set(p_qps)) > 1
    if jump_at is not None:               # three times the bits at every q_index: log2(3) / 0.049 = 32 steps down
        first = sum(1 for i, u in zip(idxs, units) if not u[0] and i + delay <= jump_at)
        assert np.median(p_qps[:first]) - np.median(p_qps[first:]) >= 15, p_qps
    print("q_index of the P units:", p_qps, "probes:", [e["probes"] for e in log if e["type"] == "P"])


def test_probe_counts_of_a_steady_clip():
    """neighbouring units, neighbouring q_index: 2 to 4 probes per unit once the search has found its level"""
    pixels = 1280 * 720
    clip = _Clip(64, pixels)
    log = []
    rc.code_sequence_probed(64, 1, clip.code_intra, clip.code_inter, clip.probe_inter, 0.05, pixels, qp_i=20, log=log)
    probes = [e["probes"] for e in log if e["type"] == "P"]
    assert max(probes[8:]) <= 4 and sum(probes) < 4 * len(probes)


class _ChunkClip(_Clip):
    """an 8-picture model: a short last chunk is padded and coded as 8 pictures, whatever n says"""

    def _bytes(self, idx, n, qp, cost):
        return _Clip._bytes(self, idx, n if cost == self.intra_cost else 8, qp, cost)


@pytest.mark.parametrize("level,falls_to_qp_min", [(45, False), (20, True)])
def test_a_ragged_last_chunk_is_8_pictures_on_the_budget_of_n(level, falls_to_qp_min):
    """The rule as it stands ("The unit budget"): the last chunk of 3 pictures gets floor(want 3) bits and
    costs what 8 pictures cost, so its q_index lies log2(8 / 3) / 0.049 = 29 steps below its neighbours', and a clip that
    runs below q 29 ends at qp_min with a unit that fits no q_index."""
    pixels, frames = 1280 * 720, 1 + 8 * 4 + 3
    clip = _ChunkClip(frames, pixels)
    target = 0.02 * 2.0 ** (0.049 * level)                             # the P pictures' cost at q = level
    log = []
    units = rc.code_sequence_probed(frames, 8, clip.code_intra, clip.code_inter, clip.probe_inter, target, pixels,
                                    qp_i=level, horizon=16, log=log)
    spent = sum(8 * len(u[3]) for u in units[:-1])
    budget = rc.unit_budget_bits(target, pixels, frames - 3, spent, 16, 3)
    last, before = log[-1], log[-2]
    assert last["budget_bits"] == budget
    curve = lambda q: 8 * clip._bytes(frames - 3, 3, q, clip.inter_cost)       # noqa: E731
    assert curve(5) == 8 * _Clip._bytes(clip, frames - 3, 8, 5, clip.inter_cost)
    assert last["qp"] == rc.pick_qp_for_budget(curve, budget, 0, 63)
    if falls_to_qp_min:
        assert before["qp"] < 29 and last["qp"] == 0 and last["predicted_bits"] > budget, (before["qp"], last["qp"])
    else:                                 # 29 steps, give or take what `want` moved between the two units
        assert 25 <= before["qp"] - last["qp"] <= 33, (before["qp"], last["qp"])
        assert 0 < last["qp"] and last["predicted_bits"] <= budget < curve(last["qp"] + 1)


# ---------------------------------------------------------------- the tool's refusals
def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is not built: the build puts it there"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode_args(tmp_path, *extra):
    return ["encode", "--intra", str(tmp_path / "missing.dcvw"), "--inter", str(tmp_path / "missing_p.dcvw"), "-i",
            str(tmp_path / "missing.yuv"), "-W", "64", "-H", "64", "-o", str(tmp_path / "o.bin")] + list(extra)


def test_rc_mode_needs_a_target(tmp_path):
    r = _run(_encode_args(tmp_path, "--rc-mode", "probe"))
    assert r.returncode == 2 and "--rc-mode needs --target-bpp" in r.stderr, r.stderr


@pytest.mark.parametrize("mode", ["search", "", "Probe"])
def test_unknown_rc_mode_is_refused(tmp_path, mode):
    r = _run(_encode_args(tmp_path, "--target-bpp", "0.1", "--rc-mode", mode))
    assert r.returncode == 2 and "--rc-mode must be feedback or probe" in r.stderr, r.stderr
