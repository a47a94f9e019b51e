"""The tool's rate control (csrc/codec/rate_control.cpp through include/dcvc_amd_rc.h) against dcvc_amd/rate_control.py:
the same q_index for the same history, the same probes for the same size curve; and the refusals of
dcvc encode --target-bpp, which run before the tool loads a model or touches the device."""
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
        create=_lib.fn("dcvc_rc_create", _vp, [_cd, _cd, _cd, _ci, _ci, _ci, _ci, _cd]),
        destroy=_lib.fn("dcvc_rc_destroy", None, [_vp]),
        next_qp=_lib.fn("dcvc_rc_next_qp", _ci, [_vp, _ci]),
        update=_lib.fn("dcvc_rc_update", _ci, [_vp, _cd, _ci, _ci]),
        state=_lib.fn("dcvc_rc_state_qp", _cd, [_vp]),
        pick=_lib.fn("dcvc_rc_pick_qp_for_budget", _ci, [_ESTIMATE, _vp, _i64, _ci, _ci, ctypes.POINTER(_ci)]),
        budget=_lib.fn("dcvc_rc_intra_budget_bits", _i64, [_cd, _cd, _ci, _i64]),
    )


class Native:
    """dcvc_rc behind the interface of rate_control.TargetBpp"""

    def __init__(self, target_bpp, pixels, qp0=32, horizon=8, intra_bonus=0, qp_min=0, qp_max=63, slope=0.049):
        self.f = _fn()
        self.h = self.f["create"](target_bpp, pixels, qp0, horizon, intra_bonus, qp_min, qp_max, slope)
        assert self.h

    def __del__(self):
        if getattr(self, "h", None):
            self.f["destroy"](self.h)

    def next_qp(self, is_intra):
        return _lib.check(self.f["next_qp"](self.h, 1 if is_intra else 0))

    def update(self, bits, pictures, is_intra):
        _lib.check(self.f["update"](self.h, float(bits), int(pictures), 1 if is_intra else 0))

    @property
    def qp(self):
        return self.f["state"](self.h)


def _drive(trace, **kw):
    """the q_index in front of every unit of `trace` = [(bits, pictures, is_intra)], from both controllers"""
    py, nat = rc.TargetBpp(**kw), Native(kw.pop("target_bpp"), kw.pop("pixels_per_picture"), **kw)
    got_py, got_nat = [], []
    for bits, pictures, intra in trace:
        got_py.append(py.next_qp(intra))
        got_nat.append(nat.next_qp(intra))
        py.update(bits, pictures, intra)
        nat.update(bits, pictures, intra)
        assert nat.qp == py.qp, (len(got_py), nat.qp, py.qp)        # the fractional state too, bit for bit
    return got_py, got_nat


def _closed_loop(ctl_kw, frames, delay, intra_period, seed):
    """a trace recorded from the Python controller on a stand-in codec whose bits follow log2 bits ~ q_index"""
    pixels = ctl_kw["pixels_per_picture"]
    rng = np.random.default_rng(seed)

    def size(qp, n, intra):
        return int(n * (0.45 if intra else 0.02) * pixels * 2.0 ** (0.05 * qp) * 2.0 ** rng.normal(0.0, 0.08)) // 8

    units = rc.code_sequence(frames, delay, lambda i, q: b"\0" * size(q, 1, True), lambda i, n, q, r: b"\0" * size(q, n, False),
                             rc.TargetBpp(**ctl_kw), intra_period=intra_period)
    trace, idx = [], 0
    for intra, qp, reset, payload in units:
        n = 1 if intra else min(delay, frames - idx)
        trace.append((8 * len(payload), n, intra))
        idx += 1 if intra else delay
    return trace, [u[1] for u in units]


@pytest.mark.parametrize("target,delay,intra_period,bonus", [
    (0.03, 8, -1, 0), (0.06, 1, 32, 0), (0.12, 1, 32, 4), (0.06, 8, 32, -3), (0.02, 1, -1, 2),
])
def test_native_controller_follows_recorded_traces(target, delay, intra_period, bonus):
    """closed-loop traces, the intra-period-32 case among them (where the Python class once saw-toothed: the update
    behind an I picture projects the last P unit to the q_index the controller stands at)"""
    kw = dict(target_bpp=target, pixels_per_picture=1920 * 1080, qp0=30, horizon=8, intra_bonus=bonus)
    trace, recorded = _closed_loop(dict(kw), 200, delay, intra_period, seed=int(target * 1000))
    got_py, got_nat = _drive(trace, **kw)
    assert got_py == recorded
    assert got_nat == got_py
    assert len(set(got_py)) > 1


@pytest.mark.parametrize("seed", range(6))
def test_native_controller_follows_random_traces(seed):
    rng = np.random.default_rng(seed)
    pixels = int(rng.integers(64 * 64, 3840 * 2160))
    trace = []
    for _ in range(300):
        intra = bool(rng.random() < 0.1)
        pictures = int(rng.integers(0, 9)) if rng.random() < 0.9 else 0          # a unit of 0 pictures is ignored
        bits = int(2.0 ** rng.uniform(0, 26)) if rng.random() < 0.95 else 0
        trace.append((bits, pictures, intra))
    kw = dict(target_bpp=float(2.0 ** rng.uniform(-7, 0)), pixels_per_picture=pixels, qp0=float(rng.integers(0, 64)),
              horizon=int(rng.integers(1, 17)), intra_bonus=int(rng.integers(-4, 9)), qp_min=int(rng.integers(0, 20)),
              qp_max=int(rng.integers(40, 64)), slope=float(rng.uniform(0.02, 0.1)))
    got_py, got_nat = _drive(trace, **kw)
    assert got_nat == got_py


def test_native_controller_clamp_ends():
    pixels = 1280 * 720
    starved = [(10 ** 9, 1, False)] * 40                    # every unit far over budget: down to qp_min and no further
    got_py, got_nat = _drive(starved, target_bpp=0.01, pixels_per_picture=pixels, qp0=32, qp_min=5, qp_max=50)
    assert got_nat == got_py and got_nat[-1] == 5
    idle = [(8, 1, False)] * 40                             # nothing spent: up to qp_max
    got_py, got_nat = _drive(idle, target_bpp=0.5, pixels_per_picture=pixels, qp0=32, qp_min=5, qp_max=50)
    assert got_nat == got_py and got_nat[-1] == 50
    # round half to even, and the intra bonus clamped with the rest
    got_py, got_nat = _drive([(8, 1, True)], target_bpp=0.5, pixels_per_picture=pixels, qp0=30.5, intra_bonus=60)
    assert got_nat == got_py == [63]
    for qp0 in (30.5, 31.5, 0.5, 62.5):
        got_py, got_nat = _drive([(8, 1, False)], target_bpp=0.5, pixels_per_picture=pixels, qp0=qp0)
        assert got_nat == got_py == [int(round(qp0))]
    assert _fn()["create"](0.0, 100.0, 32, 8, 0, 0, 63, 0.049) is None
    assert _fn()["create"](0.1, 0.0, 32, 8, 0, 0, 63, 0.049) is None


# ---------------------------------------------------------------- pick_qp_for_budget
def _native_pick(curve, budget, qp_min, qp_max):
    probed = []

    def estimate(qp, user):
        probed.append(qp)
        return int(curve(qp))

    n = _ci(-1)
    qp = _lib.check(_fn()["pick"](_ESTIMATE(estimate), None, int(budget), qp_min, qp_max, ctypes.byref(n)))
    assert n.value == len(probed)
    return qp, probed


def _python_pick(curve, budget, qp_min, qp_max):
    trace = []
    qp = rc.pick_qp_for_budget(curve, budget, qp_min, qp_max, trace=trace)
    return qp, [t[0] for t in trace]


def _cap(qp_min, qp_max):
    return math.ceil(math.log2(qp_max - qp_min + 2))


@pytest.mark.parametrize("qp_min,qp_max", [(0, 63), (0, 0), (10, 11), (5, 40), (63, 63), (17, 48)])
def test_pick_qp_monotone_curves(qp_min, qp_max):
    curve = lambda q: int(1000 * 2.0 ** (0.05 * q))          # noqa: E731
    sizes = [curve(q) for q in range(64)]
    for budget in sorted({0, sizes[0] - 1, sizes[63] + 1, 10 ** 9} | set(sizes) | {s - 1 for s in sizes}):
        qp_n, probes_n = _native_pick(curve, budget, qp_min, qp_max)
        qp_p, probes_p = _python_pick(curve, budget, qp_min, qp_max)
        assert (qp_n, probes_n) == (qp_p, probes_p)
        assert 1 <= len(probes_n) <= _cap(qp_min, qp_max)
        fitting = [q for q in range(qp_min, qp_max + 1) if sizes[q] <= budget]
        assert qp_n == (max(fitting) if fitting else qp_min)   # the largest q_index that fits, qp_min when nothing does
    assert _cap(0, 63) == 7


@pytest.mark.parametrize("seed", range(8))
def test_pick_qp_non_monotone_curves(seed):
    rng = np.random.default_rng(seed)
    sizes = (1000 * 2.0 ** (0.05 * np.arange(64)) * 2.0 ** rng.normal(0, 0.3, 64)).astype(np.int64)
    curve = lambda q: int(sizes[q])                          # noqa: E731
    for budget in rng.integers(int(sizes.min()) - 10, int(sizes.max()) + 10, 40):
        for qp_min, qp_max in ((0, 63), (7, 29)):
            qp_n, probes_n = _native_pick(curve, int(budget), qp_min, qp_max)
            qp_p, probes_p = _python_pick(curve, int(budget), qp_min, qp_max)
            assert (qp_n, probes_n) == (qp_p, probes_p)
            assert len(probes_n) <= _cap(qp_min, qp_max) and len(set(probes_n)) == len(probes_n)
            # deterministic, and it ends with "the answer fits, the one above was probed and does not"
            if qp_n in probes_n and sizes[qp_n] <= budget:
                assert qp_n == qp_max or (qp_n + 1 in probes_n and sizes[qp_n + 1] > budget)
            else:
                assert qp_n == qp_min and sizes[qp_min] > budget


def test_pick_qp_failures():
    assert _fn()["pick"](_ESTIMATE(lambda q, u: -1), None, 100, 0, 63, None) < 0      # a failing probe is passed on
    assert _fn()["pick"](_ESTIMATE(lambda q, u: 1), None, 100, 9, 8, None) < 0
    with pytest.raises(ValueError):
        rc.pick_qp_for_budget(lambda q: 1, 100, 9, 8)


def test_intra_budget_native_equals_python():
    rng = np.random.default_rng(2)
    f = _fn()["budget"]
    for _ in range(500):
        bpp, pixels = float(2.0 ** rng.uniform(-8, 1)), int(rng.integers(256, 3840 * 2160))
        k, spent = int(rng.integers(0, 1000)), int(rng.integers(0, 1 << 36))
        assert f(bpp, pixels, k, spent) == rc.intra_budget_bits(bpp, pixels, k, spent)
    assert rc.intra_budget_bits(0.5, 1000, 0, 0) == 500
    assert rc.intra_budget_bits(0.5, 1000, 3, 10 ** 6) == 125          # overspent: a quarter of one picture's share


# ---------------------------------------------------------------- the tool's refusals
def _run(args):
    if not os.path.exists(TOOL):
        pytest.skip("dcvc_amd/bin/dcvc is not built on this machine")
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode_args(tmp_path, *extra):
    return ["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.yuv"), "-W", "64", "-H", "64",
            "-o", str(tmp_path / "o.bin")] + list(extra)


@pytest.mark.parametrize("value", ["0", "-0.1", "nan", "inf", "abc", "0.1x", ""])
def test_target_bpp_must_be_positive(tmp_path, value):
    r = _run(_encode_args(tmp_path, "--target-bpp", value))
    assert r.returncode == 2 and "--target-bpp must be a positive number" in r.stderr, r.stderr


def test_target_bpp_with_a_batch_is_refused(tmp_path):
    r = _run(_encode_args(tmp_path, "--target-bpp", "0.1", "--batch", "4"))
    assert r.returncode == 2 and "--batch" in r.stderr and "one q_index" in r.stderr, r.stderr


def test_target_bpp_with_qp_p_is_refused(tmp_path):
    r = _run(_encode_args(tmp_path, "--target-bpp", "0.1", "--inter", str(tmp_path / "p.dcvw"), "--qp-p", "30"))
    assert r.returncode == 2 and "--qp-p" in r.stderr, r.stderr


def test_qp_min_above_qp_max_is_refused(tmp_path):
    r = _run(_encode_args(tmp_path, "--target-bpp", "0.1", "--qp-min", "40", "--qp-max", "20"))
    assert r.returncode == 2 and "--qp-min 40 is above --qp-max 20" in r.stderr, r.stderr
    r = _run(_encode_args(tmp_path, "--target-bpp", "0.1", "--qp-max", "64"))
    assert r.returncode == 2 and "--qp-max must be in 0..63" in r.stderr, r.stderr


def test_rate_options_need_a_target(tmp_path):
    r = _run(_encode_args(tmp_path, "--qp-min", "10"))
    assert r.returncode == 2 and "--qp-min needs --target-bpp" in r.stderr, r.stderr
