"""The search of dcvc encode --target-psnr, on the CPU: rate_control.pick_qp_for_quality against its native
restatement (csrc/codec/rate_control.cpp through include/dcvc_amd_rc.h) trial for trial, the answer, the trial order and the
trial counts on every step curve, agreement on curves that do not rise with the q_index, failures, and the quality loop
code_sequence_quality on a synthetic quality model."""
import ctypes
import math

import numpy as np
import pytest

from dcvc_amd import _lib, rate_control as rc

_vp, _ci, _cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
_MEASURE = ctypes.CFUNCTYPE(_cd, _ci, _vp)

_F = None


def _pick():
    global _F
    _F = _F or _lib.fn("dcvc_rc_pick_qp_for_quality", _ci, [_MEASURE, _vp, _cd, _ci, _ci, _ci, ctypes.POINTER(_ci)])
    return _F


def _native(curve, target, start, qp_min, qp_max):
    tried = []

    def measure(qp, user):
        tried.append(qp)
        return float(curve(qp))

    n = _ci(-1)
    qp = _lib.check(_pick()(_MEASURE(measure), None, float(target), start, qp_min, qp_max, ctypes.byref(n)))
    assert n.value == len(tried)
    return qp, tried


def _python(curve, target, start, qp_min, qp_max):
    trace = []
    qp = rc.pick_qp_for_quality(curve, target, start, qp_min, qp_max, trace=trace)
    assert all(quality == curve(q) for q, quality in trace)
    return qp, [t[0] for t in trace]


def _cap(qp_min, qp_max):
    return 2 * math.ceil(math.log2(qp_max - qp_min + 2)) + 1


def _check_procedure(qp, tried, meets, start, qp_min, qp_max):
    """the issue's procedure, step by step, on the trial sequence"""
    assert len(set(tried)) == len(tried), tried                        # no q_index twice
    assert all(qp_min <= q <= qp_max for q in tried)
    s = min(qp_max, max(qp_min, start))
    assert tried[0] == s
    # the gallop: from s with step 1, 2, 4, ... downward while the values meet, upward while they do not
    at, step, i, down = s, 1, 1, meets(s)
    lo, hi = (qp_min - 1, s) if down else (s, qp_max + 1)              # lo: does not meet (or below the range), hi: meets (or above)
    while (at > qp_min) if down else (at < qp_max):
        q = max(at - step, qp_min) if down else min(at + step, qp_max)
        assert tried[i] == q, (tried, i, q)
        i += 1
        if meets(q) != down:
            if down:
                lo = q
            else:
                hi = q
            break
        at = q
        if down:
            hi = q
        else:
            lo = q
        step *= 2
    # the bisection of the bracket
    while hi - lo > 1:
        mid = qp_min + qp_max - ((qp_min + qp_max - hi) + ((qp_min + qp_max - lo) - (qp_min + qp_max - hi)) // 2)
        assert tried[i] == mid, (tried, i, mid)
        i += 1
        if meets(mid):
            hi = mid
        else:
            lo = mid
    assert i == len(tried)
    assert qp == (hi if hi <= qp_max else qp_max)                      # the smallest bracketed q_index that meets; qp_max if none


@pytest.mark.parametrize("qp_min,qp_max", [(0, 63), (20, 29), (5, 5), (0, 1), (17, 48)])
def test_every_step_curve_and_start(qp_min, qp_max):
    worst, worst_at_start = 0, 0
    for threshold in range(0, 65):                                     # q meets iff q >= threshold
        curve = lambda q: 40.0 if q >= threshold else 30.0             # noqa: E731
        meets = lambda q: q >= threshold                               # noqa: E731
        want = min(qp_max, max(qp_min, threshold))                     # the smallest q_index in range that meets, else qp_max
        for start in range(0, 64):
            qp_n, tried_n = _native(curve, 35.0, start, qp_min, qp_max)
            qp_p, tried_p = _python(curve, 35.0, start, qp_min, qp_max)
            assert (qp_n, tried_n) == (qp_p, tried_p), (threshold, start)
            assert qp_p == want, (threshold, start)
            _check_procedure(qp_p, tried_p, meets, start, qp_min, qp_max)
            if qp_p > qp_min and meets(qp_p):                          # one lower was tried and does not meet
                assert qp_p - 1 in tried_p and not meets(qp_p - 1)
            assert meets(qp_p) or qp_p == qp_max
            worst = max(worst, len(tried_p))
            if qp_min <= start <= qp_max and qp_p == start:
                worst_at_start = max(worst_at_start, len(tried_p))
    print("range %d..%d: worst %d trials, %d when the answer is start (cap %d)" % (qp_min, qp_max, worst, worst_at_start, _cap(qp_min, qp_max)))
    assert worst <= _cap(qp_min, qp_max)
    assert worst_at_start <= 2
    if (qp_min, qp_max) == (0, 63):
        assert worst == 12


def test_the_mirror_image_of_pick_qp_near():
    """trial for trial pick_qp_near's probes under q -> qp_min + qp_max - q"""
    for qp_min, qp_max in ((0, 63), (7, 29)):
        flip = qp_min + qp_max
        for threshold in range(0, 65, 3):
            for start in range(0, 64, 5):
                trace = []
                near = rc.pick_qp_near(lambda r: 0 if flip - r >= threshold else 1, 0, flip - min(qp_max, max(qp_min, start)), qp_min, qp_max,
                                       trace=trace)
                qp, tried = _python(lambda q: 1.0 if q >= threshold else 0.0, 0.5, start, qp_min, qp_max)
                assert qp == flip - near and tried == [flip - t[0] for t in trace]


@pytest.mark.parametrize("seed", range(10))
def test_non_monotone_curves(seed):
    """a noisy quality curve has no "smallest q_index that meets", but the search is the same in both languages, follows the
    procedure and stays within the cap"""
    rng = np.random.default_rng(seed)
    for _ in range(30):
        psnr = 28.0 + 0.2 * np.arange(64) + rng.normal(0, 1.5, 64)
        curve = lambda q: float(psnr[q])                               # noqa: E731
        target = float(rng.uniform(psnr.min() - 1, psnr.max() + 1))
        for qp_min, qp_max in ((0, 63), (7, 29), (20, 29), (0, 1)):
            start = int(rng.integers(0, 64))
            qp_n, tried_n = _native(curve, target, start, qp_min, qp_max)
            qp_p, tried_p = _python(curve, target, start, qp_min, qp_max)
            assert (qp_n, tried_n) == (qp_p, tried_p)
            assert len(tried_p) <= _cap(qp_min, qp_max)
            _check_procedure(qp_p, tried_p, lambda q: psnr[q] >= target, start, qp_min, qp_max)


def test_a_start_outside_the_range_is_clamped():
    curve = lambda q: 30.0 + 0.25 * q                                  # noqa: E731
    for start in (-4, 90):
        assert _native(curve, 36.0, start, 0, 63) == _python(curve, 36.0, start, 0, 63)
        assert _python(curve, 36.0, start, 0, 63)[0] == 24


def test_search_failures():
    f = _pick()
    nan = float("nan")
    assert f(_MEASURE(lambda q, u: nan), None, 35.0, 30, 0, 63, None) < 0            # NaN = the trial failed
    assert "pick_qp_for_quality" in _lib.lib().dcvc_last_error().decode()
    seen = []

    def second_fails(q, u):
        seen.append(q)
        return 40.0 if len(seen) == 1 else nan

    n = _ci(-1)
    assert f(_MEASURE(second_fails), None, 35.0, 30, 0, 63, ctypes.byref(n)) < 0 and seen == [30, 29] and n.value == 2
    assert f(_MEASURE(lambda q, u: 1.0), None, 35.0, 8, 9, 8, None) < 0              # qp_min above qp_max
    assert f(_MEASURE(0), None, 35.0, 8, 0, 63, None) < 0                              # no callback
    with pytest.raises(ValueError):
        rc.pick_qp_for_quality(lambda q: nan, 35.0, 30)
    with pytest.raises(ValueError):
        rc.pick_qp_for_quality(lambda q: 1.0, 35.0, 8, 9, 8)


# ---------------------------------------------------------------- the quality loop
class _Clip:
    """stand-in codec: the quality of a unit at q_index q is base + 0.2 q, minus `drop` from picture `jump_at` on; a P unit's
    trials must start from the state in front of the unit, which the stand-in checks"""

    def __init__(self, frames, jump_at=None, drop=4.0):
        self.frames, self.jump_at, self.drop = frames, jump_at, drop
        self.state, self.saved, self.trials = 0, None, []

    def _quality(self, idx, qp, base):
        return base + 0.2 * qp - (self.drop if self.jump_at is not None and idx >= self.jump_at else 0.0)

    def trial_intra(self, idx, qp):
        self.trials.append((idx, qp))
        return self._quality(idx, qp, 33.0)

    def trial_inter(self, idx, n, qp, reset, first):
        if first:
            self.saved = self.state
        else:
            self.state = self.saved
        assert self.state == idx                                       # every trial starts in front of the unit
        self.state = idx + 1000 * (qp + 1)                             # ... and leaves the state behind a coding at qp
        self.trials.append((idx, qp))
        return self._quality(idx, qp, 30.0)

    def commit(self, intra, idx, n, qp, reset, last_qp):
        if not intra:
            if qp != last_qp:
                self.state = self.saved + 1000 * (qp + 1)
            assert self.state == idx + 1000 * (qp + 1)
        self.state = idx + (1 if intra else self.delay)
        return bytes([qp])


@pytest.mark.parametrize("frames,delay,intra_period,reset_interval,jump_at", [
    (40, 1, -1, 32, None), (40, 1, -1, 4, 20), (60, 8, -1, 32, 30), (77, 8, 32, 32, 40), (40, 1, 16, 8, 20),
])
def test_quality_loop_on_a_synthetic_model(frames, delay, intra_period, reset_interval, jump_at):
    clip = _Clip(frames, jump_at=jump_at)
    clip.delay = delay
    log = []
    target = 36.1
    units = rc.code_sequence_quality(frames, delay, clip.trial_intra, clip.trial_inter, clip.commit, target, qp_i=30,
                                     intra_period=intra_period, reset_interval=reset_interval, log=log)
    plain = rc.code_sequence(frames, delay, lambda i, q: b"", lambda i, n, q, r: b"", rc.ConstantQP(30), intra_period=intra_period,
                             reset_interval=reset_interval)
    assert [(u[0], u[2]) for u in units] == [(u[0], u[2]) for u in plain]      # types and reset flags: code_sequence's
    start, idx = {True: 30, False: 30}, 0
    for (intra, qp, reset, payload), entry in zip(units, log):
        assert entry["type"] == ("I" if intra else "P") and entry["qp"] == qp == payload[0]
        assert entry["trace"][0][0] == start[intra] and 2 <= entry["trials"] == len(entry["trace"]) <= 12
        base = 33.0 if intra else 30.0
        assert clip._quality(idx, qp, base) >= target > clip._quality(idx, qp - 1, base)
        assert (qp - 1, clip._quality(idx, qp - 1, base)) in entry["trace"]
        start[intra] = qp
        idx += 1 if intra else delay
    assert len(clip.trials) == sum(e["trials"] for e in log)
    p_qps = [u[1] for u in units if not u[0]]
    if jump_at is not None:                # 4 dB down at every q_index: 20 steps up
        assert max(p_qps) - min(p_qps) == 20, p_qps
    steady = [e["trials"] for e, u in zip(log[2:], units[2:]) if e["trace"][0][0] == e["qp"]]
    assert steady and set(steady) == {2}                              # the q_index stays: 2 trials
