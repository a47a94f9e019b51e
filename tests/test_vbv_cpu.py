"""The decoder-buffer cap without a device: the native model (dcvc_rc_vbv_*, include/dcvc_amd_rc.h) against
rate_control.Vbv with == on the fullness, the refusals of both, vbv_replay on a case computed by hand, the container's
overhead helper against its writers, and the fitting procedure - vbv_fit and the three loops that run it - on a stand-in codec
whose sizes rise with the q_index and whose coded size exceeds the prediction by a chosen amount."""
import ctypes
import io

import numpy as np
import pytest

from dcvc_amd import _lib, rate_control as rc, stream_helper as sh

_vp, _ci, _cd, _i64, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64, ctypes.c_longlong


def _fn():
    return dict(
        create=_lib.fn("dcvc_rc_vbv_create", _vp, [_cd, _cd, _cd, _ll]),
        destroy=_lib.fn("dcvc_rc_vbv_destroy", None, [_vp]),
        available=_lib.fn("dcvc_rc_vbv_available", _i64, [_vp]),
        admit=_lib.fn("dcvc_rc_vbv_admit", _ci, [_vp, _i64, _ci]),
        fullness=_lib.fn("dcvc_rc_vbv_fullness", _cd, [_vp]),
        capacity=_lib.fn("dcvc_rc_vbv_capacity", _cd, [_vp]),
        rate=_lib.fn("dcvc_rc_vbv_rate", _cd, [_vp]),
        underflow=_lib.fn("dcvc_rc_vbv_underflow", _i64, [_vp]),
    )


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("seed", range(8))
def test_native_model_equals_python_on_random_units(seed):
    rng = np.random.default_rng(seed)
    f = _fn()
    pixels = int(rng.integers(64 * 64, 3840 * 2160))
    maxrate, bufsize, init = float(2.0 ** rng.uniform(-8, 0)), float(rng.uniform(0.5, 40)), float(rng.uniform(0.05, 1.0))
    py = rc.Vbv(maxrate, bufsize, pixels, init)
    h = f["create"](maxrate, bufsize, init, pixels)
    assert h
    try:
        assert (f["rate"](h), f["capacity"](h), f["fullness"](h)) == (py.rate, py.capacity, py.fullness)
        assert py.rate == maxrate * pixels and py.capacity == bufsize * py.rate and py.fullness == init * py.capacity
        seen = dict(clamped=0, violated=0, chunks=0, conform=0)
        for _ in range(600):
            kind = rng.random()
            pictures = 8 if kind < 0.3 else int(rng.integers(1, 9)) if kind < 0.4 else 1
            # around what arrives, far below it (the bucket fills to the clamp) and far above it (violations)
            scale = float(2.0 ** rng.choice([-6.0, -1.0, 0.0, 0.5, 3.0], p=[0.25, 0.2, 0.3, 0.15, 0.1]))
            bits = int(py.rate * pictures * scale * rng.uniform(0.5, 1.5))
            assert f["available"](h) == py.available_bits() == int(np.floor(py.fullness))
            before, avail = py.fullness, py.available_bits()
            got_n, got_p = f["admit"](h, bits, pictures), py.admit(bits, pictures)
            assert got_n == got_p == (1 if bits > avail else 0)
            assert f["fullness"](h) == py.fullness, (before, bits, pictures)            # ==, on doubles
            assert f["underflow"](h) == py.underflow == (bits - avail if got_p else 0)
            if got_p:
                assert py.fullness == min(py.capacity, max(0.0, before - bits) + pictures * py.rate)
            else:
                assert py.fullness == min(py.capacity, (before - bits) + pictures * py.rate)
            assert 0.0 <= py.fullness <= py.capacity
            seen["clamped"] += py.fullness == py.capacity
            seen["violated"] += got_p
            seen["conform"] += 1 - got_p
            seen["chunks"] += pictures == 8
        assert all(v > 10 for v in seen.values()), seen                               # every branch was walked
    finally:
        f["destroy"](h)


BAD = [(float("nan"), 4, 0.9, 100), (float("inf"), 4, 0.9, 100), (0.0, 4, 0.9, 100), (-0.1, 4, 0.9, 100),
       (0.1, float("nan"), 0.9, 100), (0.1, float("inf"), 0.9, 100), (0.1, 0.0, 0.9, 100), (0.1, -2, 0.9, 100),
       (0.1, 4, float("nan"), 100), (0.1, 4, 0.0, 100), (0.1, 4, -0.5, 100), (0.1, 4, 1.0000001, 100), (0.1, 4, float("inf"), 100),
       (0.1, 4, 0.9, 0), (0.1, 4, 0.9, -5), (1e300, 1e10, 0.9, 100)]


@pytest.mark.parametrize("maxrate,bufsize,init,pixels", BAD)
def test_refusals(maxrate, bufsize, init, pixels):
    f = _fn()
    assert f["create"](maxrate, bufsize, init, pixels) is None
    assert "vbv" in _lib.lib().dcvc_last_error().decode()
    with pytest.raises(ValueError):
        rc.Vbv(maxrate, bufsize, pixels, init)


def test_admit_refusals_and_the_edges_that_pass():
    f = _fn()
    h = f["create"](0.1, 10.0, 1.0, 1000)                        # init 1 is allowed
    py = rc.Vbv(0.1, 10, 1000, init=1.0)
    try:
        assert f["fullness"](h) == py.fullness == py.capacity == 1000.0
        for bits, pictures in ((-1, 1), (10, 0), (10, -3)):
            assert f["admit"](h, bits, pictures) < 0
            with pytest.raises(ValueError):
                py.admit(bits, pictures)
            assert f["fullness"](h) == py.fullness == 1000.0     # unchanged
        assert f["admit"](h, 0, 1) == py.admit(0, 1) == 0        # an empty unit is a unit
        assert f["available"](None) < 0 and f["admit"](None, 1, 1) < 0
    finally:
        f["destroy"](h)
    assert rc.Vbv(0.1, 10, 1000).fullness == 0.9 * 1000.0        # the default start


def test_replay_of_a_case_computed_by_hand():
    """r = 0.1 * 1000 = 100, C = 10 r = 1000, F = 0.9 C = 900.
    unit 0: 900 bits, 1 picture: avail 900, fits exactly -> F = min(1000, (900 - 900) + 100) = 100, slack 0
    unit 1: 50 bits, 1 picture:  avail 100 -> F = (100 - 50) + 100 = 150, slack 50
    unit 2: 300 bits, 8 pictures: avail 150: a violation, underflow 150 -> F = min(1000, max(0, -150) + 800) = 800, slack -150"""
    fullness, slack, violations = rc.vbv_replay([(900, 1), (50, 1), (300, 8)], 0.1, 10, 1000)
    assert fullness == [900.0, 100.0, 150.0, 800.0]
    assert slack == -150 and violations == [(2, 150)]
    # one more chunk that takes nothing: the top clamps, nothing is padded
    fullness, slack, violations = rc.vbv_replay([(900, 1), (50, 1), (300, 8), (0, 8)], 0.1, 10, 1000)
    assert fullness[-1] == 1000.0 and violations == [(2, 150)]
    # fractional fullness: avail is its floor
    fullness, slack, violations = rc.vbv_replay([(225, 1), (226, 1)], 0.1, 2.5, 1001, init=0.9)
    assert fullness[0] == 0.9 * (2.5 * (0.1 * 1001)) and int(fullness[0]) == 225
    assert slack == min(0, int(np.floor(fullness[1])) - 226) and [v[0] for v in violations] == ([1] if slack < 0 else [])
    assert rc.vbv_replay([], 0.1, 10, 1000) == ([900.0], None, [])


# ---------------------------------------------------------------- the container's overhead helper
LENGTHS = [0, 1, 126, 127, 128, 129, 16382, 16383, 16384, 16385, 70000]
SIZES = [None, (144, 176), (127, 127), (127, 128), (128, 127), (1080, 1920), (16383, 16383), (16383, 16384), (16384, 16383), (20000, 20000)]


@pytest.mark.parametrize("size", SIZES)
def test_unit_overhead_against_the_writers(size):
    native = _lib.fn("dcvc_stream_unit_overhead", _i64, [ctypes.c_size_t, _ci, _ci, _ci])
    write_ip = _lib.fn("dcvc_stream_write_ip", _i64, [_vp, ctypes.c_size_t, _ci, _ci, _ci, _ci, _ci, _vp, ctypes.c_size_t])
    write_sps = _lib.fn("dcvc_stream_write_sps", _ci, [_vp, ctypes.c_size_t, _ci, _ci, _ci])
    sps = None if size is None else dict(sps_id=0, height=size[0], width=size[1])
    last = 0
    for n in LENGTHS:
        payload = bytes(n)
        f = io.BytesIO()
        written = (sh.write_sps(f, sps) if sps else 0) + sh.write_ip(f, False, 0, 31, 2, True, payload)
        assert written == len(f.getvalue())
        want = written - n
        assert sh.unit_overhead(n, sps) == want
        h, w = size or (0, 0)
        assert native(n, 1 if sps else 0, h, w) == want
        # ... and the native writers, asked for the size alone
        buf = ctypes.create_string_buffer(payload, max(n, 1))
        native_written = write_ip(None, 0, 0, 0, 31, 2, 1, ctypes.addressof(buf), n) + (write_sps(None, 0, 0, h, w) if sps else 0)
        assert native_written == written
        assert want >= last                                       # never smaller for a longer payload
        last = want
    assert last == 3 + 4 + (0 if sps is None else 1 + sum(1 if v < 128 else 2 if v < 16384 else 4 for v in size))


def test_unit_overhead_refusals():
    native = _lib.fn("dcvc_stream_unit_overhead", _i64, [ctypes.c_size_t, _ci, _ci, _ci])
    assert native((1 << 30) - 1, 0, 0, 0) == 7
    assert native(1 << 30, 0, 0, 0) == -1
    assert native(10, 1, -1, 10) == -1 and native(10, 1, 10, 1 << 30) == -1
    assert native(10, 0, -1, -1) == 4                             # no parameter set: the size is not looked at
    with pytest.raises(ValueError):
        sh.unit_overhead(1 << 30)
    with pytest.raises(ValueError):
        sh.unit_overhead(10, dict(height=-1, width=10))


def test_payload_budget_is_safe_and_tight():
    """every payload within the budget makes a unit that fits avail; and the budget is not a byte too small where the length
    field does not change size"""
    for sps in (None, dict(height=144, width=176)):
        overhead = lambda n: sh.unit_overhead(n, sps)            # noqa: E731
        for avail in list(range(0, 300)) + list(range(8 * 120, 8 * 140)) + list(range(8 * 16380, 8 * 16400)) + [-5, 10 ** 12]:
            budget = rc.vbv_payload_budget(avail, overhead)
            n = budget // 8
            if n >= 0:
                n = min(n, rc.MAX_PAYLOAD_BYTES)
                assert 8 * (n + overhead(n)) <= avail
            if 0 <= n < rc.MAX_PAYLOAD_BYTES and overhead(n + 1) == overhead(max(avail, 0) // 8):
                assert 8 * (n + 1 + overhead(n + 1)) > avail


# ---------------------------------------------------------------- the fitting procedure on a stand-in codec
class FakeCodec:
    """predicted payload bytes size(q) = base 2^(q / 16), rising with q; the coded payload is excess(q) bytes longer"""

    def __init__(self, base=400, excess=lambda q: 0):
        self.base, self.excess = base, excess
        self.calls = []

    def size(self, q):
        return int(self.base * 2.0 ** (q / 16.0))

    def probe(self, q):
        self.calls.append(("probe", q))
        return 8 * self.size(q)

    def code(self, q):
        self.calls.append(("code", q))
        return bytes(self.size(q) + self.excess(q))

    def restore(self):
        self.calls.append(("restore", None))


def _overhead(n):
    return sh.unit_overhead(n, None)


def _bucket(avail_bits):
    """a model whose avail is exactly avail_bits: r = 1000 bits, C = F"""
    v = rc.Vbv(1.0, avail_bits / 1000.0, 1000, init=1.0)
    assert v.available_bits() == avail_bits
    return v


def test_fit_accepts_at_once_without_a_probe():
    codec = FakeCodec()
    q = 20
    bits = 8 * (codec.size(q) + _overhead(codec.size(q)))
    vbv = _bucket(bits)                                           # fits exactly
    fit = rc.vbv_fit(vbv, 1, q, 0, codec.code, codec.probe, _overhead, codec.restore)
    assert codec.calls == [("code", q)]
    assert (fit["qp_mode"], fit["qp"], fit["probes"], fit["recodes"], fit["predicted_bits"]) == (q, q, 0, 0, None)
    assert fit["bytes"] == bits // 8 and not fit["violated"] and fit["underflow_bits"] == 0
    assert fit["fullness_before"] == float(bits) and fit["fullness_after"] == min(vbv.capacity, 0.0 + 1000.0) == vbv.fullness
    # a searching mode's probes and prediction pass through
    fit = rc.vbv_fit(_bucket(bits), 1, q, 0, codec.code, codec.probe, _overhead, None, mode_probes=3, mode_predicted_bits=777)
    assert (fit["probes"], fit["predicted_bits"], fit["recodes"]) == (3, 777, 0)


@pytest.mark.parametrize("with_restore", [True, False])
def test_fit_miss_search_fit(with_restore):
    codec = FakeCodec()
    q_mode, want_q, floor_q = 40, 29, 3
    avail = 8 * (codec.size(want_q) + _overhead(codec.size(want_q))) + 5       # q 29 fits, q 30 does not
    assert 8 * (codec.size(want_q + 1) + _overhead(codec.size(want_q + 1))) > avail
    vbv = _bucket(avail)
    fit = rc.vbv_fit(vbv, 8, q_mode, floor_q, codec.code, codec.probe, _overhead, codec.restore if with_restore else None, mode_probes=2)
    # the search alone, on the payload budget, from q_mode - 1 inside [floor_q, q_mode - 1]
    trace = []
    alone = rc.pick_qp_near(lambda q: 8 * codec.size(q), rc.vbv_payload_budget(avail, _overhead), q_mode - 1, floor_q, q_mode - 1, trace=trace)
    assert alone == want_q and fit["qp"] == want_q and fit["qp_mode"] == q_mode
    assert fit["probes"] == 2 + len(trace) and fit["recodes"] == 1
    assert fit["predicted_bits"] == 8 * codec.size(want_q)
    want_calls = [("code", q_mode)] + ([("restore", None)] if with_restore else []) + [("probe", q) for q, _ in trace] + [("code", want_q)]
    assert codec.calls == want_calls                                            # one restore, none between the probes
    assert not fit["violated"] and fit["bytes"] == codec.size(want_q) + _overhead(codec.size(want_q))
    assert fit["fullness_after"] == min(vbv.capacity, (float(avail) - 8 * fit["bytes"]) + 8 * 1000.0)


def test_fit_steps_down_when_the_coder_exceeds_the_prediction():
    codec = FakeCodec(excess=lambda q: 40)                        # 40 bytes over the prediction at every q_index
    q_mode, floor_q = 40, 0
    budget_q = 29
    avail = 8 * (codec.size(budget_q) + _overhead(codec.size(budget_q))) + 5   # the prediction of q 29 fits ...
    assert codec.size(budget_q) + 40 > avail // 8 - _overhead(codec.size(budget_q))           # ... its coding does not
    fits = [q for q in range(64) if 8 * (len(bytes(codec.size(q) + 40)) + _overhead(codec.size(q) + 40)) <= avail]
    want_q = max(fits)
    assert want_q == budget_q - 1                                 # exactly one extra step down
    fit = rc.vbv_fit(_bucket(avail), 1, q_mode, floor_q, codec.code, codec.probe, _overhead, codec.restore)
    assert fit["qp"] == want_q and fit["recodes"] == 2 and not fit["violated"]
    assert codec.calls[-3:] == [("code", budget_q), ("restore", None), ("code", want_q)]
    probed = dict((q, 8 * codec.size(q)) for kind, q in codec.calls if kind == "probe")
    assert fit["predicted_bits"] == probed.get(want_q)            # the prediction of the final q_index when it was probed
    assert fit["probes"] == len(probed)
    assert [c for c in codec.calls if c[0] == "restore"] == [("restore", None)] * 2


def test_fit_nothing_fits_at_the_floor():
    codec = FakeCodec()
    q_mode, floor_q = 12, 7
    avail = 8 * codec.size(floor_q) - 100                         # below even the payload at the floor
    vbv = _bucket(avail)
    fit = rc.vbv_fit(vbv, 1, q_mode, floor_q, codec.code, codec.probe, _overhead, codec.restore)
    nbytes = codec.size(floor_q) + _overhead(codec.size(floor_q))
    assert fit["qp"] == floor_q and fit["violated"] and fit["bytes"] == nbytes
    assert fit["underflow_bits"] == 8 * nbytes - avail == vbv.underflow
    assert fit["fullness_after"] == min(vbv.capacity, max(0.0, float(avail) - 8 * nbytes) + 1000.0) == 1000.0
    assert codec.calls[-1] == ("code", floor_q) and fit["recodes"] == 1         # the search ends at the floor: no step is left
    # q_mode at the floor already: written as it is, no probe
    codec2 = FakeCodec()
    fit = rc.vbv_fit(_bucket(avail), 1, floor_q, floor_q, codec2.code, codec2.probe, _overhead, codec2.restore)
    assert codec2.calls == [("code", floor_q)] and fit["violated"] and (fit["probes"], fit["recodes"]) == (0, 0)


# ---------------------------------------------------------------- the three loops
N, PIXELS, SIZE = 21, 176 * 144, (144, 176)


class FakeSequence:
    """I pictures 8 times a P picture; the coded payload is 1.5 % over the prediction"""

    def __init__(self):
        self.events = []

    def _bytes(self, idx, n, q, intra):
        return int((2400 if intra else 300 * n) * (1.0 + 0.1 * ((idx * 7) % 5)) * 2.0 ** (q / 16.0))

    def code_intra(self, idx, q):
        self.events.append(("code_i", idx, q))
        return bytes(int(self._bytes(idx, 1, q, True) * 1.015))

    def code_inter(self, idx, n, q, reset):
        self.events.append(("code_p", idx, q))
        return bytes(int(self._bytes(idx, n, q, False) * 1.015))

    def probe_intra(self, idx, q):
        return 8 * self._bytes(idx, 1, q, True)

    def probe_inter(self, idx, n, q):
        return 8 * self._bytes(idx, n, q, False)

    def snapshot(self):
        self.events.append(("snapshot",))

    def restore(self):
        self.events.append(("restore",))

    def accept(self, intra, idx, q):
        self.events.append(("accept", idx, q))

    def hooks(self, log):
        return dict(probe_intra=self.probe_intra, snapshot=self.snapshot, restore=self.restore, accept=self.accept,
                    picture_size=SIZE, vbv_log=log)


def _run_loop(loop, delay, s, vbv, log):
    if loop == "constant":
        hooks = dict(s.hooks(log), probe_inter=s.probe_inter) if vbv else {}
        return rc.code_sequence(N, delay, s.code_intra, s.code_inter, rc.ConstantQP(36, 40), reset_interval=4, vbv=vbv, **hooks)
    if loop == "feedback":
        hooks = dict(s.hooks(log), probe_inter=s.probe_inter) if vbv else {}
        ctl = rc.TargetBpp(0.5, PIXELS, qp0=36, horizon=6, intra_bonus=2, qp_min=4)
        return rc.code_sequence(N, delay, s.code_intra, s.code_inter, ctl, reset_interval=4, vbv=vbv, **hooks)
    if loop == "probed":
        hooks = s.hooks(log) if vbv else {}
        return rc.code_sequence_probed(N, delay, s.code_intra, s.code_inter, s.probe_inter, 0.5, PIXELS, qp_i=36, horizon=6,
                                       intra_bonus=2, qp_min=4, reset_interval=4, vbv=vbv, **hooks)
    hooks = {k: v for k, v in s.hooks(log).items() if k != "probe_intra"} if vbv else {}
    return rc.code_sequence_intra_search(N, s.code_intra, s.probe_intra, 4.0, PIXELS, qp_min=4, vbv=vbv, **hooks)


def _old_loops(loop, delay, s):
    """the loops as they were before they learnt vbv=: restated here for the all-intra search, which the tests ran inline"""
    if loop != "intra":
        return None
    units, spent = [], 0
    for k in range(N):
        budget = rc.intra_budget_bits(4.0, PIXELS, k, spent)
        qp = rc.pick_qp_for_budget(lambda q: s.probe_intra(k, q), budget, 4, 63)
        payload = s.code_intra(k, qp)
        spent += 8 * len(payload)
        units.append((True, qp, False, payload))
    return units


CASES = [("constant", 1), ("constant", 8), ("feedback", 1), ("probed", 1), ("probed", 8), ("intra", 1)]


@pytest.mark.parametrize("loop,delay", CASES)
def test_loops_under_a_cap(loop, delay):
    plain_s = FakeSequence()
    plain = _run_loop(loop, delay, plain_s, None, None)
    assert not any(e[0] in ("snapshot", "restore", "accept") for e in plain_s.events)
    old = _old_loops(loop, delay, FakeSequence())
    if old is not None:
        assert plain == old
    floor_q = 0 if loop == "constant" else 4

    def units_of(coded):
        out, idx = [], 0
        for k, (intra, qp, reset, payload) in enumerate(coded):
            n = 1 if intra else min(delay, N - idx)
            out.append((8 * (len(payload) + sh.unit_overhead(len(payload), dict(height=SIZE[0], width=SIZE[1]) if k == 0 else None)), n))
            idx += 1 if intra else delay
        return out

    # a bucket that never binds: the plain run's units, one snapshot per P unit, no restore, no probe of the cap's
    big = rc.Vbv(100.0, 50, PIXELS)
    s, log = FakeSequence(), []
    coded = _run_loop(loop, delay, s, big, log)
    assert coded == plain
    assert all(u["recodes"] == 0 and u["qp"] == u["qp_mode"] and not u["violated"] for u in log)
    assert sum(e[0] == "snapshot" for e in s.events) == sum(not u[0] for u in plain) and not any(e[0] == "restore" for e in s.events)
    assert [e for e in s.events if e[0] == "accept"] == [("accept", u["first_picture"], u["qp"]) for u in log]

    # a tight one: 0.95 of the plain run's mean bits per picture - the pictures' sizes spread by 1.4, so some units fit as they
    # are and some do not; the smallest whole bufsize at which the floor run conforms
    p_bits = [b for (b, n), u in zip(units_of(plain), plain) if not u[0]] or [b for b, n in units_of(plain)]
    p_pictures = sum(n for (b, n), u in zip(units_of(plain), plain) if not u[0]) or N
    maxrate = 0.95 * sum(p_bits) / (p_pictures * PIXELS)
    fs = FakeSequence()
    floor_run = rc.code_sequence(N, delay, fs.code_intra, fs.code_inter, rc.ConstantQP(floor_q), reset_interval=4,
                                 force_intra=loop == "intra")
    bufsize = next(b for b in range(1, 10000) if not rc.vbv_replay(units_of(floor_run), maxrate, b, PIXELS)[2])
    vbv = rc.Vbv(maxrate, bufsize, PIXELS)
    s, log = FakeSequence(), []
    coded = _run_loop(loop, delay, s, vbv, log)
    assert [u[0] for u in coded] == [u[0] for u in plain] and [u[2] for u in coded] == [u[2] for u in plain]
    # the log is the model's replay of the units, and nothing sticks out
    fullness, slack, violations = rc.vbv_replay(units_of(coded), maxrate, bufsize, PIXELS)
    assert [u["fullness_before"] for u in log] == fullness[:-1] and [u["fullness_after"] for u in log] == fullness[1:]
    assert [8 * u["bytes"] for u in log] == [b for b, n in units_of(coded)] and [u["pictures"] for u in log] == [n for b, n in units_of(coded)]
    # The procedure's promise: a unit that sticks out was coded at the floor. With one-picture units nothing does: the floor
    # run's units are each below what one picture period brings, and a unit that conforms leaves at least that behind it. A
    # chunk of 8 right behind an I picture that took the bucket finds one period's bits, and may not fit at any q_index.
    assert [i for i, u in enumerate(log) if u["violated"]] == [v[0] for v in violations]
    assert all(u["qp"] == floor_q and u["underflow_bits"] == dict(violations)[i] for i, u in enumerate(log) if u["violated"])
    if delay == 1:
        assert violations == [] and slack >= 0
    assert [u["qp"] for u in log] == [u[1] for u in coded] and all(floor_q <= u["qp"] <= u["qp_mode"] for u in log)
    lowered = [u for u in log if u["qp"] < u["qp_mode"]]
    assert lowered, "the cap was not used"
    if delay == 1 and loop != "feedback":     # (the controller chases a rate above the cap, and 21 pictures are 4 units in chunks of 8)
        assert any(u["recodes"] == 0 for u in log), "no unit was accepted as the mode gave it"
    # a unit coded again sits below what its mode gave; a mode that searches is held under the cap by its own search, and
    # says with qp_mode what its own budget would have allowed
    assert all(u["qp"] < u["qp_mode"] for u in log if u["recodes"] > 0)
    searched = [u for u in log if loop == "intra" or (loop == "probed" and u["type"] == "P")]
    assert all((u["recodes"] > 0) == (u["qp"] < u["qp_mode"]) for u in log if u not in searched)
    if searched:
        assert any(u["recodes"] == 0 and u["qp"] < u["qp_mode"] for u in searched)
    # every coding of a P unit after the first starts from the snapshot; an I picture is accepted once, after its last coding
    codings = {}
    for e in s.events:
        if e[0] in ("code_i", "code_p"):
            codings[e[1]] = codings.get(e[1], 0) + 1
    assert [codings[u["first_picture"]] - 1 for u in log] == [u["recodes"] for u in log]
    assert sum(e[0] == "restore" for e in s.events) == sum(u["recodes"] for u in log if u["type"] == "P")
    assert sum(e[0] == "snapshot" for e in s.events) == sum(u["type"] == "P" for u in log)
    for u in log:
        i = s.events.index(("accept", u["first_picture"], u["qp"]))
        kind = "code_i" if u["type"] == "I" else "code_p"
        assert s.events[i - 1] == (kind, u["first_picture"], u["qp"])


def test_a_capped_loop_needs_the_picture_size():
    s = FakeSequence()
    with pytest.raises(ValueError):
        rc.code_sequence(4, 1, s.code_intra, s.code_inter, rc.ConstantQP(30), vbv=rc.Vbv(1.0, 4, PIXELS))


# ---------------------------------------------------------------- the controller's update at another q_index
def test_native_update_at_equals_python():
    create = _lib.fn("dcvc_rc_create", _vp, [_cd, _cd, _cd, _ci, _ci, _ci, _ci, _cd])
    destroy = _lib.fn("dcvc_rc_destroy", None, [_vp])
    next_qp = _lib.fn("dcvc_rc_next_qp", _ci, [_vp, _ci])
    update = _lib.fn("dcvc_rc_update", _ci, [_vp, _cd, _ci, _ci])
    update_at = _lib.fn("dcvc_rc_update_at", _ci, [_vp, _cd, _ci, _ci, _ci])
    state = _lib.fn("dcvc_rc_state_qp", _cd, [_vp])
    for seed in range(4):
        rng = np.random.default_rng(seed)
        pixels = int(rng.integers(64 * 64, 1920 * 1080))
        kw = dict(qp0=float(rng.integers(10, 50)), horizon=int(rng.integers(1, 12)), intra_bonus=int(rng.integers(-2, 5)),
                  qp_min=int(rng.integers(0, 10)), qp_max=63, slope=0.049)
        target = float(2.0 ** rng.uniform(-6, -1))
        py, plain = rc.TargetBpp(target, pixels, **kw), rc.TargetBpp(target, pixels, **kw)
        h = create(target, pixels, kw["qp0"], kw["horizon"], kw["intra_bonus"], kw["qp_min"], kw["qp_max"], kw["slope"])
        try:
            same = True
            for _ in range(300):
                intra = bool(rng.random() < 0.1)
                pictures = int(rng.choice([1, 8]))
                q = py.next_qp(intra)
                assert next_qp(h, 1 if intra else 0) == q
                bits = int(target * pixels * pictures * 2.0 ** rng.normal(0, 0.5))
                lowered = int(rng.integers(0, q + 1)) if rng.random() < 0.4 else q
                same = same and lowered == q
                py.update(bits, pictures, intra, qp=lowered)
                assert update_at(h, float(bits), pictures, 1 if intra else 0, lowered) == 0
                assert state(h) == py.qp                          # the fractional state, bit for bit
                if same:                                          # at the controller's own q_index it is update()
                    plain.update(bits, pictures, intra)
                    assert plain.qp == py.qp and plain.slope == py.slope
        finally:
            destroy(h)
    assert update(None, 1.0, 1, 0) < 0 and update_at(None, 1.0, 1, 0, 3) < 0
