"""Rate-control hook of the coding loop.

The reference harness codes a whole sequence with ONE q_index per rate point (test_video.py:512-514:
`linspace(0, 63, rate_num)`), but its stream container already carries the q_index of every picture
(stream_helper.py:134-135 write_ip / read_ip_remaining), so a decoder needs no side information when the encoder
changes it from picture to picture. This module is the encoder-side hook for that: a controller object the coding
loop asks for the q_index of the next coded unit and tells the bits the unit took, plus `code_sequence`, the
loop of test_video.py:204-257 (picture types, reset rule, chunk padding) with the q_index taken from the
controller instead of a constant. The native tool (csrc/cli/dcvc_cli.hip) codes with the reference's constant
--qp-i / --qp-p unless it is given --target-bpp; then it runs the same controller natively (csrc/codec/rate_control.cpp),
or, in all-intra runs, the budget search at the end of this module on the GPU size probe. With
--vbv-maxrate / --vbv-bufsize every unit of any of these modes is fitted into a decoder-buffer model (Vbv, vbv_fit,
code_sequence_capped at the end of this module).

In DCVC-UF a HIGHER q_index means finer quantisation = more bits (q 0 .. 63).
"""
import math


class ConstantQP:
    """The reference behaviour: one q_index for I pictures, one for P units."""

    def __init__(self, qp_i, qp_p=None):
        self.qp_i, self.qp_p = int(qp_i), int(qp_i if qp_p is None else qp_p)

    def next_qp(self, is_intra):
        return self.qp_i if is_intra else self.qp_p

    def update(self, bits, pictures, is_intra, qp=None):
        pass


class TargetBpp:
    """One-pass control towards an average of `target_bpp` bits per pixel over the sequence.

    Model: log2(bits of a unit) is roughly linear in the q_index (measured on the synthetic 1080p intra pictures:
    115 KB at q 0, 971 KB at q 63 -> 0.049 per step); the slope is re-estimated from the units seen so far. After
    every unit the controller compares the bits spent with the budget of the pictures coded and moves the q_index
    by the step count that would cancel the error over the next `horizon` pictures. I pictures get `intra_bonus`
    steps (they anchor a whole GOP)."""

    def __init__(self, target_bpp, pixels_per_picture, qp0=32, horizon=8, intra_bonus=0, qp_min=0, qp_max=63,
                 slope=0.049):
        if target_bpp <= 0 or pixels_per_picture <= 0:
            raise ValueError("target_bpp and pixels_per_picture must be positive")
        self.target_bits = float(target_bpp) * pixels_per_picture          # per picture
        self.qp = float(qp0)
        self.horizon, self.intra_bonus = max(1, int(horizon)), int(intra_bonus)
        self.qp_min, self.qp_max = int(qp_min), int(qp_max)
        self.slope = float(slope)
        self.max_step = 4.0                                                # q_index steps per update
        self.spent, self.pictures = 0.0, 0
        self._last = None                                                  # (qp, log2 bits per picture) of the last P unit

    def next_qp(self, is_intra):
        q = self.qp + (self.intra_bonus if is_intra else 0)
        return int(min(self.qp_max, max(self.qp_min, round(q))))

    def update(self, bits, pictures, is_intra, qp=None):
        """`qp`: the q_index the unit was coded at when it is not next_qp(is_intra) - a decoder-buffer cap lowered it
        (DESIGN.md 25). The slope estimate and the last P unit then take `qp`, and the size the step compares is projected
        from `qp` to the q_index the controller stands at, as the update behind an I picture projects the last P unit."""
        if pictures <= 0:
            return
        used_qp = self.next_qp(is_intra) if qp is None else int(qp)
        moved = (not is_intra) and used_qp != self.next_qp(False)
        self.spent += bits
        self.pictures += pictures
        per_picture = max(bits / pictures, 1.0)
        if not is_intra:
            if self._last is not None and used_qp != self._last[0]:
                s = (math.log2(per_picture) - self._last[1]) / (used_qp - self._last[0])
                if 0.005 < s < 0.5:                                        # keep a sane, positive slope
                    self.slope = 0.75 * self.slope + 0.25 * s
            self._last = (used_qp, math.log2(per_picture))
        # bits the next `horizon` pictures may take so that the running average lands on the target
        budget = self.target_bits * (self.pictures + self.horizon) - self.spent
        want = max(budget / self.horizon, self.target_bits / 64.0)
        if is_intra:
            # An I picture costs several times the per-picture target by design: its bits count in `spent` (the budget above
            # already pays them back over the horizon), but its SIZE says nothing about what the P units cost at this qp, so it
            # does not enter the proportional term (advisor, round 3: it used to drop qp by ~34 steps behind every I picture).
            # Only the budget it leaves moves qp, measured against the last P unit if there is one.
            if self._last is None:
                return
            # ... projected to the q_index the controller stands at NOW: the last P unit was coded at self._last[0], and the
            # update behind it has already moved self.qp - comparing its raw size again would correct the same error twice
            # (advisor, round 4: q saw-toothed between 0 and 12 with intra period 32 in a simulation)
            per_picture = 2.0 ** (self._last[1] + self.slope * (self.qp - self._last[0]))
        elif moved:
            per_picture = 2.0 ** (self._last[1] + self.slope * (self.qp - self._last[0]))      # the unit just stored
        step = (math.log2(want) - math.log2(per_picture)) / self.slope
        self.qp += min(self.max_step, max(-self.max_step, step))           # bounded step: no oscillation with the intra period
        self.qp = min(float(self.qp_max), max(float(self.qp_min), self.qp))

    @property
    def spent_bits_per_picture(self):
        return self.spent / max(self.pictures, 1)


def code_sequence(frame_count, frames_per_p, code_intra, code_inter, controller, intra_period=-1, reset_interval=32,
                  force_intra=False, intra_at=None, vbv=None, **vbv_hooks):
    """The encode loop of test_video.py:204-257 with the q_index from `controller`.

    code_intra(frame_idx, qp) -> bytes-like          one I picture
    code_inter(frame_idx, n, qp, reset) -> bytes-like a P unit of frames_per_p pictures starting at frame_idx, of which
                                                      the first n exist in the source (the caller pads the rest by
                                                      repeating the last picture, test_video.py:104-110)
    intra_at(frame_idx, scheduled) -> bool            optional (dcvc encode --scene-cut, scene.SceneCut.push behind it): asked
                                                      once for every picture a unit starts with, in coding order, with the
                                                      index-based decision; its answer is the picture's type. None: the
                                                      index-based decision stands.
    vbv, a Vbv: every unit is fitted into the decoder buffer (vbv_fit) with the controller's q_index as
    q_mode, floor_q = the controller's qp_min (0 for ConstantQP); **vbv_hooks as code_sequence_capped takes them, probe_inter
    among them. None: the loop below, as it was.
    Returns [(is_intra, qp, reset, payload)] in coding order - what write_ip stores per unit."""
    if vbv is not None:
        def book(intra, qp, payload, n):
            controller.update(8 * len(payload), n, intra, qp=qp)
        return code_sequence_capped(frame_count, frames_per_p, code_intra, code_inter, vbv,
                                    lambda intra, idx, n, payload_avail: (controller.next_qp(intra), 0, None, None), book,
                                    floor_q=getattr(controller, "qp_min", 0), intra_period=intra_period,
                                    reset_interval=reset_interval, force_intra=force_intra, intra_at=intra_at, **vbv_hooks)
    units, idx = [], 0
    while idx < frame_count:
        # test_video.py:204-213: frame 0; every frame when intra_period == 1 (or --force_intra); with intra_period > 1
        # every frame with index % intra_period == 1 other than frame 1
        intra = idx == 0 or force_intra or intra_period == 1 or (intra_period > 1 and idx != 1 and idx % intra_period == 1)
        if intra_at is not None:
            intra = bool(intra_at(idx, intra))
        if intra:
            qp = controller.next_qp(True)
            payload = code_intra(idx, qp)
            controller.update(8 * len(payload), 1, True)
            units.append((True, qp, False, payload))
            idx += 1
            continue
        n = min(frames_per_p, frame_count - idx)
        reset = reset_interval > 0 and (idx + frames_per_p) % reset_interval == 1
        qp = controller.next_qp(False)
        payload = code_inter(idx, n, qp, reset)
        controller.update(8 * len(payload), n, False)
        units.append((False, qp, reset, payload))
        idx += frames_per_p
    return units


# ---- coding to a budget on a size probe. The native tool has the same functions
# (csrc/codec/rate_control.cpp, include/dcvc_amd_rc.h); the tests hold the two against each other probe for probe.

CODE_LENGTH_UNIT = 1 << 16          # size probes count in 2^-16 bit (csrc/rans/code_length.h)
MIN_SYMBOLS_PER_STREAM = 32768      # def_const.h:18


def ec_parallel_for(symbols):
    """sub-streams of a picture with that many coded y symbols (dmc_common.cpp:31-35)"""
    return min(8, max(1, int(symbols) // MIN_SYMBOLS_PER_STREAM))


def stream_fixed_bits(ec_parallel):
    """What the stream format adds to the coded symbols: every sub-stream ends with its 32-bit coder state, and a
    container of three or more sub-streams starts with n // 2 - 1 + n % 2 32-bit offsets."""
    n = int(ec_parallel)
    if not 1 <= n <= 8:
        raise ValueError("ec_parallel must be in [1, 8]")
    return 32 * n + 32 * (0 if n == 1 else n // 2 - 1 + n % 2)


def predicted_stream_bytes(y_units, z_units, ec_parallel):
    """ideal code length (2^-16 bit) -> predicted len(stream): the fixed bits on top, rounded up to bytes"""
    units = int(y_units) + int(z_units) + stream_fixed_bits(ec_parallel) * CODE_LENGTH_UNIT
    return (units + 8 * CODE_LENGTH_UNIT - 1) // (8 * CODE_LENGTH_UNIT)


def pick_qp_for_budget(estimate, budget_bits, qp_min=0, qp_max=63, trace=None):
    """Largest q_index whose predicted stream fits `budget_bits`, by bisection on estimate(qp) -> predicted bits.

    lo = qp_min - 1 counts as fitting, hi = qp_max + 1 as not; while hi - lo > 1: mid = (lo + hi) // 2 is probed,
    lo = mid if it fits, else hi = mid. The answer is lo, or qp_min when lo never moved: at most
    ceil(log2(qp_max - qp_min + 2)) probes. On a size curve that rises with the q_index that is the largest q_index that
    fits; on any curve it ends with "lo fits, lo + 1 was probed and does not". `trace`, a list, receives (qp, bits) of every
    probe."""
    if qp_min > qp_max:
        raise ValueError("qp_min above qp_max")
    lo, hi = qp_min - 1, qp_max + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        bits = int(estimate(mid))
        if trace is not None:
            trace.append((mid, bits))
        if bits <= budget_bits:
            lo = mid
        else:
            hi = mid
    return qp_min if lo < qp_min else lo


def pick_qp_near(estimate, budget_bits, start, qp_min=0, qp_max=63, trace=None):
    """pick_qp_for_budget's answer from a start value: neighbouring P units have neighbouring size curves, and a probe of
    an inter model costs 0.41 to 0.58 of a compress (measured at 1080p).

    s = start clamped to the range is probed. It fits: gallop upward - min(lo + step, qp_max) with step = 1, 2, 4, ...
    from lo = s, lo moving to every value that fits - to the first value that does not (hi), or until lo = qp_max. It does
    not: gallop downward from hi = s - max(hi - step, qp_min), hi moving to every value that does not fit - to the first
    that fits (lo), or until hi = qp_min. Then pick_qp_for_budget's bisection on (lo, hi), and its end: lo fits or is
    qp_min - 1, lo + 1 was probed and does not fit or is qp_max + 1; the answer is lo, or qp_min when nothing fits. No
    q_index is probed twice; 2 probes when the answer is start, at most 4 within 2 of it, at most
    2 ceil(log2(qp_max - qp_min + 2)) + 1 in any range (12 over 0 .. 63)."""
    if qp_min > qp_max:
        raise ValueError("qp_min above qp_max")

    def fits(qp):
        bits = int(estimate(qp))
        if trace is not None:
            trace.append((qp, bits))
        return bits <= budget_bits

    s = min(qp_max, max(qp_min, int(start)))
    lo, hi, step = qp_min - 1, qp_max + 1, 1
    if fits(s):
        lo = s
        while lo < qp_max:
            q = min(lo + step, qp_max)
            if not fits(q):
                hi = q
                break
            lo = q
            step *= 2
    else:
        hi = s
        while hi > qp_min:
            q = max(hi - step, qp_min)
            if fits(q):
                lo = q
                break
            hi = q
            step *= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid
    return qp_min if lo < qp_min else lo


def unit_budget_bits(target_bpp, pixels_per_picture, pictures_coded, spent_bits, horizon, n):
    """Budget of a P unit of n pictures, from what TargetBpp.update steers towards: the bits per picture that bring the
    running average onto the target over the next `horizon` pictures, at least 1/64 of a picture's share."""
    if horizon < 1 or n < 0:
        raise ValueError("horizon must be positive, n not negative")
    share = float(target_bpp) * pixels_per_picture
    budget = share * (pictures_coded + horizon) - float(spent_bits)
    want = max(budget / horizon, share / 64.0)
    return int(math.floor(want * n))


def code_sequence_probed(frame_count, frames_per_p, code_intra, code_inter, probe_inter, target_bpp, pixels_per_picture,
                         qp_i=32, horizon=8, intra_bonus=0, qp_min=0, qp_max=63, intra_period=-1, reset_interval=32,
                         force_intra=False, log=None, intra_at=None, vbv=None, **vbv_hooks):
    """code_sequence with every P unit's q_index searched on the size probe of the inter model (dcvc encode --rc-mode
    probe): the largest q_index whose predicted stream fits the unit's budget.

    probe_inter(frame_idx, n, qp) -> predicted bits of the P unit code_inter(frame_idx, n, qp, reset) would write; it
    must not advance the temporal state (DMCLDProxy / DMCHT*Proxy.estimate_bits).
    P unit of n existing pictures: pick_qp_near on the probe with the budget unit_budget_bits(...), start = the q_index
    of the previous P unit (qp_i for the first). I picture: start + intra_bonus clamped to the range, not probed; its bits
    count in what is spent. `log`, a list, receives per unit {type, qp, probes, predicted_bits, budget_bits, trace}.
    `intra_at` as in code_sequence. vbv, a Vbv: a P unit's search runs on min(its budget, the buffer's payload budget), and
    every unit is fitted into the decoder buffer (vbv_fit) with floor_q = qp_min; spent, pictures and the start
    value follow the final q_index and payload. **vbv_hooks as code_sequence_capped takes them (probe_inter is this
    function's). Returns what code_sequence returns."""
    if vbv is not None:
        state = dict(start=int(qp_i), spent=0, pictures=0)

        def q_mode(intra, idx, n, payload_avail):
            if intra:
                return min(qp_max, max(qp_min, state["start"] + int(intra_bonus))), 0, None, None
            own = unit_budget_bits(target_bpp, pixels_per_picture, state["pictures"], state["spent"], horizon, n)
            trace = []
            qp = pick_qp_near(lambda q: probe_inter(idx, n, q), min(own, payload_avail), state["start"], qp_min, qp_max, trace=trace)
            return qp, len(trace), dict(trace)[qp], vbv_searched_qp_mode(qp, trace, own)

        def book(intra, qp, payload, n):
            state["spent"] += 8 * len(payload)
            state["pictures"] += n
            if not intra:
                state["start"] = qp

        return code_sequence_capped(frame_count, frames_per_p, code_intra, code_inter, vbv, q_mode, book, floor_q=qp_min,
                                    intra_period=intra_period, reset_interval=reset_interval, force_intra=force_intra,
                                    intra_at=intra_at, probe_inter=probe_inter, **vbv_hooks)
    units, idx = [], 0
    start, spent, pictures = int(qp_i), 0, 0
    while idx < frame_count:
        intra = idx == 0 or force_intra or intra_period == 1 or (intra_period > 1 and idx != 1 and idx % intra_period == 1)
        if intra_at is not None:
            intra = bool(intra_at(idx, intra))
        if intra:
            qp = min(qp_max, max(qp_min, start + int(intra_bonus)))
            payload = code_intra(idx, qp)
            spent += 8 * len(payload)
            pictures += 1
            units.append((True, qp, False, payload))
            if log is not None:
                log.append(dict(type="I", qp=qp, probes=0, predicted_bits=None, budget_bits=None, trace=[]))
            idx += 1
            continue
        n = min(frames_per_p, frame_count - idx)
        reset = reset_interval > 0 and (idx + frames_per_p) % reset_interval == 1
        budget = unit_budget_bits(target_bpp, pixels_per_picture, pictures, spent, horizon, n)
        trace = []
        qp = pick_qp_near(lambda q: probe_inter(idx, n, q), budget, start, qp_min, qp_max, trace=trace)
        payload = code_inter(idx, n, qp, reset)
        spent += 8 * len(payload)
        pictures += n
        start = qp
        units.append((False, qp, reset, payload))
        if log is not None:
            log.append(dict(type="P", qp=qp, probes=len(trace), predicted_bits=dict(trace)[qp], budget_bits=budget, trace=trace))
        idx += frames_per_p
    return units


# ---- coding to a quality. The native tool has the same search (csrc/codec/rate_control.cpp,
# dcvc_rc_pick_qp_for_quality) and the same loop (dcvc encode --target-psnr); the tests hold them against each other.

def pick_qp_for_quality(measure, target, start, qp_min=0, qp_max=63, trace=None):
    """Smallest q_index whose trial coding meets a quality: measure(qp) -> quality, "meets" = measure(qp) >= target. The
    mirror image of pick_qp_near, and built on it through the index reflection q -> qp_min + qp_max - q with "fits" =
    "meets":

    s = start clamped to the range is tried. It meets: gallop downward - max(s - 1, qp_min), then 2, 4, ... further down from
    the last value that met - to the first value that does not meet, or until qp_min met. It does not: gallop upward in the
    same way to the first value that meets, or until qp_max did not. Then the bracket is bisected. The answer is the smallest
    bracketed q_index that meets, qp_max when nothing meets. pick_qp_near's counts: no q_index tried twice, 2 trials when the
    answer is start, at most 12 over 0 .. 63. A real model's quality rises with the q_index; nothing here assumes it.
    `trace`, a list, receives (qp, quality) of every trial. A NaN quality raises ValueError."""
    if qp_min > qp_max:
        raise ValueError("qp_min above qp_max")
    flip = qp_min + qp_max

    def misses(r):
        quality = float(measure(flip - r))
        if trace is not None:
            trace.append((flip - r, quality))
        if math.isnan(quality):
            raise ValueError("pick_qp_for_quality: the trial failed")
        return 0 if quality >= target else 1

    s = min(qp_max, max(qp_min, int(start)))
    return flip - pick_qp_near(misses, 0, flip - s, qp_min, qp_max)


def code_sequence_quality(frame_count, frames_per_p, trial_intra, trial_inter, commit, target, qp_i=32, qp_min=0, qp_max=63,
                          intra_period=-1, reset_interval=32, force_intra=False, log=None, intra_at=None):
    """code_sequence with every unit coded at the smallest q_index whose trial coding meets `target` (dcvc encode
    --target-psnr): pick_qp_for_quality on trial codings, start = the q_index of the previous unit of the same type (qp_i
    for the first of each type).

    trial_intra(frame_idx, qp) -> quality             codes the I picture as a trial and measures its reconstruction
    trial_inter(frame_idx, n, qp, reset, first) -> quality
                                                      codes the P unit (n existing pictures) as a trial and measures its
                                                      reconstruction over those n pictures. Every trial of a unit starts
                                                      from the temporal state in front of the unit: the caller exports it
                                                      when `first` is true and imports it before every later trial
    commit(is_intra, frame_idx, n, qp, reset, last_qp) -> bytes-like
                                                      the unit is the trial at qp: its stream, and the codec state behind
                                                      that trial from here on (an I picture: add_ref with its x_hat).
                                                      last_qp is the q_index of the last trial: when it is not qp the
                                                      caller kept that trial's stream and state, or codes it again from
                                                      the same state - the bytes are the same.
    `log`, a list, receives per unit {type, qp, trials, trace}; `intra_at` as in code_sequence. Returns what code_sequence
    returns."""
    units, idx = [], 0
    start = {True: int(qp_i), False: int(qp_i)}
    while idx < frame_count:
        intra = idx == 0 or force_intra or intra_period == 1 or (intra_period > 1 and idx != 1 and idx % intra_period == 1)
        if intra_at is not None:
            intra = bool(intra_at(idx, intra))
        n = 1 if intra else min(frames_per_p, frame_count - idx)
        reset = (not intra) and reset_interval > 0 and (idx + frames_per_p) % reset_interval == 1
        trace = []
        if intra:
            measure = lambda q: trial_intra(idx, q)
        else:
            measure = lambda q: trial_inter(idx, n, q, reset, not trace)
        qp = pick_qp_for_quality(measure, target, start[intra], qp_min, qp_max, trace=trace)
        payload = commit(intra, idx, n, qp, reset, trace[-1][0])
        start[intra] = qp
        units.append((intra, qp, reset, payload))
        if log is not None:
            log.append(dict(type="I" if intra else "P", qp=qp, trials=len(trace), trace=trace))
        idx += 1 if intra else frames_per_p
    return units


def intra_budget_bits(target_bpp, pixels_per_picture, k, spent_bits):
    """Budget of picture k (0-based) of an all-intra run: what k + 1 pictures may take together minus what the first k
    took, floored at a quarter of one picture's share."""
    share = float(target_bpp) * pixels_per_picture
    return int(math.floor(max(share * (k + 1) - float(spent_bits), share / 4.0)))


def code_sequence_intra_search(frame_count, code_intra, probe_intra, target_bpp, pixels_per_picture, qp_min=0, qp_max=63,
                               log=None, vbv=None, **vbv_hooks):
    """The all-intra loop of dcvc encode --target-bpp (no inter model, or --intra-period 1): picture k gets the largest q_index
    in [qp_min, qp_max] whose predicted stream fits intra_budget_bits(target_bpp, pixels, k, bits spent), by
    pick_qp_for_budget on probe_intra(frame_idx, qp) -> predicted bits, then one code_intra(frame_idx, qp) -> bytes-like.
    `log`, a list, receives per picture {type, qp, probes, predicted_bits, budget_bits, trace}. vbv, a Vbv: the search runs on
    min(that budget, the buffer's payload budget) and the picture is fitted into the decoder buffer (vbv_fit)
    with floor_q = qp_min; **vbv_hooks as code_sequence_capped takes them (probe_intra is this function's). Returns what
    code_sequence returns."""
    if vbv is not None:
        state = dict(spent=0)

        def q_mode(intra, idx, n, payload_avail):
            own = intra_budget_bits(target_bpp, pixels_per_picture, idx, state["spent"])
            trace = []
            qp = pick_qp_for_budget(lambda q: probe_intra(idx, q), min(own, payload_avail), qp_min, qp_max, trace=trace)
            return qp, len(trace), dict(trace)[qp], vbv_searched_qp_mode(qp, trace, own)

        def book(intra, qp, payload, n):
            state["spent"] += 8 * len(payload)

        return code_sequence_capped(frame_count, 1, code_intra, None, vbv, q_mode, book, floor_q=qp_min, force_intra=True,
                                    probe_intra=probe_intra, **vbv_hooks)
    units, spent = [], 0
    for k in range(frame_count):
        budget = intra_budget_bits(target_bpp, pixels_per_picture, k, spent)
        trace = []
        qp = pick_qp_for_budget(lambda q: probe_intra(k, q), budget, qp_min, qp_max, trace=trace)
        payload = code_intra(k, qp)
        spent += 8 * len(payload)
        units.append((True, qp, False, payload))
        if log is not None:
            log.append(dict(type="I", qp=qp, probes=len(trace), predicted_bits=dict(trace)[qp], budget_bits=budget, trace=trace))
    return units


# ---- coding under a decoder-buffer cap. The native tool has the same model (csrc/codec/rate_control.cpp,
# dcvc_rc_vbv_*) and the same procedure (dcvc encode --vbv-maxrate / --vbv-bufsize); the tests hold them against each other.

class Vbv:
    """Decoder-buffer model: a bucket of `capacity` = bufsize_pictures * rate bits that fills with `rate` = maxrate_bpp *
    pixels_per_picture bits per picture period and starts at init * capacity. All in IEEE double, in the operation order of
    include/dcvc_amd_rc.h; `fullness` compares with == against dcvc_rc_vbv_fullness.

    A unit's bits are 8 times every byte it adds to the output (container header, payload, a parameter set in front of it);
    it holds `pictures` source pictures and must be whole in the buffer when the first of them is due."""

    def __init__(self, maxrate_bpp, bufsize_pictures, pixels_per_picture, init=0.9):
        maxrate_bpp, bufsize_pictures, init = float(maxrate_bpp), float(bufsize_pictures), float(init)
        if not (math.isfinite(maxrate_bpp) and maxrate_bpp > 0):
            raise ValueError("vbv: maxrate must be a positive number of bits per pixel")
        if not (math.isfinite(bufsize_pictures) and bufsize_pictures > 0):
            raise ValueError("vbv: bufsize must be a positive number of picture periods")
        if not (math.isfinite(init) and 0 < init <= 1):
            raise ValueError("vbv: init must be in (0, 1] (a fraction of the capacity)")
        if int(pixels_per_picture) != pixels_per_picture or pixels_per_picture < 1:
            raise ValueError("vbv: pixels must be a whole number, at least 1")
        self.rate = maxrate_bpp * float(int(pixels_per_picture))
        self.capacity = bufsize_pictures * self.rate
        if not self.capacity < 2.0 ** 62:
            raise ValueError("vbv: the capacity must be below 2^62 bits")
        self.fullness = init * self.capacity
        self.underflow = 0

    def available_bits(self):
        """avail = floor(fullness): the bits the next unit may take"""
        return int(math.floor(self.fullness))

    def admit(self, bits, pictures):
        """The unit took `bits` for `pictures` source pictures -> 0: it conforms (bits <= avail), fullness = min(capacity,
        (fullness - bits) + pictures * rate); 1: a violation, underflow = bits - avail, fullness = min(capacity, max(0.0,
        fullness - bits) + pictures * rate). Nothing is padded at the top."""
        if int(bits) != bits or int(pictures) != pictures or bits < 0 or pictures < 1:
            raise ValueError("vbv: a unit has bits >= 0 and at least 1 picture")
        bits, pictures = int(bits), int(pictures)
        avail = self.available_bits()
        refill = float(pictures) * self.rate
        left = self.fullness - float(bits)
        if bits <= avail:
            self.underflow = 0
            self.fullness = min(self.capacity, left + refill)
            return 0
        self.underflow = bits - avail
        self.fullness = min(self.capacity, max(0.0, left) + refill)
        return 1


def vbv_replay(units, maxrate_bpp, bufsize_pictures, pixels_per_picture, init=0.9):
    """The model run over units = [(bits, pictures)] in coding order -> (fullness, slack, violations): fullness[i] in front of
    unit i and fullness[len(units)] behind the last; slack = the minimum over the units of avail - bits (negative: a unit did
    not fit; None without units); violations = [(i, underflow_bits)]."""
    vbv = Vbv(maxrate_bpp, bufsize_pictures, pixels_per_picture, init)
    fullness, slack, violations = [vbv.fullness], None, []
    for i, (bits, pictures) in enumerate(units):
        room = vbv.available_bits() - int(bits)
        slack = room if slack is None else min(slack, room)
        if vbv.admit(bits, pictures):
            violations.append((i, vbv.underflow))
        fullness.append(vbv.fullness)
    return fullness, slack, violations


MAX_PAYLOAD_BYTES = (1 << 30) - 1       # the container's length field (stream_helper.write_uint_adaptive)


def vbv_payload_budget(avail, overhead):
    """Bits a payload may take so that the unit fits `avail`: avail - 8 overhead(avail // 8), overhead(payload_bytes) ->
    container bytes around a payload of that length (stream_helper.unit_overhead). A payload that fits avail is at most
    avail // 8 bytes long and the overhead never shrinks with the length, so its own overhead is at most the one taken off:
    8 (len + overhead(len)) <= avail for every payload with 8 len <= the result."""
    avail = int(avail)
    return avail - 8 * overhead(min(max(avail, 0) // 8, MAX_PAYLOAD_BYTES))


def vbv_searched_qp_mode(qp, trace, own_budget_bits):
    """qp_mode of a unit whose rate mode searched on min(its own budget, the buffer's payload budget) and found qp: the largest
    probed q_index whose prediction fits the mode's own budget. The mode's own answer when the cap does not bind; when it
    does, a lower bound of it - how much higher the mode would have gone is not worth a probe."""
    return max([q for q, bits in trace if bits <= own_budget_bits] + [qp])


def vbv_fit(vbv, pictures, q_mode, floor_q, code, probe, overhead, restore=None, mode_probes=0, mode_predicted_bits=None, qp_mode=None):
    """One unit under the cap: coded at q_mode; accepted when it conforms - no probe, nothing else. On a miss:
    restore(); q = pick_qp_near(probe, payload budget, start = q_mode - 1, qp_min = floor_q, qp_max = q_mode - 1); code at q;
    while it still does not conform and q > floor_q: restore(), q -= 1, code again (the coder may exceed the prediction). At
    floor_q a unit that does not conform is kept and counts as a violation. Then vbv.admit.

    code(qp) -> bytes-like payload                 probe(qp) -> predicted payload bits, the codec's state untouched
    overhead(payload_bytes) -> container bytes     restore() puts the state in front of the unit back (a P unit; None: an I
                                                   picture has none)
    mode_probes / mode_predicted_bits: what the rate mode's own search spent on q_mode and predicted for it.
    qp_mode: what the log calls qp_mode when the mode's search was already held under the cap (vbv_searched_qp_mode); None: q_mode.
    Returns {qp_mode, qp, probes, recodes, predicted_bits | None, payload, bytes, fullness_before, fullness_after, violated,
    underflow_bits}; bytes = len(payload) + overhead, what the model counted."""
    before, avail = vbv.fullness, vbv.available_bits()
    qp, probes, recodes, predicted = int(q_mode), int(mode_probes), 0, mode_predicted_bits

    def unit_bytes(payload):
        return len(payload) + overhead(len(payload))

    payload = code(qp)
    if 8 * unit_bytes(payload) > avail and qp > floor_q:
        if restore is not None:
            restore()
        trace = []
        qp = pick_qp_near(probe, vbv_payload_budget(avail, overhead), qp - 1, floor_q, qp - 1, trace=trace)
        probes += len(trace)
        predicted = dict(trace)[qp]
        payload = code(qp)
        recodes += 1
        while 8 * unit_bytes(payload) > avail and qp > floor_q:
            if restore is not None:
                restore()
            qp -= 1
            predicted = dict(trace).get(qp)
            payload = code(qp)
            recodes += 1
    nbytes = unit_bytes(payload)
    violated = vbv.admit(8 * nbytes, pictures)
    return dict(qp_mode=int(q_mode if qp_mode is None else qp_mode), qp=qp, probes=probes, recodes=recodes, predicted_bits=predicted, payload=payload, bytes=nbytes,
                fullness_before=before, fullness_after=vbv.fullness, violated=bool(violated), underflow_bits=vbv.underflow)


def code_sequence_capped(frame_count, frames_per_p, code_intra, code_inter, vbv, q_mode, book, floor_q=0, intra_period=-1,
                         reset_interval=32, force_intra=False, intra_at=None, probe_intra=None, probe_inter=None, snapshot=None,
                         restore=None, accept=None, picture_size=None, vbv_log=None):
    """The loop of code_sequence with every unit fitted into the decoder buffer `vbv`; code_sequence,
    code_sequence_probed and code_sequence_intra_search run it when they are given vbv=.

    q_mode(is_intra, frame_idx, n, payload_avail) -> (qp, probes, predicted_bits | None, qp_mode | None): what the rate mode
                                    gives for the unit; a mode that searches on a budget takes min(its budget, payload_avail)
                                    and says with qp_mode what its own budget would have allowed (vbv_searched_qp_mode)
    book(is_intra, qp, payload, n)  the mode's book-keeping, with the final q_index and payload
    probe_intra(frame_idx, qp), probe_inter(frame_idx, n, qp) -> predicted payload bits, for the search behind a miss
    snapshot()                      in front of every P unit: keep the inter codec's state (export_state)
    restore()                       put it back (import_state), before every coding of the unit after the first
    accept(is_intra, frame_idx, qp) optional, after the unit's last coding: what must follow an accepted unit only (an I
                                    picture's add_ref_feature_from_frame) - code_intra may run several times here
    picture_size = (height, width)  of the coded pictures: the first unit has a parameter set in front
    vbv_log, a list, receives per unit {type, first_picture, pictures, qp_mode, qp, probes, recodes, predicted_bytes | None,
    bytes, fullness_before, fullness_after, violated, underflow_bits}. Returns what code_sequence returns."""
    from . import stream_helper
    if picture_size is None:
        raise ValueError("vbv: picture_size = (height, width) is needed, the first unit carries the parameter set")
    sps = dict(height=int(picture_size[0]), width=int(picture_size[1]))
    units, idx = [], 0
    while idx < frame_count:
        intra = idx == 0 or force_intra or intra_period == 1 or (intra_period > 1 and idx != 1 and idx % intra_period == 1)
        if intra_at is not None:
            intra = bool(intra_at(idx, intra))
        n = 1 if intra else min(frames_per_p, frame_count - idx)
        reset = (not intra) and reset_interval > 0 and (idx + frames_per_p) % reset_interval == 1
        first = not units

        def overhead(payload_bytes):
            return stream_helper.unit_overhead(payload_bytes, sps if first else None)

        qp, probes, predicted, qp_mode = q_mode(intra, idx, n, vbv_payload_budget(vbv.available_bits(), overhead))
        if intra:
            fit = vbv_fit(vbv, 1, qp, floor_q, lambda q: code_intra(idx, q), lambda q: probe_intra(idx, q), overhead, None,
                          probes, predicted, qp_mode)
        else:
            snapshot()
            fit = vbv_fit(vbv, n, qp, floor_q, lambda q: code_inter(idx, n, q, reset), lambda q: probe_inter(idx, n, q), overhead,
                          restore, probes, predicted, qp_mode)
        if accept is not None:
            accept(intra, idx, fit["qp"])
        book(intra, fit["qp"], fit["payload"], n)
        units.append((intra, fit["qp"], reset, fit["payload"]))
        if vbv_log is not None:
            entry = dict(type="I" if intra else "P", first_picture=idx, pictures=n)
            entry.update({k: fit[k] for k in ("qp_mode", "qp", "probes", "recodes", "bytes", "fullness_before", "fullness_after",
                                              "violated", "underflow_bits")})
            entry["predicted_bytes"] = None if fit["predicted_bits"] is None else fit["predicted_bits"] // 8
            vbv_log.append(entry)
        idx += 1 if intra else frames_per_p
    return units
