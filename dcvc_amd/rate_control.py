"""Rate-control hook of the coding loop.

The reference harness codes a whole sequence with ONE q_index per rate point (test_video.py:512-514:
`linspace(0, 63, rate_num)`), but its stream container already carries the q_index of every picture
(stream_helper.py:134-135 write_ip / read_ip_remaining), so a decoder needs no side information when the encoder
changes it from picture to picture. This module is the encoder-side hook for that: a controller object the coding
loop asks for the q_index of the next coded unit and tells the bits the unit took, plus `code_sequence`, the
loop of test_video.py:204-257 (picture types, reset rule, chunk padding) with the q_index taken from the
controller instead of a constant. The native tool (csrc/cli/dcvc_cli.hip) codes with the reference's constant
--qp-i / --qp-p unless it is given --target-bpp; then it runs the same controller natively (csrc/codec/rate_control.cpp),
or, in all-intra runs, the budget search at the end of this module on the GPU size probe.

In DCVC-UF a HIGHER q_index means finer quantisation = more bits (q 0 .. 63).
"""
import math


class ConstantQP:
    """The reference behaviour: one q_index for I pictures, one for P units."""

    def __init__(self, qp_i, qp_p=None):
        self.qp_i, self.qp_p = int(qp_i), int(qp_i if qp_p is None else qp_p)

    def next_qp(self, is_intra):
        return self.qp_i if is_intra else self.qp_p

    def update(self, bits, pictures, is_intra):
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

    def update(self, bits, pictures, is_intra):
        if pictures <= 0:
            return
        self.spent += bits
        self.pictures += pictures
        per_picture = max(bits / pictures, 1.0)
        used_qp = self.next_qp(is_intra)
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
        step = (math.log2(want) - math.log2(per_picture)) / self.slope
        self.qp += min(self.max_step, max(-self.max_step, step))           # bounded step: no oscillation with the intra period
        self.qp = min(float(self.qp_max), max(float(self.qp_min), self.qp))

    @property
    def spent_bits_per_picture(self):
        return self.spent / max(self.pictures, 1)


def code_sequence(frame_count, frames_per_p, code_intra, code_inter, controller, intra_period=-1, reset_interval=32,
                  force_intra=False, intra_at=None):
    """The encode loop of test_video.py:204-257 with the q_index from `controller`.

    code_intra(frame_idx, qp) -> bytes-like          one I picture
    code_inter(frame_idx, n, qp, reset) -> bytes-like a P unit of frames_per_p pictures starting at frame_idx, of which
                                                      the first n exist in the source (the caller pads the rest by
                                                      repeating the last picture, test_video.py:104-110)
    intra_at(frame_idx, scheduled) -> bool            optional (dcvc encode --scene-cut, scene.SceneCut.push behind it): asked
                                                      once for every picture a unit starts with, in coding order, with the
                                                      index-based decision; its answer is the picture's type. None: the
                                                      index-based decision stands.
    Returns [(is_intra, qp, reset, payload)] in coding order - what write_ip stores per unit."""
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
                         force_intra=False, log=None, intra_at=None):
    """code_sequence with every P unit's q_index searched on the size probe of the inter model (dcvc encode --rc-mode
    probe): the largest q_index whose predicted stream fits the unit's budget.

    probe_inter(frame_idx, n, qp) -> predicted bits of the P unit code_inter(frame_idx, n, qp, reset) would write; it
    must not advance the temporal state (DMCLDProxy / DMCHT*Proxy.estimate_bits).
    P unit of n existing pictures: pick_qp_near on the probe with the budget unit_budget_bits(...), start = the q_index
    of the previous P unit (qp_i for the first). I picture: start + intra_bonus clamped to the range, not probed; its bits
    count in what is spent. `log`, a list, receives per unit {type, qp, probes, predicted_bits, budget_bits, trace}.
    `intra_at` as in code_sequence. Returns what code_sequence returns."""
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
