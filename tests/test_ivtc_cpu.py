"""Inverse telecine of DESIGN.md 28 without a GPU: the numpy restatement (tests/ivtc_np.py) and the decisions (dcvc_amd.ivtc.Ivtc
against dcvc_ivtc_* through ctypes) on a synthetic film clip carried by 2:3 pulldown - the scene of test_deinterlace_cpu.py moving
3 samples per FILM frame, 64 rows of 96 samples, at 8 and 10 bits, both field orders and all five cadence phases.

Noiseless, the output is the film, bit for bit, but for a first frame whose partner field lies before the clip (flagged combed and
deinterlaced); the matches follow c c p p c; every complete cycle that holds a repeated first field drops exactly it. With
Gaussian noise of sigma 2 on every field the flags and the drops are the same. True video - every field with a time of its own -
is flagged in every frame. A clip that starts in mid-cadence on the repeat loses one real frame in its first cycle: the cycle grid
is fixed from frame 0 (documented behaviour, pinned below)."""
import ctypes

import numpy as np
import pytest

import ivtc_np as inp
from dcvc_amd import _lib
from dcvc_amd.ivtc import Ivtc

SH, SW, FILM = 64, 96, 12
PATTERN = "ccppc"
_vp, _ci = ctypes.c_void_p, ctypes.c_int


def _truth(n, speed, bits):
    """test_deinterlace_cpu.py's progressive scene at time n: x' = x + speed n"""
    y, x = np.mgrid[0:SH, 0:SW]
    x = x + speed * n
    v = 128 + 60 * np.sin(x / 9) * np.cos(y / 7) + 40 * ((x // 16 + y // 16) % 2) - 20 + 30 * np.sin((x + y) / 3)
    return np.clip(np.round(v * (1 << (bits - 8))), 0, (1 << bits) - 1)


def _dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


_clips = {}


def _clip(bits, order, phase, sigma=0.0):
    """-> (frames as 1-tuples of a luma plane, the film picture of every frame's first field, of its second, the film)"""
    key = (bits, order, phase, sigma)
    if key not in _clips:
        film = [(_truth(k, 3, bits).astype(_dtype(bits)),) for k in range(FILM)]
        rng = np.random.default_rng(28)

        def seen(i, k):
            noisy = film[k][0] + rng.normal(0, sigma * (1 << (bits - 8)), (SH, SW))
            return (np.clip(np.round(noisy), 0, (1 << bits) - 1).astype(_dtype(bits)),)

        tc = inp.telecine(film, order, phase, seen if sigma else None)
        _clips[key] = ([f for f, _, _ in tc], [ka for _, ka, _ in tc], [kb for _, _, kb in tc], film)
    return _clips[key]


def _orphan(phase):
    """the clip's first frame holds fields of two film pictures, and the first field's partner lies before the clip"""
    return PATTERN[phase % 5] == "p"


def _repeat(i, phase):
    """frame i of the clip repeats the first field of frame i - 1"""
    return i > 0 and (i + phase) % 5 == 2


CASES = [(bits, order, phase) for bits in (8, 10) for order in ("tff", "bff") for phase in range(5)]


@pytest.mark.parametrize("bits,order,phase", CASES)
def test_matching_gives_back_the_film(bits, order, phase):
    frames, ka, kb, film = _clip(bits, order, phase)
    assert len(frames) == 15 - phase
    pics, log = inp.ivtc_clip(frames, "match", order, bits)
    assert len(pics) == len(frames) == len(log) and not any(e["dropped"] for e in log)
    for i, (pic, e) in enumerate(zip(pics, log)):
        if i == 0 and _orphan(phase):
            assert e["combed"] and e["match"] == "c"              # no partner in the clip: deinterlaced
            assert not np.array_equal(pic[0], film[ka[i]][0])
            continue
        assert not e["combed"], (i, e)
        assert e["match"] == PATTERN[(i + phase) % 5], (i, e)
        assert np.array_equal(pic[0], film[ka[i]][0]) and pic[0].dtype == _dtype(bits)
    # the clip itself is combed: two frames in five are woven from two film pictures
    assert sum(not np.array_equal(f[0], film[a][0]) for f, a in zip(frames, ka)) == sum(a != b for a, b in zip(ka, kb)) >= 4


def _drops(log):
    return [i for i, e in enumerate(log) if e["dropped"]]


@pytest.mark.parametrize("bits,order,phase", CASES)
def test_film_mode_drops_the_repeated_first_field(bits, order, phase):
    frames, ka, _, film = _clip(bits, order, phase)
    pics, log = inp.ivtc_clip(frames, "film", order, bits)
    M = len(frames)
    assert len(pics) == 4 * (M // 5) + M % 5 and len(log) == M
    drops = _drops(log)
    assert len(drops) == M // 5 and all(d // 5 == c for c, d in enumerate(drops))         # one in every complete cycle, none in a ragged one
    for c, d in enumerate(drops):
        repeats = [i for i in range(5 * c, 5 * c + 5) if _repeat(i, phase)]
        if repeats:
            assert [d] == repeats
            assert log[d]["words"][6] == 0                       # dup of a noiseless repeat
    kept = [i for i in range(M) if i not in drops]
    for pic, i in zip(pics, kept):
        if i == 0 and _orphan(phase):
            continue
        assert np.array_equal(pic[0], film[ka[i]][0])
    if phase != 2:
        # every film picture the complete cycles hold a first field of comes out exactly once (a ragged last cycle keeps its repeat)
        whole = 5 * (M // 5)
        assert [ka[i] for i in kept if i < whole] == sorted(set(ka[:whole]))


@pytest.mark.parametrize("order", ["tff", "bff"])
def test_a_clip_cut_on_the_repeat_loses_a_real_frame_in_its_first_cycle(order):
    """phase 2: frame 0 repeats the first field of a frame that is not in the clip; it has no dup, the first cycle holds five
    different film pictures, and the fixed cycle grid still drops one of them. Later cycles are right again."""
    frames, ka, _, _ = _clip(8, order, 2)
    pics, log = inp.ivtc_clip(frames, "film", order, 8)
    drops = _drops(log)
    assert len(set(ka[:5])) == 5 and len(drops) == 2
    assert 1 <= drops[0] <= 4 and not _repeat(drops[0], 2)
    assert log[drops[0]]["words"][6] > 0 and _repeat(drops[1], 2) and log[drops[1]]["words"][6] == 0
    assert ka[drops[0]] not in [ka[i] for i in range(len(frames)) if i not in drops]          # that film picture is lost


@pytest.mark.parametrize("bits,order,phase", CASES)
def test_noise_changes_neither_the_flags_nor_the_drops(bits, order, phase):
    clean, _, _, _ = _clip(bits, order, phase)
    noisy, _, _, _ = _clip(bits, order, phase, sigma=2.0)
    _, log0 = inp.ivtc_clip(clean, "film", order, bits)
    _, log = inp.ivtc_clip(noisy, "film", order, bits)
    flagged = [i for i, e in enumerate(log) if e["combed"]]
    assert flagged == ([0] if _orphan(phase) else [])
    if phase != 2:                                               # the first cycle of phase 2 holds no repeat: its drop is arbitrary
        assert _drops(log) == _drops(log0)
    else:
        assert _drops(log)[1:] == _drops(log0)[1:]
    scale = 1 << (bits - 8)
    rep = [e["words"][6] / scale for i, e in enumerate(log) if _repeat(i, phase)]
    other = [e["words"][6] / scale for i, e in enumerate(log) if i > 0 and not _repeat(i, phase)]
    blk = [e["words"][4 + (e["match"] == "p")] for i, e in enumerate(log) if not (i == 0 and _orphan(phase))]
    print("noise %d bits %s phase %d: dup of repeats %.0f..%.0f, of the others %.0f..%.0f, blkmax of matched frames 0..%d"
          % (bits, order, phase, min(rep), max(rep), min(other), max(other), max(blk)))
    assert max(rep) * 4 < min(other) and max(blk) <= 80


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("order", ["tff", "bff"])
def test_true_video_is_flagged_in_every_frame(bits, order):
    first = 0 if order == "tff" else 1
    fields = [_truth(n, 3, bits).astype(_dtype(bits)) for n in range(16)]
    frames = []
    for f in range(8):
        wv = np.empty_like(fields[0])
        wv[first::2], wv[1 - first::2] = fields[2 * f][first::2], fields[2 * f + 1][1 - first::2]
        frames.append((wv,))
    pics, log = inp.ivtc_clip(frames, "match", order, bits)
    blk = [e["words"][4 + (e["match"] == "p")] for e in log]
    print("video %d bits %s: blkmax %d..%d against mi 80" % (bits, order, min(blk), max(blk)))
    assert all(e["combed"] for e in log) and min(blk) > 80
    # a combed frame is what --deinterlace frame gives
    import deinterlace_np as dnp
    want = dnp.deinterlace_clip([f[0] for f in frames], "frame", order, 10, bits)
    assert all(np.array_equal(p[0], w) for p, w in zip(pics, want))


def test_n_ends_inside_a_cycle():
    frames, _, _, _ = _clip(8, "tff", 0)
    full, full_log = inp.ivtc_clip(frames, "film", "tff", 8)
    pics, log = inp.ivtc_clip(frames, "film", "tff", 8, n=6)
    assert len(pics) == 6 and len(log) == 10 and log == full_log[:10]
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(pics, full))
    pics, log = inp.ivtc_clip(frames, "match", "tff", 8, n=3)
    assert len(pics) == 3 and len(log) == 3


# ------------------------------------------------------------------------------------ the measurement's restatement
def _scalar(cur, prev, first, cthresh, bits):
    """the contract, sample by sample in Python integers"""
    H, W = cur.shape
    t, q = cthresh << (bits - 8), 1 - first
    c = [[int(v) for v in row] for row in cur]
    words = [0] * 8
    for w, S in ((0, c), (1, None if prev is None else [[int(v) for v in row] for row in prev])):
        if S is None:
            continue
        blocks = {}
        for y in range(1, H - 1):
            if y % 2 != q:
                continue
            for x in range(W):
                a, b, s = c[y - 1][x], c[y + 1][x], S[y][x]
                words[w] += abs(2 * s - a - b)
                if (s - a > t and s - b > t) or (s - a < -t and s - b < -t):
                    words[2 + w] += 1
                    blocks[(y // 16, x // 32)] = blocks.get((y // 16, x // 32), 0) + 1
        words[4 + w] = max(blocks.values()) if blocks else 0
    if prev is not None:
        words[6] = sum(abs(c[y][x] - int(prev[y][x])) for y in range(first, H, 2) for x in range(W))
    return words


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("shape", [(2, 1), (3, 5), (4, 33), (17, 31), (35, 70)])
def test_the_vectorised_restatement_is_the_scalar_contract(bits, shape):
    rng = np.random.default_rng(5)
    cur = rng.integers(0, 1 << bits, shape).astype(_dtype(bits))
    near = np.clip(cur.astype(np.int64) + rng.integers(-20, 21, shape) * (1 << (bits - 8)), 0, (1 << bits) - 1).astype(_dtype(bits))
    for first in (0, 1):
        for cthresh in (0, 9, 255):
            for prev in (None, near, rng.integers(0, 1 << bits, shape).astype(_dtype(bits))):
                got = inp.field_match(cur, prev, first, cthresh, bits)
                assert got == _scalar(cur, prev, first, cthresh, bits), (first, cthresh)
                assert got[7] == 0 and (prev is not None or got[1] == got[3] == got[5] == got[6] == 0)
    if shape[0] == 2:
        assert inp.field_match(cur, near, 0, 9, bits)[:6] == [0] * 6         # no interior row


def test_weave_fields_takes_rows_by_parity():
    a, b = np.full((5, 3), 1, np.uint8), np.full((5, 3), 2, np.uint8)
    assert inp.weave_fields(a, b, 0)[:, 0].tolist() == [1, 2, 1, 2, 1]
    assert inp.weave_fields(a, b, 1)[:, 0].tolist() == [2, 1, 2, 1, 2]


# ------------------------------------------------------------------------------------ Ivtc against dcvc_ivtc_*
def _c():
    words = ctypes.c_uint64 * 8
    return dict(create=_lib.fn("dcvc_ivtc_create", _vp, [_ci, _ci]), push=_lib.fn("dcvc_ivtc_push", _ci, [_vp, _ci, _ci, ctypes.POINTER(ctypes.c_uint64)]),
                drop=_lib.fn("dcvc_ivtc_drop", _ci, [_vp]), destroy=_lib.fn("dcvc_ivtc_destroy", None, [_vp]), words=words)


def _random_words(rng, ties):
    if ties:
        m = [int(v) for v in rng.integers(0, 3, 8)]
        m[4], m[5] = int(rng.integers(79, 82)), int(rng.integers(79, 82))
    else:
        m = [int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 28)), int(rng.integers(0, 1 << 28)),
             int(rng.integers(0, 257)), int(rng.integers(0, 257)), int(rng.integers(0, 1 << 40)), 0]
    return m


@pytest.mark.parametrize("cycle", [0, 2, 5, 32])
@pytest.mark.parametrize("ties", [False, True])
def test_the_python_twin_is_the_c_object(cycle, ties):
    f = _c()
    rng = np.random.default_rng(100 + cycle)
    for mi in (0, 80, 512):
        h, t = f["create"](cycle, mi), Ivtc(cycle, mi)
        assert h
        assert f["drop"](h) == t.drop() == -1
        drops = []
        for idx in range(3 * max(cycle, 2) + 1):
            m = _random_words(rng, ties)
            has_prev = idx > 0 and not (ties and idx == 3)       # a frame measured alone in mid-clip is never dropped either
            got, want = f["push"](h, idx, int(has_prev), f["words"](*m)), t.push(idx, has_prev, m)
            assert got == want and 0 <= got <= 3
            assert (got & 1) == (1 if has_prev and m[1] < m[0] else 0)
            assert (got >> 1) == (1 if m[4 + (got & 1)] > mi else 0)
            assert f["drop"](h) == t.drop()
            if cycle == 0 or idx % cycle != cycle - 1:
                assert t.drop() == -1
            else:
                drops.append(t.drop())
                assert 0 <= t.drop() < cycle and not (idx < cycle and t.drop() == 0)          # frame 0 is never dropped
        assert len(drops) == (3 if cycle else 0)
        f["destroy"](h)


def test_drop_takes_the_smallest_dup_and_the_lowest_position_of_a_tie():
    f = _c()
    for dups, want in (([9, 5, 7, 5, 8], 1), ([0, 5, 5, 5, 5], 1), ([1, 9, 9, 9, 1], 4), ([9, 8, 7, 6, 6], 3)):
        h, t = f["create"](5, 80), Ivtc(5, 80)
        for idx, d in enumerate(dups):
            m = [0, 0, 0, 0, 0, 0, d, 0]
            assert f["push"](h, idx, int(idx > 0), f["words"](*m)) == t.push(idx, idx > 0, m) == 0
        assert f["drop"](h) == t.drop() == want, dups
        # the second cycle: position 0 has a dup now
        for idx, d in enumerate([3, 5, 3, 9, 9]):
            m = [0, 0, 0, 0, 0, 0, d, 0]
            f["push"](h, 5 + idx, 1, f["words"](*m)), t.push(5 + idx, True, m)
            assert f["drop"](h) == t.drop() == (0 if idx == 4 else -1)
        f["destroy"](h)


def test_refusals_leave_the_state_unchanged():
    f = _c()
    for cycle, mi in ((1, 80), (-1, 80), (33, 80), (5, -1), (5, 513)):
        assert not f["create"](cycle, mi)
        assert "ivtc:" in _lib.lib().dcvc_last_error().decode()
        with pytest.raises(ValueError):
            Ivtc(cycle, mi)
    h, t = f["create"](2, 80), Ivtc(2, 80)
    ok = [5, 4, 0, 0, 0, 100, 7, 0]
    big = 16384 * 16384 + 1
    bad = [(1, 0, ok, "frame 1 pushed, 0 is next"), (0, 1, ok, "frame 0 has no previous frame"),
           (0, 0, [0, 0, big, 0, 0, 0, 0, 0], "comb count"), (0, 0, [0, 0, 0, big, 0, 0, 0, 0], "comb count")]
    for idx, has_prev, m, words in bad:
        assert f["push"](h, idx, has_prev, f["words"](*m)) < 0
        assert words in _lib.lib().dcvc_last_error().decode()
        with pytest.raises(ValueError, match=words):
            t.push(idx, has_prev, m)
    assert f["push"](h, 0, 0, f["words"](*ok)) == t.push(0, False, ok) == 0            # still frame 0, and match c without prev
    for idx in (0, 2):
        assert f["push"](h, idx, 1, f["words"](*ok)) < 0
        with pytest.raises(ValueError):
            t.push(idx, True, ok)
    assert f["push"](h, 1, 1, f["words"](*ok)) == t.push(1, True, ok) == 3             # p, and blkmax_p 100 > 80
    assert f["drop"](h) == t.drop() == 1
    assert f["push"](None, 0, 0, f["words"](*ok)) < 0 and f["push"](h, 2, 1, None) < 0
    assert f["drop"](None) == -1
    f["destroy"](h)
