"""Black-bar cropping of DESIGN.md 30 without a GPU: the decision dcvc_cropdet_* through ctypes against dcvc_amd.crop.CropDetect
and against the numpy restatement (tests/crop_np.py), and what the rule does on letterboxed and pillarboxed synthetic clips.

The clips: 64 rows of 96 samples and 66 rows of 98, at 8 and 10 bits, content of 60..180 code values inside bars of limited-range
black (16), Gaussian noise of sigma 2 code values on bars and content alike, 8 pictures of which the first is all black. With the
tool's defaults (limit 24, frac 4, min_bar 8) and YUV420's alignment (2, 2) the window is the true rectangle with every bar
below 8 dropped and the others rounded down to even, and the black picture casts no vote. A bar sample passes the limit only
4 sigma out; a bar row of 96 samples would need 2 of them to become active. The seeds are pinned."""
import ctypes

import numpy as np
import pytest

import crop_np as cnp
from dcvc_amd import _lib
from dcvc_amd.crop import CropDetect

_vp, _ci = ctypes.c_void_p, ctypes.c_int
_u32p = ctypes.POINTER(ctypes.c_uint32)


class CDet:
    """dcvc_cropdet_* through ctypes"""

    def __init__(self, H, W, frac, min_bar, ax, ay):
        create = _lib.fn("dcvc_cropdet_create", _vp, [_ci] * 6)
        self.h = create(H, W, frac, min_bar, ax, ay)
        self.n = H + W

    def ok(self):
        return bool(self.h)

    def push(self, counts):
        f = _lib.fn("dcvc_cropdet_push", _ci, [_vp, _u32p])
        if counts is None:
            return f(self.h, None)
        arr = (ctypes.c_uint32 * self.n)(*[int(v) for v in counts])
        return f(self.h, arr)

    def result(self):
        f = _lib.fn("dcvc_cropdet_result", _ci, [_vp] + [ctypes.POINTER(_ci)] * 4)
        x, y, w, h = _ci(-1), _ci(-1), _ci(-1), _ci(-1)
        votes = f(self.h, ctypes.byref(x), ctypes.byref(y), ctypes.byref(w), ctypes.byref(h))
        return x.value, y.value, w.value, h.value, votes

    def __del__(self):
        if self.h:
            _lib.fn("dcvc_cropdet_destroy", None, [_vp])(self.h)


def _three(H, W, frac, min_bar, ax, ay, pictures):
    """the three statements of the decision on the same pictures -> the one result, after asserting they agree"""
    c, p = CDet(H, W, frac, min_bar, ax, ay), CropDetect(H, W, frac, min_bar, ax, ay)
    assert c.ok()
    for i, m in enumerate(pictures):
        voted = cnp.picture_vote(m, H, W, frac) is not None
        assert c.push(m) == (1 if voted else 0), i
        assert p.push(m) is voted, i
        assert c.result() == p.result() == cnp.crop_window(pictures[:i + 1], H, W, frac, min_bar, ax, ay), i
    return c.result()


def _counts(H, W, rows, cols):
    m = np.zeros(H + W, dtype=np.int64)
    m[:H], m[H:] = rows, cols
    return m


@pytest.mark.parametrize("ax", [1, 2, 4])
@pytest.mark.parametrize("ay", [1, 2, 4])
def test_random_counts(ax, ay):
    rng = np.random.default_rng(30 + 4 * ax + ay)
    for trial in range(12):
        H, W = int(rng.integers(1, 20)) * 4, int(rng.integers(1, 24)) * 4
        frac, min_bar = int(rng.integers(0, 256)), int(rng.integers(0, 12))
        pictures = []
        for _ in range(int(rng.integers(1, 6))):
            # sparse and dense pictures, bars of random sizes, some pictures blank
            rows, cols = rng.integers(0, W + 1, H), rng.integers(0, H + 1, W)
            t, b, l, r = (int(v) for v in rng.integers(0, 14, 4))
            rows[:min(t, H)] = 0
            rows[max(H - b, 0):] = 0
            cols[:min(l, W)] = 0
            cols[max(W - r, 0):] = 0
            if rng.integers(0, 4) == 0:
                rows[:] = 0
            pictures.append(_counts(H, W, rows, cols))
        x, y, w, h, votes = _three(H, W, frac, min_bar, ax, ay, pictures)
        assert x % ax == 0 and y % ay == 0 and (W - x - w) % ax == 0 and (H - y - h) % ay == 0
        assert w >= 1 and h >= 1 and 0 <= votes <= len(pictures)


def test_a_tie_is_not_active():
    H, W, frac = 32, 64, 4
    # W * frac = 256: a row count of 1 ties (1 * 256 == 256), 2 is active; H * frac = 128: a column count of 0 never is, 1 is
    tie = _counts(H, W, np.r_[np.zeros(8), np.ones(16), np.zeros(8)], np.ones(W))
    assert _three(H, W, frac, 0, 1, 1, [tie]) == (0, 0, W, H, 0)
    over = tie.copy()
    over[8:24] = 2
    assert _three(H, W, frac, 0, 1, 1, [over]) == (0, 8, W, 16, 1)
    # the column rule has its own product: H * frac = 32 * 8 = 256
    cols = np.r_[np.zeros(10), np.ones(40), np.zeros(14)]
    tie_c = _counts(H, W, np.full(H, W), cols)
    assert _three(H, W, 8, 0, 1, 1, [tie_c]) == (0, 0, W, H, 0)
    assert _three(H, W, 8, 0, 1, 1, [_counts(H, W, np.full(H, W), 2 * cols)]) == (10, 0, 40, H, 1)
    # frac 0: any sample above the limit makes its row and column active
    assert _three(H, W, 0, 0, 1, 1, [_counts(H, W, np.r_[np.zeros(31), 1], np.r_[1, np.zeros(63)])]) == (0, 31, 1, 1, 1)


def _boxed(H, W, t, b, l, r):
    rows, cols = np.zeros(H), np.zeros(W)
    rows[t:H - b] = W - l - r
    cols[l:W - r] = H - t - b
    return _counts(H, W, rows, cols)


def test_blank_pictures_between_voting_ones_and_the_union():
    H, W = 48, 64
    blank = _counts(H, W, np.zeros(H), np.zeros(W))
    only_rows = _counts(H, W, np.full(H, W), np.zeros(W))      # active rows but no active column: no vote
    pictures = [blank, _boxed(H, W, 12, 10, 20, 18), blank, only_rows, _boxed(H, W, 10, 14, 16, 22), blank]
    assert _three(H, W, 4, 8, 1, 1, pictures) == (16, 10, W - 16 - 18, H - 10 - 10, 2)
    assert _three(H, W, 4, 8, 2, 2, [blank, blank]) == (0, 0, W, H, 0)


@pytest.mark.parametrize("bar,kept", [(7, 0), (8, 8), (9, 9)])
def test_min_bar_edges(bar, kept):
    H, W = 64, 96
    for side in range(4):
        bars = [0, 0, 0, 0]
        bars[side] = bar
        t, b, l, r = bars
        k = [0, 0, 0, 0]
        k[side] = kept
        assert _three(H, W, 4, 8, 1, 1, [_boxed(H, W, t, b, l, r)]) == (k[2], k[0], W - k[2] - k[3], H - k[0] - k[1], 1)
        # ... and rounded down, never up: 9 -> 8 at an alignment of 2, 4 or (7: dropped first) 0
        for a in (2, 4):
            k[side] = kept - kept % a
            assert _three(H, W, 4, 8, a, a, [_boxed(H, W, t, b, l, r)]) == (k[2], k[0], W - k[2] - k[3], H - k[0] - k[1], 1)


def test_min_bar_0_keeps_a_bar_of_one_and_rounding_can_still_drop_it():
    H, W = 16, 16
    assert _three(H, W, 4, 0, 1, 1, [_boxed(H, W, 1, 0, 0, 3)]) == (0, 1, 13, 15, 1)
    assert _three(H, W, 4, 0, 2, 2, [_boxed(H, W, 1, 0, 0, 3)]) == (0, 0, 14, 16, 1)
    assert _three(H, W, 4, 0, 4, 1, [_boxed(H, W, 1, 0, 0, 3)]) == (0, 1, 16, 15, 1)


CREATE_REFUSED = [
    ("H = 0", (0, 64, 4, 8, 2, 2), "H and W must be in 1..16384"),
    ("H = 16386", (16386, 64, 4, 8, 2, 2), "H and W must be in 1..16384"),
    ("W = 0", (64, 0, 4, 8, 2, 2), "H and W must be in 1..16384"),
    ("W = 16388", (64, 16388, 4, 8, 2, 2), "H and W must be in 1..16384"),
    ("frac = -1", (64, 64, -1, 8, 2, 2), "frac must be in 0..255"),
    ("frac = 256", (64, 64, 256, 8, 2, 2), "frac must be in 0..255"),
    ("min_bar = -1", (64, 64, 4, -1, 2, 2), "min_bar must be in 0..4096"),
    ("min_bar = 4097", (64, 64, 4, 4097, 2, 2), "min_bar must be in 0..4096"),
    ("ax = 0", (64, 64, 4, 8, 0, 2), "ax and ay must be 1, 2 or 4"),
    ("ax = 3", (66, 66, 4, 8, 3, 2), "ax and ay must be 1, 2 or 4"),
    ("ay = 8", (64, 64, 4, 8, 2, 8), "ax and ay must be 1, 2 or 4"),
    ("ay = -2", (64, 64, 4, 8, 2, -2), "ax and ay must be 1, 2 or 4"),
    ("H not a multiple of ay", (66, 64, 4, 8, 2, 4), "H must be a multiple of ay and W of ax"),
    ("W not a multiple of ax", (64, 63, 4, 8, 2, 1), "H must be a multiple of ay and W of ax"),
]


@pytest.mark.parametrize("why,args,words", CREATE_REFUSED, ids=[r[0].replace(" ", "_") for r in CREATE_REFUSED])
def test_create_refuses(why, args, words):
    assert not CDet(*args).ok(), why
    assert words in _lib.lib().dcvc_last_error().decode()
    with pytest.raises(ValueError, match=words.replace("(", r"\(").replace(")", r"\)")):
        CropDetect(*args)


def test_the_largest_parameters_are_taken():
    assert CDet(16384, 16384, 255, 4096, 4, 4).ok() and CDet(1, 1, 0, 0, 1, 1).ok()
    CropDetect(16384, 16384, 255, 4096, 4, 4)


def test_a_refused_push_changes_nothing():
    H, W = 32, 48
    c, p = CDet(H, W, 4, 8, 2, 2), CropDetect(H, W, 4, 8, 2, 2)
    good = _boxed(H, W, 8, 8, 0, 0)
    assert c.push(good) == 1 and p.push(good) is True
    before = c.result()
    assert before == p.result() == (0, 8, W, 16, 1)
    row_over, col_over = _boxed(H, W, 0, 0, 0, 0), _boxed(H, W, 0, 0, 0, 0)
    row_over[3] = W + 1
    col_over[H + 5] = H + 1
    for bad, words in ((row_over, "a row count is above the width"), (col_over, "a column count is above the height")):
        assert c.push(bad) < 0
        assert words in _lib.lib().dcvc_last_error().decode()
        with pytest.raises(ValueError, match=words):
            p.push(bad)
        assert c.result() == p.result() == before
    assert c.push(None) < 0 and "null words" in _lib.lib().dcvc_last_error().decode()
    with pytest.raises(ValueError, match="words expected"):
        p.push(good[:-1])
    assert c.result() == p.result() == before
    # a count AT the side is taken
    assert c.push(_boxed(H, W, 0, 0, 0, 0)) == 1 and c.result() == (0, 0, W, H, 2)


def test_null_handles_and_results_are_refused():
    push = _lib.fn("dcvc_cropdet_push", _ci, [_vp, _u32p])
    assert push(None, (ctypes.c_uint32 * 4)()) < 0
    result = _lib.fn("dcvc_cropdet_result", _ci, [_vp] + [ctypes.POINTER(_ci)] * 4)
    v = _ci()
    assert result(None, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) < 0
    c = CDet(8, 8, 4, 0, 1, 1)
    assert result(c.h, None, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) < 0
    _lib.fn("dcvc_cropdet_destroy", None, [_vp])(None)


# ---------------------------------------------------------------- what it does
LIMIT, FRAC, MIN_BAR, PICTURES, SIGMA = 24, 4, 8, 8, 2.0
BARS = [(12, 12, 0, 0), (0, 0, 16, 16), (10, 14, 6, 8)]         # top, bottom, left, right
SIZES = [(64, 96), (66, 98)]
SEEDS = {8: 3001, 10: 3002}


def _clip(H, W, bars, bits):
    """8 luma planes: limited-range black bars around content of 60..180 code values that moves, sigma 2 noise everywhere; the
    first picture is all black"""
    t, b, l, r = bars
    sh = bits - 8
    rng = np.random.default_rng(SEEDS[bits] + 17 * H + bars[0] + bars[2])
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for n in range(PICTURES):
        pic = np.full((H, W), 16.0)
        if n > 0:
            content = 120 + 60 * np.sin((x + 3 * n) / 9) * np.cos(y / 7)
            pic[t:H - b, l:W - r] = content[t:H - b, l:W - r]
        pic = (pic + rng.normal(0, SIGMA, (H, W))) * (1 << sh)
        out.append(np.clip(np.round(pic), 0, (1 << bits) - 1).astype(np.uint8 if bits == 8 else np.uint16))
    return out


def _rounded(bars, ax, ay):
    t, b, l, r = bars
    return [0 if v < MIN_BAR else v // a * a for v, a in ((t, ay), (b, ay), (l, ax), (r, ax))]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("bars", BARS)
def test_the_window_is_the_true_rectangle(bars, H, W, bits):
    clip = _clip(H, W, bars, bits)
    counts = [cnp.crop_stats(p, LIMIT, bits) for p in clip]
    assert cnp.picture_vote(counts[0], H, W, FRAC) is None                      # the black picture
    assert all(cnp.picture_vote(c, H, W, FRAC) is not None for c in counts[1:])
    T, B, L, R = _rounded(bars, 2, 2)
    assert cnp.crop_window(counts, H, W, FRAC, MIN_BAR, 2, 2) == (L, T, W - L - R, H - T - B, PICTURES - 1)
    # the host code and its Python twin on the same words
    assert _three(H, W, FRAC, MIN_BAR, 2, 2, counts) == (L, T, W - L - R, H - T - B, PICTURES - 1)
    # the content is never cut: at 4:4:4's alignment the window is the truth with the bars below min_bar given back
    T1, B1, L1, R1 = _rounded(bars, 1, 1)
    assert cnp.crop_window(counts, H, W, FRAC, MIN_BAR, 1, 1) == (L1, T1, W - L1 - R1, H - T1 - B1, PICTURES - 1)
    # the largest count of a bar row or column stays below what would make it active
    t, b, l, r = bars
    for c in counts:
        bar_rows = np.r_[c[:t], c[H - b:H]]
        bar_cols = np.r_[c[H:H + l], c[H + W - r:]]
        assert bar_rows.size == 0 or bar_rows.max() * 256 <= W * FRAC
        assert bar_cols.size == 0 or bar_cols.max() * 256 <= H * FRAC


def test_the_restatements_window_copy():
    src = np.arange(2 * 5 * 7, dtype=np.uint16).reshape(2, 5, 7)
    crop = cnp.window_planes(src, 3, 4, 2, 1, [9, 8])
    assert np.array_equal(crop, src[:, 1:4, 2:6])
    pad = cnp.window_planes(crop, 5, 7, -2, -1, [9, 8])
    want = np.empty_like(src)
    want[0], want[1] = 9, 8
    want[:, 1:4, 2:6] = src[:, 1:4, 2:6]
    assert np.array_equal(pad, want)
    # hanging over all four sides
    over = cnp.window_planes(src[:1], 9, 11, -2, -3, 77)
    assert np.array_equal(over[0, 3:8, 2:9], src[0]) and (over[0, :3] == 77).all() and (over[0, 8:] == 77).all()
    assert (over[0, :, :2] == 77).all() and (over[0, :, 9:] == 77).all()


def test_probe_indexes_spread_over_the_clip():
    assert cnp.probe_indexes(16, 8) == list(range(8))
    assert cnp.probe_indexes(4, 100) == [12, 37, 62, 87]
    assert cnp.probe_indexes(1, 9) == [4]
    assert cnp.probe_indexes(16, 1) == [0]
