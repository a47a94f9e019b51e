"""Film grain of DESIGN.md 29 without a GPU: the numpy restatement (tests/grain_np.py), the Python twins (dcvc_amd.grain
grain_template, grain_fit) and the C host functions (dcvc_grain_template, dcvc_grain_fit through ctypes) held against each other
with ==, the template's statistics, and what the whole chain does on a synthetic scene: a luma ramp under noise whose strength
rises with the luma, through the denoiser's restatement, the measurement, the fit and the synthesis."""
import ctypes

import numpy as np
import pytest

import denoise_np as dnp
import grain_np as gnp
from dcvc_amd import _lib
from dcvc_amd.grain import grain_fit, grain_template

SIZES = [0, 8, 16, 24, 32, 37]
SEEDS = [1234, 7]
_ci, _u32, _ll = ctypes.c_int, ctypes.c_uint32, ctypes.c_longlong


def _c_template(seed, plane, size):
    buf = (ctypes.c_int16 * 4096)()
    rc = _lib.fn("dcvc_grain_template", _ci, [_u32, _ci, _ci, ctypes.c_void_p])(seed, plane, size, buf)
    assert rc == 0, _lib.lib().dcvc_last_error().decode()
    return np.frombuffer(buf, np.int16).reshape(64, 64).copy()


def _c_fit(words, bit_depth, gain, min_count):
    flat = [int(v) for w in words for v in w]
    out = (ctypes.c_uint8 * 27)()
    rc = _lib.fn("dcvc_grain_fit", _ci, [ctypes.c_void_p, _ci, _ci, _ll, ctypes.c_void_p])((ctypes.c_uint64 * 48)(*flat), bit_depth, gain,
                                                                                       min_count, out)
    if rc < 0:
        return None
    return [list(out[9 * p:9 * p + 9]) for p in range(3)]


_templates = {}


def _template(seed, plane, size):
    if (seed, plane, size) not in _templates:
        _templates[(seed, plane, size)] = gnp.template(seed, plane, size)
    return _templates[(seed, plane, size)]


@pytest.mark.parametrize("size", SIZES)
def test_the_c_template_and_the_python_twin_are_the_restatement(size):
    for seed, plane in ((1234, 0), (1234, 2), (0xFFFFFFFF, 1)):
        want = _template(seed, plane, size)
        assert want.dtype == np.int16 and want.shape == (64, 64)
        assert np.array_equal(_c_template(seed, plane, size), want)
        assert grain_template(seed, plane, size) == want.tolist()
        assert np.abs(want.astype(np.int64)).max() <= 1023


def _lag1(T):
    t = T.astype(np.float64) - T.mean()
    return float((t * np.roll(t, -1, axis=1)).sum() / (t * t).sum())


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", SIZES)
def test_the_template_has_a_deviation_of_64_and_the_models_correlation(seed, size):
    T = _template(seed, 0, size)
    a, b = size, 128 - 2 * size
    model = 2 * a * b / (2 * a * a + b * b)
    std, rho = float(T.std()), _lag1(T)
    print("seed %d size %d: std %.2f, max |T| %d, lag-1 %.3f (model %.3f)" % (seed, size, std, np.abs(T).max(), rho, model))
    assert 62 <= std <= 66
    assert abs(rho - model) <= 0.05
    assert abs(_lag1(T.T) - model) <= 0.05          # the vertical pass is the horizontal one


def test_templates_differ_by_seed_and_plane():
    assert not np.array_equal(_template(1234, 0, 16), _template(1234, 2, 16))
    assert not np.array_equal(_template(1234, 0, 16), _template(7, 0, 16))


def test_template_refusals():
    f = _lib.fn("dcvc_grain_template", _ci, [_u32, _ci, _ci, ctypes.c_void_p])
    buf = (ctypes.c_int16 * 4096)()
    for plane, size, words in ((-1, 12, "plane"), (3, 12, "plane"), (0, -1, "size"), (0, 38, "size")):
        assert f(1, plane, size, buf) < 0
        err = _lib.lib().dcvc_last_error().decode()
        assert err.startswith("grain_template:") and words in err, err
        with pytest.raises(ValueError, match=words):
            grain_template(1, plane, size)
        with pytest.raises(ValueError):
            gnp.template(1, plane, size)
    assert f(1, 0, 12, None) < 0 and "null" in _lib.lib().dcvc_last_error().decode()


# ------------------------------------------------------------------------------------ the fit
def _random_words(rng, kind):
    words = []
    for _ in range(3):
        if kind == "plain":
            n = [int(v) for v in rng.integers(0, 1 << 22, 8)]
            S = [int(v * rng.integers(0, 3000)) for v in n]
        elif kind == "empty bins":
            n = [int(v) if rng.random() < 0.5 else int(rng.integers(0, 256)) for v in rng.integers(256, 1 << 20, 8)]
            S = [int(v * rng.integers(0, 400)) for v in n]
        elif kind == "all empty":
            n = [int(v) for v in rng.integers(0, 256, 8)]
            S = [int(v * 100) for v in n]
        elif kind == "ties":
            n = [0] * 8
            for k in rng.choice(8, 2, replace=False):
                n[int(k)] = 1000
            S = [int(v * rng.integers(1, 200)) for v in n]
        elif kind == "clamped":
            n = [int(v) for v in rng.integers(256, 1 << 12, 8)]
            S = [int(v) * int(rng.integers(200, 1 << 30)) for v in n]
        else:                                        # the largest words a window can sum
            n = [int(v) for v in rng.integers(1 << 40, 1 << 56, 8)]
            S = [int(v) for v in rng.integers(1 << 60, (1 << 63) - 1, 8, dtype=np.uint64)]
        words.append(n + S)
    return words


@pytest.mark.parametrize("kind", ["plain", "empty bins", "all empty", "ties", "clamped", "huge"])
def test_the_fit_twin_is_the_c_function(kind):
    rng = np.random.default_rng(29)
    seen = set()
    for trial in range(40):
        words = _random_words(rng, kind)
        bits = int(rng.integers(8, 17)) if kind != "clamped" else 8
        gain = int(rng.integers(1, 401)) if kind != "clamped" else 400
        got, want, twin = _c_fit(words, bits, gain, 256), gnp.fit(words, bits, gain, 256), grain_fit(words, bits, gain, 256)
        assert got == want == twin, (words, bits, gain)
        seen.update(v for t in want for v in t)
    if kind == "all empty":
        assert seen == {0}
    if kind == "clamped":
        assert 255 in seen


def test_an_empty_bin_takes_the_nearest_valid_one_and_a_tie_the_lower():
    def words(valid):
        n = [1000 if k in valid else 255 for k in range(8)]
        return [n + [v * (k + 1) ** 2 for k, v in enumerate(n)]] * 3        # bin k: sigma = (k + 1) code values = 16 (k + 1)

    for valid, full in (((2, 6), [48, 48, 48, 48, 48, 112, 112, 112]), ((0,), [16] * 8), ((7,), [128] * 8),
                        ((1, 3), [32, 32, 32, 64, 64, 64, 64, 64]), (range(8), [16 * (k + 1) for k in range(8)])):
        want = [full[0]] + [(full[k - 1] + full[k] + 1) >> 1 for k in range(1, 8)] + [full[7]]
        assert _c_fit(words(valid), 8, 100, 256) == gnp.fit(words(valid), 8, 100, 256) == grain_fit(words(valid), 8, 100, 256) == [want] * 3
    # the same grain at 10 bits: d is 4 times as large, the table the same; gain scales it
    w10 = [[1000] * 8 + [1000 * 16 * 9] * 8] * 3
    assert _c_fit(w10, 10, 100, 256) == [[48] * 9] * 3 and _c_fit(w10, 10, 200, 256) == [[96] * 9] * 3
    assert _c_fit(w10, 10, 100, 1001) == [[0] * 9] * 3


def test_fit_refusals():
    ok = [[1000] * 16] * 3
    for kwargs, words_ in ((dict(bit_depth=7), "bit_depth"), (dict(bit_depth=17), "bit_depth"), (dict(gain=0), "gain_percent"),
                           (dict(gain=401), "gain_percent"), (dict(min_count=0), "min_count")):
        args = dict(bit_depth=8, gain=100, min_count=256)
        args.update(kwargs)
        assert _c_fit(ok, args["bit_depth"], args["gain"], args["min_count"]) is None
        err = _lib.lib().dcvc_last_error().decode()
        assert err.startswith("grain_fit:") and words_ in err, err
        with pytest.raises(ValueError, match=words_):
            grain_fit(ok, args["bit_depth"], args["gain"], args["min_count"])
        with pytest.raises(ValueError):
            gnp.fit(ok, args["bit_depth"], args["gain"], args["min_count"])
    big = [[1000] * 15 + [1 << 63]] + ok[1:]
    assert _c_fit(big, 8, 100, 256) is None and "2^63" in _lib.lib().dcvc_last_error().decode()
    with pytest.raises(ValueError, match="2\\^63"):
        grain_fit(big, 8, 100, 256)
    f = _lib.fn("dcvc_grain_fit", _ci, [ctypes.c_void_p, _ci, _ci, _ll, ctypes.c_void_p])
    assert f(None, 8, 100, 256, (ctypes.c_uint8 * 27)()) < 0 and f((ctypes.c_uint64 * 48)(), 8, 100, 256, None) < 0


# ------------------------------------------------------------------------------------ what it does
SH, SW, PICS = 64, 256, 4
FLAT, MIN_COUNT, SIZE = 4, 256, 12                   # the tool's defaults


def _sigma(L8):
    """the scene's noise, in 8-bit code values, at 8-bit luma L8"""
    return 1 + 3 * L8 / 255


_scenes = {}


def _scene(bits, strength):
    """-> (the filtered pictures, the summed words of the luma plane)"""
    if (bits, strength) not in _scenes:
        scale = 1 << (bits - 8)
        ramp = np.tile(np.linspace(16, 235, SW), (SH, 1))
        rng = np.random.default_rng(2900 + bits)
        dt = np.uint8 if bits == 8 else np.uint16
        clip = [(np.clip(np.round((ramp + rng.normal(0, 1, (SH, SW)) * _sigma(ramp)) * scale), 0, (1 << bits) - 1).astype(dt),)
                for _ in range(PICS)]
        den = dnp.denoise_clip(clip, strength, strength, bits)
        words = [0] * 16
        for s, d in zip(clip, den):
            words = [a + b for a, b in zip(words, gnp.stats_plane(s[0], d[0], d[0], bits, 0, 0, FLAT))]
        _scenes[(bits, strength)] = (den, words)
    return _scenes[(bits, strength)]


@pytest.mark.parametrize("bits", [8, 10])
def test_the_fit_reads_the_scenes_noise(bits):
    _, words = _scene(bits, 16)
    bins = gnp.fit_bins(words, bits, 100, MIN_COUNT)
    assert sorted(bins) == list(range(8))            # the ramp 16..235 fills every bin
    ratios = [bins[k] / 16 / _sigma(32 * k + 16) for k in range(8)]
    print("%d bits, --denoise 16: counts %s, fitted / true sigma %s" % (bits, words[:8], " ".join("%.2f" % r for r in ratios)))
    assert all(0.75 <= r <= 1.30 for r in ratios), ratios
    lut = gnp.fit([words] * 3, bits, 100, MIN_COUNT)[0]
    assert lut == grain_fit([words] * 3, bits, 100, MIN_COUNT)[0] == _c_fit([words] * 3, bits, 100, MIN_COUNT)[0]
    assert all(lut[k] <= lut[k + 1] + 2 for k in range(8))       # noise that rises with the luma gives a rising table


@pytest.mark.parametrize("bits", [8, 10])
def test_closure_the_synthesised_grain_has_the_tables_deviation(bits):
    den, words = _scene(bits, 16)
    lut = gnp.fit([words] * 3, bits, 100, MIN_COUNT)[0]
    T = _template(1, 0, SIZE)
    sh = bits - 8
    n_all, i_all = [], []
    for pic, d in enumerate(den):
        rec = d[0]
        out = gnp.apply_plane(rec, rec, T, lut, 1, pic, 0, bits, 0, 0)
        assert out.dtype == rec.dtype
        n_all.append(out.astype(np.int64) - rec.astype(np.int64))          # luma 16..235 under grain of a few code values: no clamp
        i_all.append(rec.astype(np.int64) >> sh)
    n, i = np.concatenate(n_all), np.concatenate(i_all)
    lt = np.asarray(lut, np.float64)
    v = (lt[i >> 5] * (32 - (i & 31)) + lt[(i >> 5) + 1] * (i & 31)) / 32
    ratios = []
    for k in range(8):
        m = (i >> 5) == k
        assert m.sum() >= MIN_COUNT
        ratios.append(float(n[m].std() * 16 / (1 << sh) / v[m].mean()))
    print("%d bits: synthesised / table deviation per bin %s" % (bits, " ".join("%.2f" % r for r in ratios)))
    assert all(0.8 <= r <= 1.2 for r in ratios), ratios


def test_a_table_of_zeros_copies_and_pic_moves_the_blocks():
    rng = np.random.default_rng(3)
    rec = rng.integers(0, 256, (70, 100)).astype(np.uint8)
    T = _template(1, 0, SIZE)
    assert np.array_equal(gnp.apply_plane(rec, rec, T, [0] * 9, 1, 0, 0, 8, 0, 0), rec)
    a, b = (gnp.apply_plane(rec, rec, T, [64] * 9, 1, pic, 0, 8, 0, 0) for pic in (0, 1))
    assert not np.array_equal(a, b) and not np.array_equal(a, rec)
    ox, oy = gnp.block_offsets(1, 0, 0, 3, 4)
    assert ox.shape == (3, 4) and 0 <= ox.min() and ox.max() <= 63 and 0 <= oy.min() and oy.max() <= 63
    assert len({(int(x), int(y)) for x, y in zip(ox.ravel(), oy.ravel())}) > 6           # the blocks do not share an offset
