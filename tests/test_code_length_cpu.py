"""Code-length tables (csrc/rans/code_length.cpp) against their numpy restatement, entry for entry, and the length they
predict against the bytes the product's own rANS coder writes. No GPU involved."""
import ctypes
import os
import sys

import numpy as np
import pytest

import dcvc_amd
from dcvc_amd import _lib, rate_control

dcvc_amd.install_plugin()
import MLCodec_extensions_cpp as mine  # noqa: E402  (the product's plug-in module)

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import code_length_np as cl  # noqa: E402
from make_rans_golden import case_inputs  # noqa: E402

_i32p, _u32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)

# DESIGN.md 15, "Measured prediction error": the largest (coded - ideal - fixed) / ideal over the inputs of
# test_prediction_against_the_coder was r = 3.78e-5 (2026-10-16, case_inputs at 500 000 symbols, one sub-stream).
# The bound is twice that.
R_MEASURED = 3.78e-5
R_BOUND = 2 * R_MEASURED

COUNTS = (4099, 70001, 500000)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "rans_golden.npz"))


def native_table(cdfs, sizes, cols):
    f = _lib.fn("dcvc_code_length_table", ctypes.c_int, [_i32p, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, _u32p])
    cdfs = np.ascontiguousarray(cdfs, dtype=np.int32)
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    out = np.zeros((cdfs.shape[0], cols), dtype=np.uint32)
    _lib.check(f(cdfs.ctypes.data_as(_i32p), cdfs.shape[0], cdfs.shape[1], sizes.ctypes.data_as(_i32p), cols,
                 out.ctypes.data_as(_u32p)))
    return out


@pytest.mark.parametrize("family,cols", [("y", 256), ("z", 128)])
def test_table_equals_numpy_entry_for_entry(golden, family, cols):
    want = cl.table(golden[family + "_cdf"], golden[family + "_len"], cols)
    got = native_table(golden[family + "_cdf"], golden[family + "_len"], cols)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert (got != cl.UNCODABLE).all()


def test_cost_of_every_frequency():
    """equality, not closeness: a log2 that differed in the last place between libm and numpy would show here"""
    f = _lib.fn("dcvc_code_length_cost", ctypes.c_uint32, [ctypes.c_int, ctypes.c_int])
    freqs = np.arange(1, 65536)
    want = cl.cost(freqs)
    got = np.array([f(int(v), 0) for v in freqs], dtype=np.uint64)
    assert np.array_equal(got, want), freqs[got != want][:8]
    assert f(65536, 0) == 0 and f(1, 0) == 16 << 16
    # bypass groups: 2 bits each on top
    assert f(4096, 5) == (4 << 16) + 5 * (2 << 16)
    assert f(0, 0) == cl.UNCODABLE and f(65537, 0) == cl.UNCODABLE


def test_escapes_and_mapping_on_a_two_symbol_family():
    """cdf_len 3: values 0 and 1, max_value = 1 -> every symbol but 0 is an escape with its own group count"""
    cdfs = np.array([[0, 49152, 65536, 0]], dtype=np.int32)
    t = native_table(cdfs, [3], 256)
    assert np.array_equal(t, cl.table(cdfs, [3], 256))
    unit = 1 << 16
    esc = int(cl.cost(16384))                                  # 2 bits
    assert t[0, 0] == int(cl.cost(49152))
    assert t[0, 1] == esc + 2 * unit                           # symbol 1 -> value 1 = max_value, raw 0: the count group only
    assert t[0, 255] == esc + 2 * 2 * unit                     # symbol -1 -> value 2, raw 1: 1 raw group + count
    assert t[0, 2] == esc + 2 * 2 * unit                       # symbol 2 -> value 3, raw 2: still one raw group
    assert t[0, 3] == esc + 3 * 2 * unit                       # symbol 3 -> value 5, raw 4: 2 raw groups + count
    assert t[0, 0x80] == esc + (4 + 1 + 1) * 2 * unit          # symbol -128 -> value 256, raw 255: 4 raw + count + 1 continuation


def _encode(g, n, comb, z):
    e = mine.RansEncoder()
    e.set_cdf(g["z_cdf"], g["z_len"], 0)
    e.set_cdf(g["y_cdf"], g["y_len"], 1)
    e.reset()
    e.set_entropy_coder_parallel(n)
    e.encode_y(comb)
    e.encode_z(z, 128, 128)
    e.flush()
    return e.get_encoded_stream()


def prediction_cases(g):
    for count in COUNTS:
        comb, z = case_inputs(7 + count, count)
        yield "case_inputs", count, comb, z
        yield "drawn", count, cl.draw_from_tables(g["y_cdf"], g["y_len"], 11 + count, count), z
        yield "all-zero", count, np.zeros(count, dtype=np.int16), np.zeros_like(z)


def test_prediction_against_the_coder(golden):
    """8 len(stream) of the product's RansEncoder against the table-gathered ideal length: never below it, and above it by
    at most the format's fixed bits plus R_BOUND of the ideal length, for 1 .. 8 sub-streams."""
    ty = native_table(golden["y_cdf"], golden["y_len"], 256)
    tz = native_table(golden["z_cdf"], golden["z_len"], 128)
    worst = 0.0
    for name, count, comb, z in prediction_cases(golden):
        y_units, symbols = cl.sum_y(ty, comb)
        assert symbols == count
        z_units = cl.sum_z(tz[128:256], z, 128)
        ideal = (y_units + z_units) / cl.UNIT
        for n in range(1, 9):
            coded = 8 * len(_encode(golden, n, comb, z))
            fixed = rate_control.stream_fixed_bits(n)
            excess = max(coded - ideal - fixed, 0.0)
            worst = max(worst, excess / ideal)
            print("%-11s %6d symbols, %d sub-streams: coded %8d, ideal %11.1f, fixed %3d, excess %6.1f (%.3g of ideal)"
                  % (name, count, n, coded, ideal, fixed, excess, excess / ideal))
            assert coded >= ideal, (name, count, n, coded, ideal)
            assert coded <= ideal + fixed + R_BOUND * ideal, (name, count, n, coded, ideal)
            # the helper the probe's users call: ideal + fixed bits, rounded up to bytes
            pred = rate_control.predicted_stream_bytes(y_units, z_units, n)
            assert 8 * pred >= ideal + fixed > 8 * (pred - 1)
    print("largest excess / ideal: %.3g" % worst)


def test_predicted_stream_bytes_native_equals_python():
    f = _lib.fn("dcvc_predicted_stream_bytes", ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int])
    rng = np.random.default_rng(5)
    for n in range(1, 9):
        assert rate_control.stream_fixed_bits(n) == 32 * n + 32 * (0 if n < 3 else n // 2 - 1 + n % 2)
        for y, z in [(0, 0), (1, 0), (8 * 65536, 0), (8 * 65536 + 1, 0)] + [tuple(rng.integers(0, 1 << 40, 2)) for _ in range(50)]:
            assert f(int(y), int(z), n) == rate_control.predicted_stream_bytes(int(y), int(z), n)
    assert f(0, 0, 0) < 0 and f(0, 0, 9) < 0 and f(-1, 0, 1) < 0
    e = _lib.fn("dcvc_ec_parallel_for", ctypes.c_int, [ctypes.c_int64])
    for s in (0, 1, 32767, 32768, 65535, 65536, 8 * 32768 - 1, 8 * 32768, 10 ** 7):
        assert e(s) == rate_control.ec_parallel_for(s)
