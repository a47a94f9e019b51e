"""MS-SSIM without a GPU: the numpy restatement (tests/msssim_np.py) against the reference's calc_msssim values stored in
tests/golden/msssim_golden.npz, and the C-ABI entry point's argument checks, which refuse before touching the device."""
import ctypes
import math
import os

import numpy as np
import pytest

import msssim_np


def _cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "msssim_golden.npz"))
    names = sorted(k[:-len("_value")] for k in z.files if k.endswith("_value"))
    return [(n, z[n + "_src"], z[n + "_rec"], float(z[n + "_value"])) for n in names]


def test_numpy_restatement_matches_the_reference(golden_dir):
    cases = _cases(golden_dir)
    assert len(cases) == 9
    for name, src, rec, want in cases:
        got = msssim_np.msssim_rgb(src, rec) if src.ndim == 3 else msssim_np.msssim(src, rec)
        if math.isnan(want):
            assert math.isnan(got), name
        else:
            assert abs(got - want) <= 1e-12, (name, got, want)
    values = {n: v for n, _, _, v in cases}
    assert values["same_120x128"] == 1.0 and math.isnan(values["inv_120x128"])


def test_numpy_level_count_and_minimum_size():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (88, 176)).astype(np.uint8)
    assert 0 < msssim_np.msssim(a, a // 2 + 60) < 1
    for shape in [(87, 200), (200, 87)]:
        with pytest.raises(ValueError, match="88"):
            msssim_np.msssim(np.zeros(shape), np.zeros(shape))


def test_abi_refuses_bad_arguments():
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_msssim", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p,
                                              ctypes.c_void_p])
    p = ctypes.c_void_p(16)      # never dereferenced: every call below is refused by the argument checks
    bad = [((p, 0, p, 1, 1, 87, 200, 200, 0, p, None), "88"),          # a side below 88
           ((p, 0, p, 1, 1, 200, 87, 87, 0, p, None), "88"),
           ((p, 2, p, 1, 1, 100, 100, 100, 0, p, None), "sample type"),  # bad dtype
           ((p, 0, p, 7, 1, 100, 100, 100, 0, p, None), "sample type"),
           ((p, 0, p, 0, 1, 100, 100, 99, 0, p, None), "row_stride"),   # row_stride < W
           ((p, 0, p, 0, 2, 100, 100, 100, 5000, p, None), "overlap"),  # planes overlap
           ((p, 0, p, 0, 0, 100, 100, 100, 0, p, None), "planes"),
           ((None, 0, p, 0, 1, 100, 100, 100, 0, p, None), "missing")]
    for args, msg in bad:
        assert f(*args) == -1, args
        assert msg in _lib.lib().dcvc_last_error().decode(), (args, _lib.lib().dcvc_last_error())
