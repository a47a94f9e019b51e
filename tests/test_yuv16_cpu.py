"""High-bit-depth YUV420 without a GPU: the numpy restatement (tests/yuv16_np.py) against the torch-op fixture
tests/golden/yuv16_golden.npz and against DCVC-FM's reader formula, the MS-SSIM restatement at a data range, and the argument
checks of dcvc_yuv420p16_to_x, dcvc_x_to_yuv420p16, dcvc_sse / dcvc_sse_ws with the new sample types and dcvc_msssim_range,
which refuse before touching the device."""
import ctypes
import os

import numpy as np

import msssim_np
import msssim_range_np
import yuv16_np

vp, ci, ll, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a.view(np.uint32) if a.dtype == np.float32 else a


def test_restatement_equals_the_fixture_bit_for_bit(golden_dir):
    z = np.load(os.path.join(golden_dir, "yuv16_golden.npz"))
    assert sorted(set(z["y10"].ravel().tolist())) == list(range(1024))
    assert np.array_equal(_bits(yuv16_np.yuv420p16_to_x(z["y10"], z["uv10"], 10)), _bits(z["x10"]))
    H, W = (int(v) for v in z["crop"])
    for b in (10, 16):
        dy, duv, y16, uv16 = yuv16_np.x_to_yuv420p16(z["x_hat"], H, W, b)
        assert np.array_equal(_bits(dy), _bits(z["dist_y%d" % b])), b
        assert np.array_equal(_bits(duv), _bits(z["dist_uv%d" % b])), b
        assert np.array_equal(y16, z["y16_%d" % b]) and np.array_equal(uv16, z["uv16_%d" % b]), b
        m = (1 << b) - 1
        # the fixture reaches both clamps, and the writer rounds half to even on every plane
        assert (z["dist_y%d" % b] == 0).any() and (z["dist_y%d" % b] == m).any()
    assert np.rint(np.float32(2.5)) == 2 and np.array_equal(np.rint(np.float32([0.5, 1.5])), [0, 2])


def test_reader_equals_fm_formula():
    """YUVReader: np.frombuffer(b, '<u2').astype(np.float32) / max_val, for every code, little-endian bytes"""
    for b in (9, 10, 12, 16):
        m = (1 << b) - 1
        y, uv = yuv16_np.all_codes(b, W=256)
        raw = y.astype("<u2").tobytes() + uv.astype("<u2").tobytes()
        H, W = y.shape
        ry, ruv = yuv16_np.read_picture(raw, H, W)
        assert np.array_equal(ry, y) and np.array_equal(ruv, uv)
        fm = np.frombuffer(raw, "<u2").astype(np.float32) / m
        mine = np.concatenate([yuv16_np.reader_scale(ry, b).ravel(), yuv16_np.reader_scale(ruv, b).ravel()])
        assert np.array_equal(_bits(mine), _bits(fm)), b
        # x = fp16(fp16(that) - 0.5) on Y
        x = yuv16_np.yuv420p16_to_x(ry, ruv, b)
        want = (fm[:H * W].astype(np.float16).astype(np.float32) - np.float32(0.5)).astype(np.float16).reshape(H, W)
        assert np.array_equal(_bits(x[..., 0]), _bits(want)), b
    # the byte order is little-endian whatever the host's
    assert yuv16_np.read_picture(bytes([0x01, 0x02] * 6), 2, 2)[0][0, 0] == 0x0201


def test_psnr_restatement():
    rng = np.random.default_rng(3)
    y = rng.integers(0, 1024, (16, 16)).astype(np.uint16)
    uv = rng.integers(0, 1024, (2, 8, 8)).astype(np.uint16)
    dy = (y + rng.normal(0, 3, y.shape)).astype(np.float32)
    duv = (uv + rng.normal(0, 3, uv.shape)).astype(np.float32)
    p = yuv16_np.psnr_yuv420(y, uv, dy, duv, 10)
    mse_y = np.mean((y.astype(np.float64) - dy) ** 2)
    assert abs(p[1] - 10 * np.log10(1023.0 ** 2 / mse_y)) < 1e-12
    assert p[0] == (6 * p[1] + p[2] + p[3]) / 8
    assert yuv16_np.psnr(0.0, 100, 10) == 99.9


def test_msssim_range_restatement_at_255_equals_msssim_np():
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, (96, 100)).astype(np.float64)
    b = np.clip(a + rng.normal(0, 6, a.shape), 0, 255)
    assert msssim_range_np.msssim(a, b, 255.0) == msssim_np.msssim(a, b)
    # scaling both planes and the range together leaves the metric unchanged up to rounding
    assert abs(msssim_range_np.msssim(a * 4, b * 4, 1020.0) - msssim_np.msssim(a, b)) < 1e-12


def _err():
    from dcvc_amd import _lib
    return _lib.lib().dcvc_last_error().decode()


def _refused(f, cases):
    for args, msg in cases:
        assert f(*args) == -1, args
        assert msg in _err(), (args, _err())


def test_abi_refuses_bad_arguments():
    from dcvc_amd import _lib
    to_x = _lib.fn("dcvc_yuv420p16_to_x", ci, [vp, vp, ci, ci, ci, vp, ci, vp])
    to_yuv = _lib.fn("dcvc_x_to_yuv420p16", ci, [vp, ci, ci, ci, ci, vp, vp, vp])
    p = vp(4096)     # never dereferenced: every call below is refused by the argument checks
    _refused(to_x, [((p, p, 64, 128, 8, p, 3, None), "bit depth"),
                    ((p, p, 64, 128, 17, p, 3, None), "bit depth"),
                    ((p, p, 64, 128, 0, p, 3, None), "bit depth"),
                    ((p, p, 63, 128, 10, p, 3, None), "even"),
                    ((p, p, 64, 127, 10, p, 3, None), "even"),
                    ((p, p, 0, 128, 10, p, 3, None), "even"),
                    ((None, p, 64, 128, 10, p, 3, None), "null"),
                    ((p, None, 64, 128, 10, p, 3, None), "null"),
                    ((p, p, 64, 128, 10, None, 3, None), "null"),
                    ((p, p, 64, 128, 10, p, 2, None), ">= 3"),
                    ((p, p, 1 << 30, 1 << 30, 10, p, 3, None), "too large")])
    _refused(to_yuv, [((p, 128, 64, 128, 8, p, p, None), "bit depth"),
                      ((p, 128, 64, 128, 17, p, p, None), "bit depth"),
                      ((p, 128, 63, 128, 10, p, p, None), "even"),
                      ((p, 128, 64, 126 + 1, 10, p, p, None), "even"),
                      ((p, 127, 64, 128, 10, p, p, None), "shorter"),
                      ((None, 128, 64, 128, 10, p, p, None), "x_hat")])
    # both outputs null: nothing to do, and nothing launched
    assert to_yuv(p, 128, 64, 128, 10, None, None, None) == 0

    sse = _lib.fn("dcvc_sse", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, vp, vp])
    sse_ws = _lib.fn("dcvc_sse_ws", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, vp, vp, ll, vp])
    ws_bytes = _lib.fn("dcvc_sse_workspace_bytes", ll, [ci, ci, ci])
    need = ws_bytes(1, 64, 64)
    # the new sample types pass the type check and meet the same geometry checks as u8 / fp16 ...
    _refused(sse, [((p, 3, p, 4, 1, 64, 64, 63, 0, p, None), "row stride"),
                   ((p, 4, p, 3, 3, 64, 64, 64, 4000, p, None), "plane stride"),
                   ((None, 3, p, 4, 1, 64, 64, 64, 0, p, None), "null"),
                   ((p, 3, p, 4, 0, 64, 64, 64, 0, p, None), "empty"),
                   # ... and unknown types are still refused: 2 stays unassigned, 5 and -1 are unknown
                   ((p, 2, p, 4, 1, 64, 64, 64, 0, p, None), "sample type"),
                   ((p, 3, p, 5, 1, 64, 64, 64, 0, p, None), "sample type"),
                   ((p, -1, p, 3, 1, 64, 64, 64, 0, p, None), "sample type")])
    _refused(sse_ws, [((p, 3, p, 4, 1, 64, 64, 64, 0, p, None, need, None), "workspace"),
                      ((p, 3, p, 4, 1, 64, 64, 64, 0, p, p, need - 8, None), "workspace"),
                      ((p, 3, p, 6, 1, 64, 64, 64, 0, p, p, need, None), "sample type")])

    ms = _lib.fn("dcvc_msssim", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, vp, vp])
    ms_range = _lib.fn("dcvc_msssim_range", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, dbl, vp, vp])
    # dcvc_msssim keeps its contract: u8 / fp16 only
    _refused(ms, [((p, 3, p, 4, 1, 100, 100, 100, 0, p, None), "sample type"),
                  ((p, 0, p, 4, 1, 100, 100, 100, 0, p, None), "sample type")])
    _refused(ms_range, [((p, 3, p, 4, 1, 100, 100, 100, 0, 0.0, p, None), "data_range"),
                        ((p, 3, p, 4, 1, 100, 100, 100, 0, -1023.0, p, None), "data_range"),
                        ((p, 3, p, 4, 1, 100, 100, 100, 0, float("nan"), p, None), "data_range"),
                        ((p, 3, p, 4, 1, 100, 100, 100, 0, float("inf"), p, None), "data_range"),
                        ((p, 2, p, 4, 1, 100, 100, 100, 0, 1023.0, p, None), "sample type"),
                        ((p, 3, p, 9, 1, 100, 100, 100, 0, 1023.0, p, None), "sample type"),
                        ((p, 3, p, 4, 1, 87, 100, 100, 0, 1023.0, p, None), "88"),
                        ((p, 3, p, 4, 1, 100, 100, 99, 0, 1023.0, p, None), "row_stride"),
                        ((None, 3, p, 4, 1, 100, 100, 100, 0, 1023.0, p, None), "operand")])


def test_python_wrapper_checks():
    """dcvc_amd.yuv16's own refusals and bit-depth helper, before any device work"""
    import pytest
    from dcvc_amd import yuv16
    assert yuv16.max_val(10) == 1023 and yuv16.max_val(16) == 65535
    for b in (8, 17):
        with pytest.raises(ValueError):
            yuv16.max_val(b)
    assert yuv16.DCVC_SAMPLE_U16 == 3 and yuv16.DCVC_SAMPLE_F32 == 4
