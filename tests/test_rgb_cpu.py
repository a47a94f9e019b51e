"""RGB pictures without a GPU: the numpy restatement (tests/rgb_np.py) against the reference's colour transforms stored in
tests/golden/rgb_golden.npz (CPU torch, so div="true"), and the argument checks of dcvc_rgb_to_x, dcvc_x_to_rgb and
dcvc_sse, which refuse before touching the device."""
import ctypes
import os

import numpy as np

import rgb_np

vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


def _bits(a):
    return a.view(np.uint16) if a.dtype == np.float16 else a


def test_restatement_equals_the_reference_bit_for_bit(golden_dir):
    z = np.load(os.path.join(golden_dir, "rgb_golden.npz"))
    rgb = z["rgb"]
    for c in range(3):
        assert sorted(set(rgb[c, c].tolist())) == list(range(256))
    assert np.array_equal(_bits(rgb_np.rgb_to_x(rgb, "true")), _bits(z["x"]))
    H, W = (int(v) for v in z["crop"])
    rgb16, rgb8 = rgb_np.x_to_rgb(z["x_hat"], H, W, "true")
    assert np.array_equal(_bits(rgb16), _bits(z["rgb16"]))
    assert np.array_equal(rgb8, z["rgb8"])
    # the fixture reaches both clamps
    assert (z["rgb16"] == 0).any() and (z["rgb16"] == 255).any()


def test_restatement_division_conventions_differ():
    """the two conventions are distinguishable on the colour cube, so the GPU tests tell which one the kernels follow"""
    cube = rgb_np.all_colours()[:, :512]
    assert not np.array_equal(_bits(rgb_np.rgb_to_x(cube, "true")), _bits(rgb_np.rgb_to_x(cube, "recip")))


def _err():
    from dcvc_amd import _lib
    return _lib.lib().dcvc_last_error().decode()


def test_abi_refuses_bad_arguments():
    from dcvc_amd import _lib
    to_x = _lib.fn("dcvc_rgb_to_x", ci, [vp, ll, ll, ll, ci, ci, vp, ci, vp, vp])
    to_rgb = _lib.fn("dcvc_x_to_rgb", ci, [vp, ci, ci, ci, vp, vp, vp])
    sse = _lib.fn("dcvc_sse", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, vp, vp])
    p = vp(4096)     # never dereferenced: every call below is refused by the argument checks
    bad_to_x = [((p, 384, 3, 1, 63, 128, p, 3, None, None), "even"),         # odd height
                ((p, 384, 3, 1, 64, 127, p, 3, None, None), "even"),         # odd width
                ((p, 384, 3, 1, 0, 128, p, 3, None, None), "even"),          # empty
                ((p, 384, 3, 1, 64, 128, None, 3, None, None), "neither"),   # no output
                ((None, 384, 3, 1, 64, 128, p, 3, None, None), "source"),
                ((p, 384, 3, 1, 64, 128, p, 2, None, None), ">= 3"),         # ldx
                ((p, 383, 3, 1, 64, 128, p, 3, None, None), "too small"),    # packed rows overlap
                ((p, 384, 2, 1, 64, 128, p, 3, None, None), "too small"),    # pixels overlap
                ((p, 128, 1, 128 * 63, 64, 128, p, 3, None, None), "too small"),   # planar: planes overlap
                ((p, 384, 3, 0, 64, 128, p, 3, None, None), "positive"),
                ((p, -384, 3, 1, 64, 128, p, 3, None, None), "positive"),
                ((p, 3 << 30, 3, 1, 1 << 30, 1 << 30, p, 3, None, None), "too large")]
    for args, msg in bad_to_x:
        assert to_x(*args) == -1, args
        assert msg in _err(), (args, _err())
    bad_to_rgb = [((p, 128, 63, 128, p, p, None), "even"),
                  ((p, 127, 64, 128, p, p, None), "shorter"),
                  ((None, 128, 64, 128, p, p, None), "x_hat")]
    for args, msg in bad_to_rgb:
        assert to_rgb(*args) == -1, args
        assert msg in _err(), (args, _err())
    bad_sse = [((p, 2, p, 1, 1, 64, 64, 64, 0, p, None), "sample type"),
               ((p, 0, p, 5, 1, 64, 64, 64, 0, p, None), "sample type"),
               ((None, 0, p, 0, 1, 64, 64, 64, 0, p, None), "null"),
               ((p, 0, p, 0, 1, 64, 64, 64, 0, None, None), "null"),
               ((p, 0, p, 0, 1, 64, 64, 63, 0, p, None), "row stride"),
               ((p, 0, p, 0, 3, 64, 64, 64, 4000, p, None), "plane stride"),
               ((p, 0, p, 0, 0, 64, 64, 64, 4096, p, None), "empty"),
               ((p, 0, p, 0, 1, 0, 64, 64, 0, p, None), "empty"),
               ((p, 0, p, 0, 1, 1 << 30, 1 << 30, 1 << 30, 0, p, None), "too large")]
    for args, msg in bad_sse:
        assert sse(*args) == -1, args
        assert msg in _err(), (args, _err())
    ws_bytes = _lib.fn("dcvc_sse_workspace_bytes", ll, [ci, ci, ci])
    sse_ws = _lib.fn("dcvc_sse_ws", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, vp, vp, ll, vp])
    need = ws_bytes(3, 1080, 1920)
    assert need == 3 * 1013 * 8 and ws_bytes(0, 64, 64) == 0
    for args, msg in [((p, 0, p, 1, 3, 1080, 1920, 1920, 1080 * 1920, p, None, need, None), "workspace"),
                      ((p, 0, p, 1, 3, 1080, 1920, 1920, 1080 * 1920, p, p, need - 8, None), "workspace"),
                      ((p, 0, p, 1, 3, 1080, 1920, 1919, 1080 * 1920, p, p, need, None), "row stride")]:
        assert sse_ws(*args) == -1, args
        assert msg in _err(), (args, _err())
