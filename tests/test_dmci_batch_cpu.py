"""Intra batches: the argument checks of the batched C ABI run before any device work, so they hold on a box
without a GPU (tests/test_dmci_batch_gpu.py checks the rest on an MI355X)."""
import ctypes

import pytest

_vp, _ci = ctypes.c_void_p, ctypes.c_int


def _fn(name, restype, args):
    from dcvc_amd import _lib
    return _lib.fn(name, restype, args)


def _err():
    from dcvc_amd import _lib
    return _lib.lib().dcvc_last_error().decode()


FAKE = _vp(0x1000)       # never dereferenced: every call below is refused before it reaches the device


@pytest.mark.parametrize("n", [0, 2, 17])
def test_codec_batch_entry_points_refuse_a_null_codec_and_bad_n(n):
    ec = (_ci * 16)()
    cb = _fn("dcvc_dmci_compress_batch", _ci, [_vp, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _vp, ctypes.POINTER(_ci), _vp])
    assert cb(None, n, FAKE, 64, 64, 20, 0, 0, FAKE, ec, None) < 0
    assert "codec" in _err() or "batch size" in _err()
    db = _fn("dcvc_dmci_decompress_batch", _ci, [_vp, _ci, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_size_t),
                                                 ctypes.POINTER(_ci), _ci, _ci, _ci, _vp, _vp])
    ptrs, sizes = (_vp * 16)(), (ctypes.c_size_t * 16)()
    assert db(None, n, ptrs, sizes, ec, 20, 64, 64, FAKE, None) < 0
    gs = _fn("dcvc_dmci_get_stream_at", ctypes.c_int64, [_vp, _ci, _vp, ctypes.c_size_t])
    assert gs(None, 0, None, 0) < 0


@pytest.mark.parametrize("n", [0, 17, -3])
def test_kernel_batch_entry_points_refuse_n_out_of_range(n):
    dw = _fn("dcvc_dwconv3x3_b", _ci, [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp])
    assert dw(FAKE, 64, FAKE, FAKE, 64, 4, 4, 64, n, None) < 0
    assert "n must be in [1, 16]" in _err()
    crop = _fn("dcvc_crop_b", _ci, [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _vp])
    assert crop(FAKE, 64, 8, 8, FAKE, 64, 4, 4, 64, n, None) < 0
    pu = _fn("dcvc_pad_unshuffle8_b", _ci, [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _vp])
    assert pu(FAKE, 16, 16, 3, FAKE, 2, 2, n, None) < 0


def test_kernel_batch_entry_points_refuse_null_pointers_and_bad_geometry():
    dw = _fn("dcvc_dwconv3x3_b", _ci, [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp])
    assert dw(None, 64, FAKE, FAKE, 64, 4, 4, 64, 2, None) < 0
    assert dw(FAKE, 64, FAKE, FAKE, 64, 0, 4, 64, 2, None) < 0
    crop = _fn("dcvc_crop_b", _ci, [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _vp])
    assert crop(FAKE, 64, 4, 4, FAKE, 64, 5, 4, 64, 2, None) < 0             # taller than its input
    rp = _fn("dcvc_replicate_pad_b", _ci, [_vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _vp])
    assert rp(FAKE, 64, 4, 4, 64, -1, 0, FAKE, 64, 2, None) < 0              # negative padding
    pu = _fn("dcvc_pad_unshuffle8_b", _ci, [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _vp])
    assert pu(FAKE, 17, 16, 3, FAKE, 2, 2, 2, None) < 0                      # 2 x 8 rows < 17
    kxk = _fn("dcvc_conv_kxk_b", _ci, [_vp, _ci, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp])
    assert kxk(FAKE, 64, FAKE, None, None, 64, 8, 8, 64, 64, 3, 2, 1, 2, None) < 0
