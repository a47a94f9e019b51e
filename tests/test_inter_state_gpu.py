"""The temporal-state hand-off format and the debug_read edges of the inter codecs on a real MI355X (-m gpu): DMCLDProxy /
DMCHTSProxy / DMCHTLProxy.

  * state layout: export_state() is, byte for byte, a 64-byte header [magic, H8, W8, flags, 0 x 12] (little-endian uint32)
    followed by the reference feature, memory | feature_p per pixel, ctx and (LD) the temporal prior, each dense, as
    debug_read gives them; the flags are those of an encoder behind one compress (15) and of a decoder behind one
    decompress without reset (13); a fresh object that imports the buffer exports the same bytes;
  * debug_read: an unknown name and a destination one byte short are refused and leave the object usable; a channel slice
    of a wider buffer ("y_hat") comes back dense and equal to the oracle's.

144 x 176: the 9 x 11 latent is padded to 12 x 12 for the hyper networks; 64 x 64: 4 x 4, no padding."""
import ctypes

import numpy as np
import pytest
import torch

from codec_util import oracle_for, picture
from dcvc_amd import _lib
from test_inter_probe_gpu import KINDS, _model, _padding, _proxy, _ref, _x

pytestmark = pytest.mark.gpu

SIZES = [(144, 176), (64, 64)]
MAGIC = {"ld": 0x44434C44, "hts": 0x44434854 ^ 1, "htl": 0x44434854}
HEADER_BYTES = 64


def _expected_state(p, kind, h, w, flags):
    header = np.zeros(HEADER_BYTES // 4, dtype="<u4")
    header[:4] = [MAGIC[kind], -(-h // 16) * 2, -(-w // 16) * 2, flags]
    p8 = int(header[1]) * int(header[2])

    def part(name):
        return p.debug_read(name, np.float16).reshape(p8, -1)

    parts = [part("feature_i"), np.concatenate([part("memory"), part("feature_p")], axis=1), part("ctx")]
    if kind == "ld":
        parts.append(p.debug_read("temporal", np.float16))
    return np.concatenate([header.view(np.uint8)] + [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in parts])


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_state_layout(kind, h, w):
    pb, pr = _padding(h, w)
    ref, x = _ref(h, w), _x(kind, h, w, 0)
    enc, dec = _proxy(kind), _proxy(kind)
    enc.add_ref_feature_from_frame(ref, True)
    bs, ec = enc.compress(x, 30, False, pb, pr)
    dec.add_ref_feature_from_frame(ref, False)
    dec.decompress(bs, 30, h, w, ec, False)
    torch.cuda.synchronize()
    for p, flags in ((enc, 15), (dec, 13)):
        state = p.export_state()
        got = state.cpu().numpy()
        print(kind, h, w, "flags", int(got[12:16].view("<u4")[0]), "bytes", got.size)
        assert np.array_equal(got, _expected_state(p, kind, h, w, flags))
        q = _proxy(kind)
        q.import_state(state, h, w)
        assert torch.equal(q.export_state(), state)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_debug_read_refusals(kind, h, w):
    pb, pr = _padding(h, w)
    ref, x = _ref(h, w), _x(kind, h, w, 0)
    p, twin = _proxy(kind), _proxy(kind)
    for o in (p, twin):
        o.add_ref_feature_from_frame(ref, True)
    with pytest.raises(_lib.DcvcError, match="unknown debug tensor"):
        p.debug_read("no_such_tensor", np.float16)
    from inference_extensions_cuda import _HT, _LD      # importable once a proxy exists
    fn = (_LD if kind == "ld" else _HT)["debug_read"]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = _lib.check(fn(p._h, b"ctx", None, 0, stream))
    buf = np.zeros(n, dtype=np.uint8)
    with pytest.raises(_lib.DcvcError, match="destination too small"):
        _lib.check(fn(p._h, b"ctx", buf.ctypes.data_as(ctypes.c_void_p), n - 1, stream))
    assert not buf.any()                                             # refused before anything was copied
    assert _lib.check(fn(p._h, b"ctx", buf.ctypes.data_as(ctypes.c_void_p), n, stream)) == n
    assert np.array_equal(buf.view(np.float16), twin.debug_read("ctx", np.float16))
    got, want = p.compress(x, 30, False, pb, pr), twin.compress(x, 30, False, pb, pr)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]


@pytest.mark.parametrize("kind", KINDS)
def test_debug_read_strided_view_is_dense(kind):
    """y_hat is the first kChY channels of the wider spatial-prior input (LD: 128 of ld 512, HT: 256 of ld 512)"""
    h, w = 64, 64
    m = _model(kind)
    o, p = oracle_for(m), _proxy(kind)
    o.add_ref_feature_from_frame(picture(h, w, index=0), True)
    p.add_ref_feature_from_frame(_ref(h, w), True)
    x = _x(kind, h, w, 0)
    want = o.compress(x[0].permute(1, 2, 0).contiguous().cpu().numpy(), 30, False)
    bs, ec = p.compress(x, 30, False, 0, 0)
    torch.cuda.synchronize()
    assert bytes(bs) == bytes(want["bit_stream"]) and ec == want["ec_parallel"]
    y_hat = o.debug["y_hat"]
    assert y_hat.shape[:2] == (h // 16, w // 16)
    assert np.array_equal(p.debug_read("y_hat", np.float16).reshape(y_hat.shape), y_hat)
