"""The encoder-side reconstruction of the inter codecs on a real MI355X (-m gpu), DESIGN.md 21: DMCLDProxy / DMCHTSProxy /
DMCHTLProxy.reconstruct.

  * equals the decoder: behind every compress of a plan with a reset and two q changes, reconstruct gives, bit for bit, what a
    second object's decompress of that stream writes - at 144 x 176 and at 240 x 424, whose latent is padded;
  * no trace: an object that reconstructs behind every unit - twice in a row once, once with a size probe in between - writes
    the streams, holds the temporal state and feeds a decoder exactly as one that never does, with graphs and without (the
    head output goes to a scratch plane: the reference feature is state);
  * hand-off: an object that imported the state reconstructs the same pictures;
  * refused right behind add_ref, and with a null x_hat, the state untouched."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from codec_util import chunk, dmc_ht_model, dmc_ld_model, picture, to_device_input
from dcvc_amd import _lib

pytestmark = pytest.mark.gpu

KINDS = ["ld", "hts", "htl"]
PLAN = [(30, 0), (30, 0), (45, 1), (45, 0), (12, 0), (12, 0)]       # a reset and two q changes; graphs: eager, captured, replayed


def _model(kind):
    return dmc_ld_model(skip_thres=0.15) if kind == "ld" else dmc_ht_model(kind, skip_thres=0.15)


def _proxy(kind, graphs=None):
    g = copy.deepcopy(_model(kind)).half().cuda()
    g.proxy = None
    p = g._ensure_proxy()
    if graphs is not None:
        p.set_use_graphs(graphs)
    return p


def _ref(h, w):
    x = picture(h, w, index=0)
    return to_device_input(np.pad(x, ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge"))


def _x(kind, h, w, i):
    """unit i of the clip: one picture (LD) or the 8-picture chunk compress takes (HT)"""
    return to_device_input(picture(h, w, index=1 + i) if kind == "ld" else chunk(h, w, 1 + 8 * i))


def _pictures(kind, d):
    """the proxy-owned result of decompress / reconstruct as one tensor of its own"""
    if kind != "ld":
        assert len(d) == 8 and all(t is not None for t in d)
    return (d if kind == "ld" else torch.cat(list(d), 0)).clone()


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("h,w", [(144, 176), (240, 424)])          # 240 x 424: 15 x 27 latent rows, padded to 16 x 28
@pytest.mark.parametrize("kind", KINDS)
def test_reconstruct_equals_the_decoder(kind, h, w, graphs):
    pb, pr = -h % 16, -w % 16
    ref = _ref(h, w)
    enc, dec = _proxy(kind, graphs), _proxy(kind, graphs)
    enc.add_ref_feature_from_frame(ref, True)
    dec.add_ref_feature_from_frame(ref, False)
    for i, (qp, reset) in enumerate(PLAN):
        bs, ec = enc.compress(_x(kind, h, w, i), qp, reset, pb, pr)
        got = _pictures(kind, enc.reconstruct(h, w))
        want = _pictures(kind, dec.decompress(bs, qp, h, w, ec, reset))
        torch.cuda.synchronize()
        assert got.shape == want.shape == ((1 if kind == "ld" else 8), 3, h + pb, w + pr)
        assert torch.equal(got, want), (i, qp, reset)
        # the decoder holds that unit's feature_p too: its own reconstruct gives its own pictures
        assert torch.equal(_pictures(kind, dec.reconstruct(h, w)), want), i


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_reconstruct_leaves_no_trace(kind, graphs):
    h, w = 144, 176
    pb, pr = -h % 16, -w % 16
    ref = _ref(h, w)
    xs = [_x(kind, h, w, i) for i in range(len(PLAN))]
    a, b, dec_a, dec_b, c = (_proxy(kind, graphs) for _ in range(5))
    for rep in range(2):                                             # a second GOP re-enters the stages behind add_ref
        for o in (a, b):
            o.add_ref_feature_from_frame(ref, True)
        for o in (dec_a, dec_b):
            o.add_ref_feature_from_frame(ref, False)
        for i, (qp, reset) in enumerate(PLAN):
            bs_a, ec_a = a.compress(xs[i], qp, reset, pb, pr)
            bs_b, ec_b = b.compress(xs[i], qp, reset, pb, pr)
            assert np.array_equal(bs_a, bs_b) and ec_a == ec_b, (rep, i)
            if i == 3:
                a.estimate_bits(xs[(i + 1) % len(xs)], 50, pb, pr)   # a size probe between compress and reconstruct
            r1 = _pictures(kind, a.reconstruct(h, w))
            if i == 1:
                assert torch.equal(_pictures(kind, a.reconstruct(h, w)), r1), "the same reconstruction twice in a row"
            assert np.array_equal(a._stream_bytes(), bs_b), "reconstruct replaced the stream of the last compress"
            state_a, state_b = a.export_state(), b.export_state()
            assert torch.equal(state_a, state_b), (rep, i)
            d_a = _pictures(kind, dec_a.decompress(bs_a, qp, h, w, ec_a, reset))
            d_b = _pictures(kind, dec_b.decompress(bs_b, qp, h, w, ec_b, reset))
            torch.cuda.synchronize()
            assert torch.equal(d_a, d_b) and torch.equal(r1, d_b), (rep, i)
            assert torch.equal(dec_a.export_state(), dec_b.export_state())
            if i in (2, 4):
                # hand-off: an object that imported a's state gives a's pictures, and its state stays the imported one
                c.import_state(state_a, h, w)
                assert torch.equal(_pictures(kind, c.reconstruct(h, w)), r1), (rep, i)
                assert torch.equal(c.export_state(), state_a)
            if i == 2:
                dec_a.reconstruct(h, w)                              # ... and a decoder that reconstructs decodes on as one that does not


@pytest.mark.parametrize("kind", ["hts", "htl"])
def test_reconstruct_gives_all_8_pictures_whatever_the_mask(kind):
    h, w = 144, 176
    pb, pr = -h % 16, -w % 16
    enc, dec = _proxy(kind), _proxy(kind)
    enc.add_ref_feature_from_frame(_ref(h, w), True)
    dec.add_ref_feature_from_frame(_ref(h, w), False)
    bs, ec = enc.compress(_x(kind, h, w, 0), 30, False, pb, pr)
    want = _pictures(kind, dec.decompress(bs, 30, h, w, ec, False))
    state = dec.export_state().clone()
    dec.set_recon_mask(0x85)
    got = dec.reconstruct(h, w)
    assert torch.equal(_pictures(kind, got), want)
    assert torch.equal(dec.export_state(), state)
    enc.set_recon_mask(0x80)
    assert torch.equal(_pictures(kind, enc.reconstruct(h, w)), want)


@pytest.mark.parametrize("kind", KINDS)
def test_reconstruct_refusals(kind):
    h, w = 144, 176
    pb, pr = -h % 16, -w % 16
    from inference_extensions_cuda import _HT, _LD
    fn = (_LD if kind == "ld" else _HT)["reconstruct"]
    name = "dcvc_dmcld_reconstruct" if kind == "ld" else "dcvc_dmcht_reconstruct"
    p = _proxy(kind)
    with pytest.raises(_lib.DcvcError, match="reconstruct: no feature_p yet"):
        p.reconstruct(h, w)                                          # a fresh object with parameters
    for adaptor in (True, False):
        p.add_ref_feature_from_frame(_ref(h, w), adaptor)
        before = p.export_state().clone()
        with pytest.raises(_lib.DcvcError, match="reconstruct: no feature_p yet"):
            p.reconstruct(h, w)                                      # right behind add_ref
        assert torch.equal(p.export_state(), before)
    with pytest.raises(_lib.DcvcError, match=name + ": null"):
        _lib.check(fn(p._h, None, None))
    assert torch.equal(p.export_state(), before)
    # no parameters set: an object of its own, straight from the C ABI
    import inference_extensions_cuda as ext
    bare = (ext.DMCLDProxy if kind == "ld" else ext.DMCHTSProxy if kind == "hts" else ext.DMCHTLProxy)()
    buf = torch.zeros(16, dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.DcvcError, match="reconstruct: set_param"):
        _lib.check(fn(bare._h, ctypes.c_void_p(buf.data_ptr()), None))
    assert not buf.any()
    # ... and the refused object goes on as one that was never asked
    q = _proxy(kind)
    q.add_ref_feature_from_frame(_ref(h, w), True)
    p.add_ref_feature_from_frame(_ref(h, w), True)
    x = _x(kind, h, w, 0)
    assert np.array_equal(p.compress(x, 40, False, pb, pr)[0], q.compress(x, 40, False, pb, pr)[0])
    assert torch.equal(_pictures(kind, p.reconstruct(h, w)), _pictures(kind, q.reconstruct(h, w)))
