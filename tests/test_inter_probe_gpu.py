"""The size probe of the inter codecs on a real MI355X (-m gpu), DESIGN.md 7 and 15: DMCLDProxy / DMCHTSProxy /
DMCHTLProxy.estimate_bits.

  * probe equals product: the probe's sums equal the numpy sums over the symbols, totals and z a compress at that q_index
    leaves on the device (integer equality), and the prediction stands to len(stream) within the bound of
    test_code_length_cpu.py;
  * no trace: an object that probes between its compress calls - other q_indexes, other pictures, several in a row, one
    right behind add_ref - writes the streams, holds the temporal state and feeds a decoder exactly as one that never
    probes, with graphs and without (LD: its first stage used to scale the temporal prior in place and run the fusion
    chain over it; that buffer is state, and a probe would have consumed it);
  * refusals, with the temporal state untouched."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from codec_util import chunk, dmc_ht_model, dmc_ld_model, picture, to_device_input
from dcvc_amd import _lib, rate_control

sys.path.insert(0, os.path.dirname(__file__))
import code_length_np as cl  # noqa: E402
from test_code_length_cpu import R_BOUND, native_table  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["ld", "hts", "htl"]


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


def _padding(h, w):
    return -h % 16, -w % 16


def _tables(kind):
    z_cdf, z_len, y_cdf, y_len = _model(kind).get_cdf_info()
    return native_table(np.asarray(y_cdf), np.asarray(y_len), 256), native_table(np.asarray(z_cdf), np.asarray(z_len), 128)


def _pictures(kind, d):
    return (d if kind == "ld" else torch.cat(list(d), 0)).clone()


@pytest.mark.parametrize("h,w", [(144, 176), (240, 424)])          # 240 x 424: 15 x 27 latent rows, padded to 16 x 28
@pytest.mark.parametrize("kind", KINDS)
def test_probe_equals_the_symbols_compress_codes(kind, h, w):
    p = _proxy(kind)
    ty, tz = _tables(kind)
    pb, pr = _padding(h, w)
    ref, x0, x1 = _ref(h, w), _x(kind, h, w, 0), _x(kind, h, w, 1)
    groups = 4 if kind == "htl" else 1
    for qp in (0, 21, 42, 63):
        p.add_ref_feature_from_frame(ref, True)
        p.compress(x0, 30, False, pb, pr)                            # one P unit: the state is that of a running GOP
        y_units, z_units, symbols = p.estimate_bits(x1, qp, pb, pr)
        assert p.estimate_bits(x1, qp, pb, pr) == (y_units, z_units, symbols)      # the same probe twice
        bs, ec = p.compress(x1, qp, False, pb, pr)
        torch.cuda.synchronize()
        totals = p.debug_read("totals", np.int32)[:groups]
        comp = p.debug_read("symbols", np.int16)[:int(totals.sum())]
        z = p.debug_read("z_i8", np.int8)
        assert symbols == int(totals.sum())
        assert (y_units, symbols) == cl.sum_y(ty, comp)
        assert z_units == cl.sum_z(tz[qp * 128:(qp + 1) * 128], z, 128)
        assert ec == rate_control.ec_parallel_for(symbols)
        ideal = (y_units + z_units) / cl.UNIT
        coded, fixed = 8 * len(bs), rate_control.stream_fixed_bits(ec)
        predicted = rate_control.predicted_stream_bytes(y_units, z_units, ec)
        print("%s %dx%d q %2d: %6d symbols, %d sub-streams, ideal %.1f bits, coded %d, predicted %d bytes, stream %d bytes"
              % (kind, w, h, qp, symbols, ec, ideal, coded, predicted, len(bs)))
        assert coded >= ideal
        assert coded <= ideal + fixed + R_BOUND * ideal
        assert 8 * predicted >= ideal + fixed > 8 * (predicted - 1)


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_probe_leaves_no_trace(kind, graphs):
    h, w = 144, 176
    pb, pr = _padding(h, w)
    plan = [(30, 0), (30, 0), (45, 1), (45, 0), (12, 0), (12, 0)]       # a reset and two q changes; graphs: eager, captured, replayed
    ref = _ref(h, w)
    xs = [_x(kind, h, w, i) for i in range(len(plan))]
    a, b, dec_a, dec_b = (_proxy(kind, graphs) for _ in range(4))
    for rep in range(2):                                             # a second GOP re-enters the stages behind add_ref
        for o in (a, b):
            o.add_ref_feature_from_frame(ref, True)
        for o in (dec_a, dec_b):
            o.add_ref_feature_from_frame(ref, False)
        first = a.estimate_bits(xs[0], 50, pb, pr)                   # directly behind add_ref
        assert torch.equal(a.export_state(), b.export_state()), "a probe behind add_ref changed the temporal state"
        last = None
        for i, (qp, reset) in enumerate(plan):
            # another q_index, another picture, several in a row
            e1 = a.estimate_bits(xs[i], (qp + 17) % 64, pb, pr)
            a.estimate_bits(xs[(i + 2) % len(xs)], qp, pb, pr)
            a.estimate_bits(xs[(i + 3) % len(xs)], 63 - qp, pb, pr)
            assert a.estimate_bits(xs[i], (qp + 17) % 64, pb, pr) == e1, "the same probe twice"
            if last is not None:
                assert np.array_equal(a._stream_bytes(), last), "a probe replaced the stream of the last compress"
            if i == 0:
                assert a.estimate_bits(xs[0], 50, pb, pr) == first
            want = a.estimate_bits(xs[i], qp, pb, pr)
            bs_a, ec_a = a.compress(xs[i], qp, reset, pb, pr)
            bs_b, ec_b = b.compress(xs[i], qp, reset, pb, pr)
            last = bs_a.copy()
            assert np.array_equal(bs_a, bs_b) and ec_a == ec_b, (rep, i)
            assert ec_a == rate_control.ec_parallel_for(want[2])
            a.estimate_bits(xs[(i + 1) % len(xs)], 5, pb, pr)        # ... and one behind the compress
            assert np.array_equal(a._stream_bytes(), last)
            assert torch.equal(a.export_state(), b.export_state()), (rep, i)
            d_a = _pictures(kind, dec_a.decompress(bs_a, qp, h, w, ec_a, reset))
            d_b = _pictures(kind, dec_b.decompress(bs_b, qp, h, w, ec_b, reset))
            torch.cuda.synchronize()
            assert torch.equal(d_a, d_b), (rep, i)
            assert torch.equal(dec_a.export_state(), dec_b.export_state())


@pytest.mark.parametrize("kind", KINDS)
def test_probe_refusals(kind):
    h, w = 144, 176
    pb, pr = _padding(h, w)
    p = _proxy(kind)
    x = _x(kind, h, w, 0)
    with pytest.raises(_lib.DcvcError, match="reference feature"):
        p.estimate_bits(x, 20, pb, pr)                               # a fresh object
    p.add_ref_feature_from_frame(_ref(h, w), False)                  # the decoder's call: no encoder-side state
    with pytest.raises(_lib.DcvcError, match="reference feature"):
        p.estimate_bits(x, 20, pb, pr)
    p.add_ref_feature_from_frame(_ref(h, w), True)
    p.compress(x, 30, False, pb, pr)
    before = p.export_state().clone()
    stream = p._stream_bytes().copy()
    other = _x(kind, 64, 64, 0)
    with pytest.raises(_lib.DcvcError, match="picture size"):
        p.estimate_bits(other, 20, 0, 0)                             # prepare() would have dropped the temporal state
    for qp in (64, -1):
        with pytest.raises(_lib.DcvcError, match="qp"):
            p.estimate_bits(x, qp, pb, pr)
    with pytest.raises(_lib.DcvcError, match="padding"):
        p.estimate_bits(x, 20, pb + 1, pr)
    from inference_extensions_cuda import _HT, _LD
    with pytest.raises(_lib.DcvcError):
        _lib.check((_LD if kind == "ld" else _HT)["estimate_symbols"](p._h))      # every refused probe cleared it
    assert torch.equal(p.export_state(), before)
    assert np.array_equal(p._stream_bytes(), stream)
    # ... and the object goes on as one that was never asked
    q = _proxy(kind)
    q.add_ref_feature_from_frame(_ref(h, w), True)
    q.compress(x, 30, False, pb, pr)
    x1 = _x(kind, h, w, 1)
    assert p.estimate_bits(x1, 40, pb, pr) == q.estimate_bits(x1, 40, pb, pr)
    assert np.array_equal(p.compress(x1, 40, False, pb, pr)[0], q.compress(x1, 40, False, pb, pr)[0])
