"""The size probe on a real MI355X (-m gpu), DESIGN.md 15:

  * kernels: dcvc_code_length_y / _z equal the numpy gather-and-sum exactly (integer sums), uncompacted (symbols + keep
    flags) and compacted (symbols + device totals), counts that are not multiples of 2048, none, all skipped, a batch of 3;
  * probe against product: DMCIProxy.estimate_bits equals the numpy sum over the symbols compress() leaves on the device
    (dcvc_dmci_debug_read), and the predicted bytes stand to len(stream) within the bound of test_code_length_cpu.py;
  * the probe leaves no trace: compress(A); estimate(B, another qp, another size); compress(A) gives the first call's
    bytes and x_hat, graphs on and off; a batch probe of N equals N single probes."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from codec_util import dmci_model, picture
from dcvc_amd import _lib, rate_control

sys.path.insert(0, os.path.dirname(__file__))
import code_length_np as cl  # noqa: E402
from test_code_length_cpu import R_BOUND, native_table  # noqa: E402

pytestmark = pytest.mark.gpu

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


def _p(t):
    return _vp(t.data_ptr()) if t is not None else None


def _stream():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "rans_golden.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ kernels
def _symbols(rng, count, num_cdf=128):
    sym = rng.integers(-8, 9, count)
    big = rng.random(count) < 0.05
    sym[big] = rng.integers(-128, 128, int(big.sum()))
    idx = rng.integers(0, num_cdf, count)
    return ((sym << 8) + idx).astype(np.int16)


@pytest.mark.parametrize("count,n", [(0, 1), (1, 1), (7, 1), (2048, 1), (4099, 1), (70001, 1), (2048 * 1024 + 13, 1),
                                      (4104, 3), (70000, 3)])
@pytest.mark.parametrize("keep_mode", ["random", "none", "all", "no_flags"])
def test_code_length_y_uncompacted(count, n, keep_mode):
    f = _lib.fn("dcvc_code_length_y", _ci, [_vp, _ll, _vp, _ll, _vp, _ci, _ci, _ci, _vp, _ci, _vp, _ci, _vp])
    g = _golden()
    ty = native_table(g["y_cdf"], g["y_len"], 256)
    rng = np.random.default_rng(count + n)
    # picture stride: a multiple of 8 symbols, so that every picture's flags start at a byte
    stride = (count + 7) // 8 * 8
    comb = np.zeros((n, max(stride, 8)), dtype=np.int16)
    keep = np.zeros((n, max(stride, 8)), dtype=bool)
    for b in range(n):
        comb[b, :count] = _symbols(rng, count)
        keep[b, :count] = {"random": rng.random(count) < 0.4, "none": np.zeros(count, bool)}.get(keep_mode, np.ones(count, bool))
    cond = np.packbits(keep, axis=1, bitorder="little")
    d_sym, d_cond, d_table = _dev(comb), _dev(cond), _dev(ty)
    out = torch.full((n, 2), 12345, dtype=torch.int64, device="cuda")        # the call zeroes it
    use_flags = keep_mode != "no_flags"
    _lib.check(f(_p(d_sym), comb.shape[1], _p(d_cond) if use_flags else None, cond.shape[1], None, 0, 0, count, _p(d_table),
                 ty.shape[0], _p(out), n, _stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b in range(n):
        want = cl.sum_y(ty, comb[b, :count], keep[b, :count] if use_flags else None)
        assert (int(got[b, 0]), int(got[b, 1])) == want, (b, got[b], want)


@pytest.mark.parametrize("n", [1, 3])
def test_code_length_y_compacted_with_device_totals(n):
    """the layout the codec uses: picture b's kept symbols of four steps back to back, their counts in totals[4 b ..]"""
    f = _lib.fn("dcvc_code_length_y", _ci, [_vp, _ll, _vp, _ll, _vp, _ci, _ci, _ci, _vp, _ci, _vp, _ci, _vp])
    g = _golden()
    ty = native_table(g["y_cdf"], g["y_len"], 256)
    rng = np.random.default_rng(n)
    cap = 40000
    comb = np.stack([_symbols(rng, cap) for _ in range(n)])                   # beyond the totals: stale symbols, not counted
    totals = np.array([[5000, 0, 12345, 3001], [0, 0, 0, 0], [10000, 10000, 10000, 10000]], dtype=np.int32)[:n]
    out = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    d_sym, d_tot, d_table = _dev(comb), _dev(totals), _dev(ty)
    _lib.check(f(_p(d_sym), cap, None, 0, _p(d_tot), 4, 4, cap, _p(d_table), ty.shape[0], _p(out), n, _stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for b in range(n):
        used = int(totals[b].sum())
        assert (int(got[b, 0]), int(got[b, 1])) == cl.sum_y(ty, comb[b, :used]), b
        # ... and the same number as the uncompacted form gives for the same symbols
    keep = np.zeros((1, cap), dtype=bool)
    keep[0, ::3] = True
    packed = comb[0][keep[0]]
    flat = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    d_packed, d_cond = _dev(np.concatenate([packed, np.zeros(8, np.int16)])), _dev(np.packbits(keep, axis=1, bitorder="little"))
    _lib.check(f(_p(d_sym), cap, _p(d_cond), cap // 8, None, 0, 0, cap, _p(d_table), ty.shape[0], _p(out[:1]), 1, _stream()))
    _lib.check(f(_p(d_packed), 0, None, 0, None, 0, 0, packed.size, _p(d_table), ty.shape[0], _p(flat), 1, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[:1], flat) and int(flat[0, 1]) == packed.size


@pytest.mark.parametrize("count,n", [(0, 1), (128, 1), (128 * 5 + 3, 1), (128 * 510, 1), (128 * 35, 3)])
def test_code_length_z(count, n):
    f = _lib.fn("dcvc_code_length_z", _ci, [_vp, _ci, _ci, _vp, _vp, _ci, _vp])
    g = _golden()
    tz = native_table(g["z_cdf"], g["z_len"], 128)
    rng = np.random.default_rng(count + n)
    z = rng.integers(-64, 64, (n, max(count, 1))).astype(np.int8)
    rows = tz[128:256]
    d_z, d_rows = _dev(z[:, :count] if count else z), _dev(rows)
    out = torch.full((n,), 777, dtype=torch.int64, device="cuda")
    _lib.check(f(_p(d_z), count, 128, _p(d_rows), _p(out), n, _stream()))
    torch.cuda.synchronize()
    for b in range(n):
        assert int(out[b]) == cl.sum_z(rows, z[b, :count], 128), b


def test_kernel_refusals():
    f = _lib.fn("dcvc_code_length_y", _ci, [_vp, _ll, _vp, _ll, _vp, _ci, _ci, _ci, _vp, _ci, _vp, _ci, _vp])
    t = torch.zeros(4096, dtype=torch.int16, device="cuda")
    tab = torch.zeros((128, 256), dtype=torch.int32, device="cuda")
    out = torch.zeros(2, dtype=torch.int64, device="cuda")
    ok = [_p(t), 0, None, 0, None, 0, 0, 64, _p(tab), 128, _p(out), 1, _stream()]
    assert f(*ok) == 0
    for pos, bad in [(0, None), (0, _vp(t.data_ptr() + 2)), (8, None), (9, 0), (9, 257), (10, None), (11, 0), (7, -1)]:
        args = list(ok)
        args[pos] = bad
        assert f(*args) < 0, (pos, bad)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the probe
def _proxy(thres, graphs):
    m = dmci_model(skip_thres=thres)
    g = copy.deepcopy(m).half().cuda()
    g.proxy = None
    p = g._ensure_proxy()
    p.set_use_graphs(graphs)
    return p, m


def _x(h, w, index):
    return torch.from_numpy(picture(h, w, index=index)).permute(2, 0, 1)[None].cuda().contiguous(memory_format=torch.channels_last)


def _padding(h, w):
    return (h + 15) // 16 * 16 - h, (w + 15) // 16 * 16 - w


def _tables(model):
    z_cdf, z_len, y_cdf, y_len = model.get_cdf_info()
    return native_table(np.asarray(y_cdf), np.asarray(y_len), 256), native_table(np.asarray(z_cdf), np.asarray(z_len), 128)


@pytest.mark.parametrize("h,w", [(256, 384), (240, 424)])          # 240 x 424: 15 x 27 latent rows, padded to 16 x 28
@pytest.mark.parametrize("qp", [0, 21, 42, 63])
def test_probe_equals_the_symbols_compress_codes(h, w, qp):
    p, model = _proxy(0.15, True)
    ty, tz = _tables(model)
    x = _x(h, w, 2)
    pb, pr = _padding(h, w)
    y_units, z_units, symbols = p.estimate_bits(x, qp, pb, pr)
    bs, _, ec = p.compress(x, qp, pb, pr)
    torch.cuda.synchronize()
    totals = p.debug_read("totals", np.int32)[:4]
    comp = p.debug_read("symbols", np.int16)[:int(totals.sum())]
    z = p.debug_read("z_i8", np.int8)
    assert symbols == int(totals.sum())
    assert (y_units, symbols) == cl.sum_y(ty, comp)
    assert z_units == cl.sum_z(tz[qp * 128:(qp + 1) * 128], z, 128)
    assert ec == rate_control.ec_parallel_for(symbols)
    ideal = (y_units + z_units) / cl.UNIT
    coded, fixed = 8 * len(bs), rate_control.stream_fixed_bits(ec)
    predicted = rate_control.predicted_stream_bytes(y_units, z_units, ec)
    print("%dx%d q %2d: %6d symbols, %d sub-streams, ideal %.1f bits, coded %d, predicted %d bytes, stream %d bytes"
          % (w, h, qp, symbols, ec, ideal, coded, predicted, len(bs)))
    assert coded >= ideal
    assert coded <= ideal + fixed + R_BOUND * ideal
    assert 8 * predicted >= ideal + fixed > 8 * (predicted - 1)
    # the probe after the compress: the same numbers again
    assert p.estimate_bits(x, qp, pb, pr) == (y_units, z_units, symbols)


@pytest.mark.parametrize("graphs", [True, False])
def test_probe_leaves_no_trace(graphs):
    h, w, qp = 256, 384, 30
    a, b = _x(h, w, 1), _x(240, 424, 5)
    pb, pr = _padding(h, w)
    fresh, _ = _proxy(0.15, graphs)
    bs0, xh0, ec0 = fresh.compress(a, qp, pb, pr)
    bs0, xh0 = bs0.copy(), xh0.clone()
    torch.cuda.synchronize()

    p, _ = _proxy(0.15, graphs)
    for rep in range(4):                    # graphs: eager, captured, replayed - with probes in between at every stage
        bs, xh, ec = p.compress(a, qp, pb, pr)
        torch.cuda.synchronize()
        assert np.array_equal(bs, bs0) and ec == ec0 and torch.equal(xh, xh0), rep
        want_dec = p.decompress(bs0, qp, h, w, ec0).clone()
        p.estimate_bits(b, 55, *_padding(240, 424))          # another picture, another qp, another size
        p.estimate_bits(a, 3, pb, pr)                        # the same size, another qp
        if rep == 2:
            p.estimate_bits_batch(torch.cat([a, a]), 40, pb, pr)
        d = p.decompress(bs0, qp, h, w, ec0)
        torch.cuda.synchronize()
        assert torch.equal(d, want_dec) and torch.equal(d, xh0), rep
    # a probe behind a compress: the object still holds that compress's stream
    p.compress(a, qp, pb, pr)
    p.estimate_bits(b, 9, *_padding(240, 424))
    assert np.array_equal(p._stream_bytes(), bs0)


@pytest.mark.parametrize("graphs", [True, False])
def test_batch_probe_equals_single_probes(graphs):
    h, w, qp, n = 240, 424, 37, 3
    xs = torch.cat([_x(h, w, 3 * i + 1) for i in range(n)]).contiguous(memory_format=torch.channels_last)
    pb, pr = _padding(h, w)
    p, _ = _proxy(0.15, graphs)
    want = [p.estimate_bits(xs[i:i + 1], qp, pb, pr) for i in range(n)]
    assert len({wv[0] for wv in want}) == n                  # distinct pictures, distinct sizes
    for rep in range(3):
        assert p.estimate_bits_batch(xs, qp, pb, pr) == want, rep
    assert [p.estimate_bits(xs[i:i + 1], qp, pb, pr) for i in range(n)] == want


def test_probe_refusals():
    p, _ = _proxy(0.15, True)
    x = _x(64, 64, 0)
    with pytest.raises(_lib.DcvcError):
        p.estimate_bits(x, 64, 0, 0)
    with pytest.raises(_lib.DcvcError):
        p.estimate_bits(x, -1, 0, 0)
    with pytest.raises(_lib.DcvcError):
        p.estimate_bits(x, 10, 1, 0)
    from inference_extensions_cuda import _F
    with pytest.raises(_lib.DcvcError):
        _lib.check(_F["estimate_symbols"](p._h, 0))          # no probe yet
    p.estimate_bits(x, 10, 0, 0)
    with pytest.raises(_lib.DcvcError):
        _lib.check(_F["estimate_symbols"](p._h, 1))
