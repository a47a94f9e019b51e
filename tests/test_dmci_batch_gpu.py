"""Intra batches on a real MI355X (-m gpu): N pictures per DMCI call give exactly what N single calls give.

  * kernels: every batched `_b` entry point of include/dcvc_amd_ops.h equals N single launches bit for bit, on per-picture
    geometries with odd row counts (H16 = 45, H64 = 17, H = 15), where stacking the pictures as one taller one would not
    (the symbol steps' dcvc_y_step_enc_b / _dec_index_b / _dec_restore_b: tests/test_symbols_edges_gpu.py::test_batches);
  * codec: DMCIProxy.compress_batch gives the streams, ec_parallel and x_hat of single compress() calls on a fresh object,
    decompress_batch the x_hat of single decompress() calls; with and without graphs, skip_thres 0 and 0.15; a single call
    behind a batch call gives what a fresh object gives;
  * ABI: dcvc_dmci_compress_batch / _get_stream_at / _decompress_batch refuse what include/dcvc_amd_codec.h lists."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from codec_util import dmci_model, picture

pytestmark = pytest.mark.gpu

_vp, _ci = ctypes.c_void_p, ctypes.c_int


def _lib():
    from dcvc_amd import _lib as lib
    return lib


def _p(t):
    return _vp(t.data_ptr())


def _stream():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _check(rc):
    lib = _lib()
    assert rc == 0, lib.lib().dcvc_last_error().decode()


def _fn(name, args):
    return _lib().fn(name, _ci, args)


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) - 0.5).half().cuda()


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("H,W,C", [(15, 26, 128), (45, 20, 192)])
def test_dwconv3x3_b(n, H, W, C):
    f = _fn("dcvc_dwconv3x3_b", [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp])
    x, w = _rand((n, H, W, C), 1), _rand((9, C), 2)
    got, want = torch.full_like(x, 7), torch.full_like(x, 7)
    _check(f(_p(x), C, _p(w), _p(got), C, H, W, C, n, _stream()))
    for b in range(n):
        _check(f(_p(x[b]), C, _p(w), _p(want[b]), C, H, W, C, 1, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("k,s,p,in_h,in_w,cin,cout", [(3, 2, 1, 90, 20, 128, 64), (2, 2, 0, 34, 12, 128, 128)])
def test_conv_kxk_b(n, k, s, p, in_h, in_w, cin, cout):
    f = _fn("dcvc_conv_kxk_b", [_vp, _ci, _vp, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _vp])
    oh, ow = (in_h + 2 * p - k) // s + 1, (in_w + 2 * p - k) // s + 1
    x, w, bias = _rand((n, in_h, in_w, cin), 3), _rand((cout, k, k, cin), 4) * 0.1, _rand((cout,), 5)
    got, want = torch.zeros((n, oh, ow, cout), dtype=torch.half, device="cuda"), torch.ones((n, oh, ow, cout), dtype=torch.half, device="cuda")
    _check(f(_p(x), cin, _p(w), _p(bias), _p(got), cout, in_h, in_w, cin, cout, k, s, p, n, _stream()))
    for b in range(n):
        _check(f(_p(x[b]), cin, _p(w), _p(bias), _p(want[b]), cout, in_h, in_w, cin, cout, k, s, p, 1, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("n", [2, 3])
def test_tconv2x2_b(n):
    f = _fn("dcvc_tconv2x2_b", [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp])
    H, W, cin, cout = 17, 6, 128, 128
    x, w = _rand((n, H, W, cin), 6), _rand((4, cout, cin), 7) * 0.1
    got, want = torch.zeros((n, 2 * H, 2 * W, cout), dtype=torch.half, device="cuda"), torch.ones((n, 2 * H, 2 * W, cout), dtype=torch.half, device="cuda")
    _check(f(_p(x), cin, _p(w), _p(got), cout, H, W, cin, cout, n, _stream()))
    for b in range(n):
        _check(f(_p(x[b]), cin, _p(w), _p(want[b]), cout, H, W, cin, cout, 1, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


@pytest.mark.parametrize("n", [2, 3])
def test_layout_b(n):
    stream = _stream()
    # pad + unshuffle: a 117 x 70 picture -> 16 x 10 blocks of 8 x 8 (replicated bottom / right edges of EACH picture)
    f = _fn("dcvc_pad_unshuffle8_b", [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _vp])
    x = _rand((n, 117, 70, 3), 8)
    got, want = torch.zeros((n, 16, 10, 192), dtype=torch.half, device="cuda"), torch.ones((n, 16, 10, 192), dtype=torch.half, device="cuda")
    _check(f(_p(x), 117, 70, 3, _p(got), 16, 10, n, stream))
    for b in range(n):
        _check(f(_p(x[b]), 117, 70, 3, _p(want[b]), 16, 10, 1, stream))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # shuffle + clamp: 15 x 6 blocks
    f = _fn("dcvc_shuffle8_b", [_vp, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _vp])
    x = _rand((n, 15, 6, 192), 9) * 3
    got, want = torch.zeros((n, 120, 48, 3), dtype=torch.half, device="cuda"), torch.ones((n, 120, 48, 3), dtype=torch.half, device="cuda")
    _check(f(_p(x), 192, 15, 6, 3, 1, _p(got), n, stream))
    for b in range(n):
        _check(f(_p(x[b]), 192, 15, 6, 3, 1, _p(want[b]), 1, stream))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # replicate pad: H16 = 45 -> 48, 20 -> 24
    f = _fn("dcvc_replicate_pad_b", [_vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _ci, _ci, _vp])
    x = _rand((n, 45, 20, 256), 10)
    got, want = torch.zeros((n, 48, 24, 256), dtype=torch.half, device="cuda"), torch.ones((n, 48, 24, 256), dtype=torch.half, device="cuda")
    _check(f(_p(x), 256, 45, 20, 256, 3, 4, _p(got), 256, n, stream))
    for b in range(n):
        _check(f(_p(x[b]), 256, 45, 20, 256, 3, 4, _p(want[b]), 256, 1, stream))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # crop: 48 x 24 -> 45 x 20
    f = _fn("dcvc_crop_b", [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _vp])
    x = _rand((n, 48, 24, 512), 11)
    got, want = torch.zeros((n, 45, 20, 512), dtype=torch.half, device="cuda"), torch.ones((n, 45, 20, 512), dtype=torch.half, device="cuda")
    _check(f(_p(x), 512, 48, 24, _p(got), 512, 45, 20, 512, n, stream))
    for b in range(n):
        _check(f(_p(x[b]), 512, 48, 24, _p(want[b]), 512, 45, 20, 512, 1, stream))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_kernel_b_refusals():
    f = _fn("dcvc_dwconv3x3_b", [_vp, _ci, _vp, _vp, _ci, _ci, _ci, _ci, _ci, _vp])
    x = torch.zeros((2, 4, 4, 64), dtype=torch.half, device="cuda")
    for n in (0, 17):
        assert f(_p(x), 64, _p(x), _p(x), 64, 4, 4, 64, n, _stream()) < 0
    assert f(None, 64, _p(x), _p(x), 64, 4, 4, 64, 2, _stream()) < 0
    assert f(_p(x), 64, _p(x), _p(x), 64, 0, 4, 64, 2, _stream()) < 0
    f = _fn("dcvc_crop_b", [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _ci, _ci, _ci, _vp])
    assert f(_p(x), 64, 4, 4, _p(x), 64, 5, 4, 64, 2, _stream()) < 0      # crop taller than its input
    f = _fn("dcvc_dcb_tail_b", [_vp, _vp, _vp, _ci, _vp, _vp, _ci] + [_vp] * 9 + [_ci] * 8 + [_vp])
    z = torch.zeros((2 * 16, 512), dtype=torch.half, device="cuda")
    y = torch.full((2 * 16, 256), 7.0, dtype=torch.half, device="cuda")
    ws = [_p(z)] * 6                       # w3, b3, w0, b0, w2, b2

    def tail_b(n, t=_p(z), x=_p(z), ldx=256, Hh=4, w1=None, b1=None, dw=None):
        return f(w1, b1, t, 128, dw, x, ldx, *ws, None, None, _p(y), 256, Hh, 4, 256, 128, 128, 0, n, _stream())
    for n in (0, 17):
        assert tail_b(n) < 0
    assert tail_b(2, t=None) < 0                                            # neither dc.0's output nor its weights
    assert tail_b(2, x=None) < 0
    assert tail_b(2, Hh=0) < 0
    assert tail_b(2, ldx=128) < 0                                           # leading dimension below c
    assert tail_b(2, w1=_p(z), b1=_p(z)) < 0                                # dc.0 inside without the depthwise taps
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ------------------------------------------------------------------------------------------------ codec
def _proxy(thres, graphs):
    g = copy.deepcopy(dmci_model(skip_thres=thres)).half().cuda()
    g.proxy = None
    p = g._ensure_proxy()
    p.set_use_graphs(graphs)
    return p


def _pictures(h, w, n):
    x = np.stack([picture(h, w, index=3 * i + 1) for i in range(n)])          # distinct pictures
    return torch.from_numpy(x).permute(0, 3, 1, 2).cuda().contiguous(memory_format=torch.channels_last)


def _padding(h, w):
    return (h + 15) // 16 * 16 - h, (w + 15) // 16 * 16 - w


@pytest.mark.parametrize("h,w,n,graphs,thres,qp", [
    (240, 416, 1, True, 0.15, 32),
    (240, 416, 3, False, 0.0, 0),
    (240, 416, 8, True, 0.15, 63),
    (720, 1280, 3, True, 0.0, 32),
    (1080, 1920, 2, False, 0.15, 20),
    (2160, 3840, 2, True, 0.15, 40),
])
def test_batch_equals_single_calls(h, w, n, graphs, thres, qp):
    x = _pictures(h, w, n)
    pb, pr = _padding(h, w)
    single = _proxy(thres, graphs)
    want = []
    for i in range(n):
        bs, xh, ec = single.compress(x[i:i + 1], qp, pb, pr)
        want.append((bs.copy(), xh.clone(), ec))
    torch.cuda.synchronize()
    want_dec = []
    for bs, _, ec in want:
        want_dec.append(single.decompress(bs, qp, h, w, ec).clone())
    torch.cuda.synchronize()

    batch = _proxy(thres, graphs)
    # graphs: the first call runs eagerly, the second captures, the third replays - all three must agree
    for rep in range(3 if graphs else 1):
        got = batch.compress_batch(x, qp, pb, pr)
        torch.cuda.synchronize()
        assert len(got) == n
        for i, (bs, xh, ec) in enumerate(got):
            assert ec == want[i][2], (rep, i)
            assert np.array_equal(bs, want[i][0]), "picture %d: stream differs (call %d)" % (i, rep)
            assert torch.equal(xh, want[i][1]), "picture %d: x_hat differs (call %d)" % (i, rep)
        dec = batch.decompress_batch([g[0] for g in got], qp, h, w, [g[2] for g in got])
        torch.cuda.synchronize()
        assert dec.shape[0] == n
        for i in range(n):
            assert torch.equal(dec[i:i + 1], want_dec[i]), "picture %d: decoded x_hat differs (call %d)" % (i, rep)
            assert torch.equal(dec[i:i + 1], want[i][1])

    # a single call behind the batch calls: what the fresh object gave
    bs, xh, ec = batch.compress(x[n - 1:n], qp, pb, pr)
    torch.cuda.synchronize()
    assert np.array_equal(bs, want[n - 1][0]) and ec == want[n - 1][2] and torch.equal(xh, want[n - 1][1])
    d = batch.decompress(want[0][0], qp, h, w, want[0][2])
    torch.cuda.synchronize()
    assert torch.equal(d, want_dec[0])


def test_mixed_batch_sizes_on_one_object():
    """batch sizes change from call to call on one object (a short last batch), graphs on"""
    h, w, qp = 240, 416, 25
    pb, pr = _padding(h, w)
    x = _pictures(h, w, 5)
    single = _proxy(0.15, True)
    want = [single.compress(x[i:i + 1], qp, pb, pr)[0].copy() for i in range(5)]
    p = _proxy(0.15, True)
    for lo, hi in [(0, 4), (4, 5), (0, 2), (0, 4), (1, 5)]:
        got = p.compress_batch(x[lo:hi], qp, pb, pr)
        for i, g in enumerate(got):
            assert np.array_equal(g[0], want[lo + i]), (lo, hi, i)


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_refusals():
    p = _proxy(0.15, False)
    from inference_extensions_cuda import _F          # (importable once a proxy exists: dcvc_amd.install_plugin)
    h, w = 64, 96
    x = _pictures(h, w, 2)
    x_hat = torch.empty((2, 3, h, w), dtype=torch.half, device="cuda").contiguous(memory_format=torch.channels_last)
    ec = (_ci * 16)()
    cb = _F["compress_batch"]
    for n in (0, 17, -1):
        assert cb(p._h, n, _p(x), h, w, 20, 0, 0, _p(x_hat), ec, _stream()) < 0
    assert cb(p._h, 2, None, h, w, 20, 0, 0, _p(x_hat), ec, _stream()) < 0
    assert cb(p._h, 2, _p(x), h, w, 20, 0, 0, None, ec, _stream()) < 0
    assert cb(p._h, 2, _p(x), h, w, 20, 0, 0, _p(x_hat), None, _stream()) < 0
    assert cb(p._h, 2, _p(x), h, w, 20, 16, 0, _p(x_hat), ec, _stream()) < 0        # wrong padding
    assert cb(None, 2, _p(x), h, w, 20, 0, 0, _p(x_hat), ec, _stream()) < 0
    # get_stream_at: only indexes of the last call
    assert _F["get_stream_at"](p._h, 0, None, 0) < 0                                # no call yet
    got = p.compress_batch(x, 20, 0, 0)
    torch.cuda.synchronize()
    for i in (-1, 2, 16):
        assert _F["get_stream_at"](p._h, i, None, 0) < 0
    assert _F["get_stream_at"](p._h, 1, None, 0) == got[1][0].size
    bs, _, _ = p.compress(x[:1], 20, 0, 0)
    assert _F["get_stream_at"](p._h, 1, None, 0) < 0                                # a single call has n = 1
    assert _F["get_stream_at"](p._h, 0, None, 0) == bs.size == _F["get_stream"](p._h, None, 0)
    # decompress_batch
    db = _F["decompress_batch"]
    streams = [g[0] for g in got]
    ptrs = (_vp * 2)(*[s.ctypes.data for s in streams])
    sizes = (ctypes.c_size_t * 2)(*[s.size for s in streams])
    for bad_ec in (0, 9):
        ecs = (_ci * 2)(got[0][2], bad_ec)
        assert db(p._h, 2, ptrs, sizes, ecs, 20, h, w, _p(x_hat), _stream()) < 0
    ecs = (_ci * 2)(got[0][2], got[1][2])
    for n in (0, 17):
        assert db(p._h, n, ptrs, sizes, ecs, 20, h, w, _p(x_hat), _stream()) < 0
    assert db(p._h, 2, None, sizes, ecs, 20, h, w, _p(x_hat), _stream()) < 0
    assert db(p._h, 2, ptrs, None, ecs, 20, h, w, _p(x_hat), _stream()) < 0
    assert db(p._h, 2, ptrs, sizes, None, 20, h, w, _p(x_hat), _stream()) < 0
    assert db(p._h, 2, ptrs, sizes, ecs, 20, h, w, None, _stream()) < 0
    assert db(p._h, 2, ptrs, sizes, ecs, 20, h, w, _p(x_hat), _stream()) == 0
    torch.cuda.synchronize()
