"""conv_gemm.hip through the production dispatcher, tile shape by tile shape (-m gpu).

`launch()` picks one of five tile shapes (BM x BN: 256x256, 256x192, 64x64, 64x128, 128x128) from (M, N, K); each tile shape
and epilogue (bias, WSiLU, WSiLU + chunk-add, chunk-add alone, r1, r1 + r2, q, r1 + q; the k x k convs and the transposed
conv, single and batched) is its own kernel with its own LDS layout, output swizzle and WSiLU table copies. CASES lands
`launch()` itself on every reachable pair - the launch records of dcvc_gemm_profile_* confirm which tile ran - and checks:

* every output element against the float64 reference and its error bound (tests/f64_ref.py, fixed on the CPU by
  test_f64_ref_cpu.py), plus the rounding-bias statistic;
* a row subset bit-exact against the oracle: the first rows, both sides of the ragged last tile and of every picture boundary,
  the last rows;
* batched k x k / transposed convs bit-exact against one launch per picture;
* sentinels in the channels around the output slice and in the rows behind it stay untouched;
* three input distributions (f64_ref.DISTS): N(0, 1), a wide exponent range with zero rows and subnormals, outputs near 3e4.

test_wsilu_edges_gpu puts chosen accumulator values (segment boundaries, the rounded-sum sliver below them, the clamp points,
+-8, +-1000, +-65504) through the WSiLU and chunk-add epilogues of every tile that has one: zero activations but one column,
so each accumulator is its bias moved by 0, 1 or 2 float32 ulps."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

T256, T192, T64, T64x128, T128 = (256, 256), (256, 192), (64, 64), (64, 128), (128, 128)
TILES = (T256, T192, T64, T64x128, T128)
FAMILIES = ("bias", "wsilu", "wsilu_chunk", "chunk", "r1", "r1r2", "q", "r1q", "spatial", "spatial_b", "upsample", "upsample_b")
REACHABLE = {(t, f) for t in TILES for f in FAMILIES if not (f in ("wsilu_chunk", "chunk") and t in (T192, T64))}
SENT = 0x7E5A                       # a NaN payload no kernel produces
OFF = 8                             # every operand is a channel slice starting 8 channels (16 bytes) into its rows


def C(tile, fam, M=0, N=0, K=0, **kw):
    return dict(tile=tile, fam=fam, M=M, N=N, K=K, **kw)


def S(tile, fam, k, s, p, n, H, W, cin, cout):
    return dict(tile=tile, fam=fam, k=k, s=s, p=p, n=n, H=H, W=W, K=cin, N=cout)


def U(tile, fam, n, H, W, cin, cout):
    return dict(tile=tile, fam=fam, n=n, H=H, W=W, K=cin, N=cout)


CASES = [
    # 256 x 256: N % 256 == 0 and ceil(M / 256) * N / 256 >= 224
    C(T256, "bias", 14337, 1024, 64),                  # M one past a tile
    C(T256, "bias", 14400, 1024, 192, q2=True),
    C(T256, "wsilu", 14400, 1024, 64),
    C(T256, "wsilu_chunk", 14400, 1024, 192),
    C(T256, "chunk", 14401, 1024, 64),
    C(T256, "r1", 14400, 1024, 64),
    C(T256, "r1r2", 14400, 1024, 64, q2=True),
    C(T256, "q", 14400, 1024, 64),
    C(T256, "r1q", 14400, 1024, 192),
    S(T256, "spatial", 3, 1, 1, 1, 60, 240, 64, 1024),
    S(T256, "spatial_b", 3, 2, 1, 4, 120, 240, 64, 512),     # enc_down-like: picture boundaries inside the 256-pixel tiles
    U(T256, "upsample", 1, 100, 142, 64, 256),
    U(T256, "upsample_b", 2, 60, 120, 64, 256),
    # 256 x 192: N % 192 == 0 (not 256) and ceil(M / 256) * N / 192 >= 224
    C(T192, "bias", 19300, 576, 64),
    C(T192, "wsilu", 19300, 576, 64, q2=True),
    C(T192, "r1", 19300, 576, 64),
    C(T192, "r1r2", 19300, 576, 192),
    C(T192, "q", 19300, 576, 64, q2=True),
    C(T192, "r1q", 19300, 576, 64),
    S(T192, "spatial", 2, 2, 0, 1, 140, 560, 64, 576),
    S(T192, "spatial_b", 3, 2, 1, 2, 140, 280, 64, 576),
    U(T192, "upsample", 1, 60, 120, 64, 384),
    U(T192, "upsample_b", 3, 40, 60, 64, 384),
    # 64 x 64: K >= 512 and ceil(M / 64) * ceil(N / 128) <= 160
    C(T64, "bias", 1, 128, 512),                       # M = 1
    C(T64, "bias", 1000, 128, 512, q2=True),
    C(T64, "wsilu", 33, 192, 512),
    C(T64, "r1", 1000, 128, 512),
    C(T64, "r1r2", 65, 128, 512),
    C(T64, "q", 1000, 64, 512),
    C(T64, "r1q", 31, 128, 512, q2=True),
    S(T64, "spatial", 3, 2, 1, 1, 30, 40, 64, 128),
    S(T64, "spatial_b", 2, 2, 0, 3, 18, 22, 128, 128),
    U(T64, "upsample", 1, 17, 30, 512, 128),
    U(T64, "upsample_b", 2, 10, 20, 512, 128),
    # 64 x 128: the rest of the small grids (tiles of 128 x 128 < 640)
    C(T64x128, "bias", 33, 64, 64),                    # N = 64: the second wave of the tile idles
    C(T64x128, "bias", 31, 192, 192, q2=True),         # N = 192
    C(T64x128, "bias", 1, 320, 64),                    # N = 320, M = 1
    C(T64x128, "wsilu", 257, 256, 128),
    C(T64x128, "wsilu_chunk", 1000, 256, 128),
    C(T64x128, "chunk", 65, 512, 64),
    C(T64x128, "r1", 1000, 256, 128),
    C(T64x128, "r1r2", 1000, 192, 64, q2=True),
    C(T64x128, "q", 129, 256, 128),
    C(T64x128, "r1q", 1000, 256, 192),
    S(T64x128, "spatial", 3, 1, 1, 1, 50, 120, 64, 256),
    S(T64x128, "spatial_b", 2, 2, 0, 2, 18, 30, 64, 128),
    U(T64x128, "upsample", 1, 17, 30, 64, 128),
    U(T64x128, "upsample_b", 3, 5, 7, 64, 128),
    # 128 x 128: tiles of 128 x 128 >= 640 and neither 256-pixel tile nor 64 x 64
    C(T128, "bias", 20609, 512, 64),                   # M one past a tile
    C(T128, "bias", 81921, 64, 64),                    # N = 64: the second wave idles
    C(T128, "bias", 41000, 192, 192, q2=True),         # N = 192
    C(T128, "bias", 27300, 320, 64),                   # N = 320
    C(T128, "wsilu", 20600, 512, 64),
    C(T128, "wsilu_chunk", 20600, 512, 192),
    C(T128, "chunk", 20600, 512, 64),
    C(T128, "r1", 20600, 512, 64, q2=True),
    C(T128, "r1r2", 20600, 512, 64),
    C(T128, "q", 20600, 512, 192),
    C(T128, "r1q", 20600, 512, 64, q2=True),
    S(T128, "spatial", 2, 2, 0, 1, 140, 600, 64, 512),
    S(T128, "spatial_b", 3, 2, 1, 3, 120, 240, 64, 512),
    U(T128, "upsample", 1, 100, 204, 64, 128),
    U(T128, "upsample_b", 2, 80, 128, 64, 128),
]


def _geom(c):
    """(M, N, K, up_cout) of the contraction a case launches"""
    if c["fam"].startswith("spatial"):
        Ho = (c["H"] + 2 * c["p"] - c["k"]) // c["s"] + 1
        Wo = (c["W"] + 2 * c["p"] - c["k"]) // c["s"] + 1
        return c["n"] * Ho * Wo, c["N"], c["k"] * c["k"] * c["K"], 0
    if c["fam"].startswith("upsample"):
        return c["n"] * c["H"] * c["W"], 4 * c["N"], c["K"], c["N"]
    return c["M"], c["N"], c["K"], 0


def predict_tile(M, N, K, chunk=False, up_cout=0):
    """conv_gemm.hip launch(), restated"""
    nq = up_cout if up_cout else N
    mt256 = (M + 255) // 256
    if nq % 256 == 0 and mt256 * (N // 256) >= 224:
        return T256
    if not chunk and nq % 192 == 0 and mt256 * (N // 192) >= 224:
        return T192
    if not chunk and ((M + 63) // 64) * ((N + 127) // 128) <= 160 and K >= 512 and (not up_cout or up_cout % 64 == 0):
        return T64
    return T64x128 if ((M + 127) // 128) * ((N + 127) // 128) < 640 else T128


def _name(c):
    M, N, K, _ = _geom(c)
    extra = ("_n%d_k%ds%d" % (c["n"], c["k"], c["s"])) if "k" in c else ("_n%d" % c["n"]) if "n" in c else ""
    return "%dx%d-%s-M%d-N%d-K%d%s%s" % (c["tile"] + (c["fam"], M, N, K, extra, "-q2" if c.get("q2") else ""))


def test_cases_cover_every_reachable_tile_and_family():
    """the table lands on every reachable (tile, family) pair (per the dispatcher restated here; the GPU tests assert the
    tile that actually ran), q2 runs on every tile, and the edge shapes are in it"""
    got = set()
    for c in CASES:
        M, N, K, up = _geom(c)
        assert predict_tile(M, N, K, "chunk" in c["fam"], up) == c["tile"], _name(c)
        got.add((c["tile"], c["fam"]))
    missing = sorted(REACHABLE - got)
    print("covered %d (tile, family) pairs of %d reachable; missing: %s" % (len(got & REACHABLE), len(REACHABLE), missing or "none"))
    assert not missing and got <= REACHABLE
    assert {c["tile"] for c in CASES if c.get("q2")} == set(TILES)
    g = [_geom(c) for c in CASES]
    assert {64, 192} <= {K for _, _, K, _ in g}
    for t in (T64x128, T128):
        assert {64, 192, 320} <= {_geom(c)[1] for c in CASES if c["tile"] == t and not c["fam"].startswith(("up", "sp"))}
    assert {1, 31, 33} <= {M for M, _, _, _ in g}
    assert any(M % c["tile"][0] == 1 and M > c["tile"][0] for c, (M, _, _, _) in zip(CASES, g))
    assert (T256, "spatial_b") in got and (T128, "chunk") in got and (T64x128, "chunk") in got and (T256, "chunk") in got


# ---------------------------------------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "needs the MI355X"
    from gpu_util import Ops
    from dcvc_amd import _lib
    o = Ops()
    o.conv_kxk_b = _lib.fn("dcvc_conv_kxk_b", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                               ctypes.c_void_p] + [ctypes.c_int] * 9 + [ctypes.c_void_p])
    o.tconv2x2_b = _lib.fn("dcvc_tconv2x2_b", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
                           + [ctypes.c_int] * 6 + [ctypes.c_void_p])
    o.prof_en = _lib.fn("dcvc_gemm_profile_enable", ctypes.c_int, [ctypes.c_int])
    o.prof_reset = _lib.fn("dcvc_gemm_profile_reset", ctypes.c_int, [])
    o.prof_get = _lib.fn("dcvc_gemm_profile_launches", ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_longlong])
    return o


REC = np.dtype([("M", np.int32), ("N", np.int32), ("K", np.int32), ("variant", np.int32), ("ms", np.float32)])
RESULTS = {}


def _profiled(ops, fn):
    """runs fn() with the launch records on; returns [(M, N, K, BM, BN, epilogue bits)]"""
    from dcvc_amd import _lib
    _lib.check(ops.prof_reset())
    _lib.check(ops.prof_en(1))
    try:
        fn()
        torch.cuda.synchronize()
        buf = np.zeros(16, dtype=REC)
        n = int(ops.prof_get(buf.ctypes.data, len(buf)))
        assert 0 < n <= len(buf)
        v = buf["variant"][:n].astype(np.int64)
        assert ((v >> 28) & 0xF == 0).all(), "not a conv_gemm launch"
        return [(int(r["M"]), int(r["N"]), int(r["K"]), int((x >> 8) & 0x3FF), int((x >> 18) & 0x3FF), int(x & 0x7F))
                for r, x in zip(buf[:n], v)]
    finally:
        ops.prof_en(0)
        ops.prof_reset()


def _vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 2 * off)


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _slice(rows_shape, C, dev, fill=None):
    """buffer [..., C + 2 OFF] and its channel slice [..., OFF:OFF + C]"""
    buf = torch.empty(rows_shape + (C + 2 * OFF,), dtype=torch.half, device=dev)
    if fill is None:
        buf.view(torch.int16).fill_(SENT)
    return buf, buf[..., OFF:OFF + C]


def _put(src, dev):
    buf, view = _slice(tuple(src.shape[:-1]), src.shape[-1], dev)
    view.copy_(src.to(dev))
    return buf, view


def _untouched(buf, C, what):
    bits = buf.view(torch.int16)
    assert bool((bits[..., :OFF] == SENT).all()) and bool((bits[..., OFF + C:] == SENT).all()), what + ": wrote outside the channel slice"


def _rows(M, BM, bounds=()):
    s = set(range(min(M, 16))) | set(range(max(0, M - 16), M))
    for r in [BM, (M - 1) // BM * BM] + list(bounds):
        s |= set(range(max(0, r - 3), min(M, r + 3)))
    return sorted(s)


def _cols_rows(xh, rows, k, s, p, Ho, Wo):
    """numpy im2col for chosen output pixels of a batch xh [n, H, W, C], (ky, kx, cin) order as conv_gemm / nn.conv_kxk"""
    n, H, W, Cc = xh.shape
    out = np.zeros((len(rows), k * k * Cc), dtype=np.float16)
    for i, m in enumerate(rows):
        b, r = divmod(m, Ho * Wo)
        oy, ox = divmod(r, Wo)
        for ky in range(k):
            for kx in range(k):
                iy, ix = oy * s + ky - p, ox * s + kx - p
                if 0 <= iy < H and 0 <= ix < W:
                    out[i, (ky * k + kx) * Cc:(ky * k + kx + 1) * Cc] = xh[b, iy, ix]
    return out


def _record(c, dist, st, extra=""):
    RESULTS.setdefault((c["tile"], c["fam"]), []).append((_name(c) + extra, dist, st["max_ulp"], st["exact"]))


# ---------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("case", CASES, ids=[_name(c) for c in CASES])
def test_gemm_matrix(ops, case):
    from dcvc_amd.plugin import MLCodec_extensions_cpp  # noqa: F401  (loads the library)
    for i, dist in enumerate(R.DISTS):
        fam = case["fam"]
        if fam.startswith("spatial"):
            _run_spatial(ops, case, dist, 1000 + i)
        elif fam.startswith("upsample"):
            _run_upsample(ops, case, dist, 2000 + i)
        else:
            _run_1x1(ops, case, dist, 3000 + i)


def _tile_ran(recs, c, what):
    M, N, K, _ = _geom(c)
    assert len(recs) == 1 and recs[0][:3] == (M, N, K), (what, recs)
    assert (recs[0][3], recs[0][4]) == c["tile"], "%s: ran on %dx%d, the case is for %dx%d" % ((what,) + recs[0][3:5] + c["tile"])
    return recs[0][5]


def _run_1x1(ops, c, dist, seed):
    from dcvc_amd import _lib
    from oracle import nn
    dev = "cuda"
    M, N, K, fam = c["M"], c["N"], c["K"], c["fam"]
    wsilu, chunk = fam.startswith("wsilu"), fam.endswith("chunk")
    nr = 2 if fam.startswith("r1r2") else 1 if fam.startswith("r1") else 0
    hasq = fam in ("q", "r1q")
    nout = N // 4 if chunk else N
    x, w, b = R.inputs(dist, (M, K), N, seed)
    g = torch.Generator().manual_seed(seed + 7)
    big = dist == "near_overflow"
    rs = 100.0 if big else 1.0
    r1 = (torch.randn((M, nout), generator=g) * rs).half() if nr >= 1 else None
    r2 = (torch.randn((M, nout), generator=g) * rs).half() if nr >= 2 else None
    q = (torch.randn((nout,), generator=g) * 0.25 + 1).clamp(0.5, 1.5).half() if hasq else None
    q2 = (torch.randn((nout,), generator=g) * 0.25 + 1).clamp(0.5, 1.5).half() if c.get("q2") else None
    xb, xv = _put(x, dev)
    w, b = w.to(dev), b.to(dev)
    if big:
        peak = R.conv1x1(xv, w, b).t.abs().amax(0)
        w, b = R.fit_overflow(w, b, peak, 6e3 if chunk else 2e4)
    r1b, r1v = _put(r1, dev) if r1 is not None else (None, None)
    r2b, r2v = _put(r2, dev) if r2 is not None else (None, None)
    q, q2 = (None if t is None else t.to(dev) for t in (q, q2))
    yb = torch.empty((M + 3, nout + 2 * OFF), dtype=torch.half, device=dev)
    yb.view(torch.int16).fill_(SENT)
    flags = (1 if wsilu else 0) | (2 if chunk else 0)
    what = "%s %s" % (_name(c), dist)

    def go():
        _lib.check(ops.conv1x1(_vp(xb, OFF), K + 2 * OFF, _vp(w), _vp(b), None if r1b is None else _vp(r1b, OFF), nout + 2 * OFF,
                               None if r2b is None else _vp(r2b, OFF), nout + 2 * OFF, None if q is None else _vp(q),
                               None if q2 is None else _vp(q2), _vp(yb, OFF), nout + 2 * OFF, M, K, N, flags, _strm()))
    bits = _tile_ran(_profiled(ops, go), c, what)
    assert bits == (2 if wsilu else 0) | (4 if chunk else 0) | (nr << 3) | (32 if hasq else 0), (what, bits)
    _untouched(yb[:M], nout, what)
    assert bool((yb[M:].view(torch.int16) == SENT).all()), what + ": wrote rows past M"
    y = yb[:M, OFF:OFF + nout]
    ap = R.conv1x1(xv, w, b, r1=r1v, r2=r2v, q=q, q2=q2, wsilu=wsilu, chunk_add=chunk)
    st = R.check(y, ap, what)
    rows = _rows(M, c["tile"][0])
    npx = lambda t: None if t is None else t[rows].cpu().numpy()
    orc = nn.conv1x1(npx(xv), w.cpu().numpy(), b.cpu().numpy(), r1=npx(r1v), r2=npx(r2v),
                     q=None if q is None else q.cpu().numpy(), q2=None if q2 is None else q2.cpu().numpy(), wsilu=wsilu,
                     chunk_add=chunk)
    got = y[rows].cpu().numpy()
    assert np.array_equal(got.view(np.int16), orc.view(np.int16)), "%s: %d of %d oracle rows' elements differ" % (
        what, int((got.view(np.int16) != orc.view(np.int16)).sum()), got.size)
    _record(c, dist, st)


def _run_spatial(ops, c, dist, seed):
    from dcvc_amd import _lib
    from oracle import nn
    dev = "cuda"
    k, s, p, n, H, W, cin, cout = (c[f] for f in ("k", "s", "p", "n", "H", "W", "K", "N"))
    M, N, K, _ = _geom(c)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x, w1, b = R.inputs(dist, (n, H, W, cin), cout * k * k, seed)
    w = w1.view(cout, k * k, cin)[:, :, :].reshape(cout, k, k, cin).permute(0, 3, 1, 2).contiguous()   # [cout][cin][k][k]
    b = b[:cout]
    xb, xv = _put(x, dev)
    w, b = w.to(dev), b.to(dev)
    if dist == "near_overflow":
        peak = R.conv_kxk(xv, w, b, k, s, p).t.abs().amax(0)
        w2, b = R.fit_overflow(w.reshape(cout, -1), b, peak)
        w = w2.reshape(cout, cin, k, k)
    wt = w.permute(0, 2, 3, 1).contiguous()           # [cout][ky][kx][cin]
    yb = torch.empty((M + 3, cout + 2 * OFF), dtype=torch.half, device=dev)
    yb.view(torch.int16).fill_(SENT)
    what = "%s %s" % (_name(c), dist)

    def go():
        _lib.check(ops.conv_kxk_b(_vp(xb, OFF), cin + 2 * OFF, _vp(wt), _vp(b), _vp(yb, OFF), cout + 2 * OFF, H, W, cin, cout, k, s,
                                  p, n, _strm()))
    bits = _tile_ran(_profiled(ops, go), c, what)
    assert bits == 1, (what, bits)
    _untouched(yb[:M], cout, what)
    assert bool((yb[M:].view(torch.int16) == SENT).all()), what + ": wrote rows past M"
    y = yb[:M, OFF:OFF + cout]
    st = R.check(y, R.conv_kxk(xv, w, b, k, s, p), what)
    rows = _rows(M, c["tile"][0], [i * Ho * Wo for i in range(1, n)])
    cols = _cols_rows(xv.cpu().numpy(), rows, k, s, p, Ho, Wo)
    orc = nn.conv1x1(cols, wt.reshape(cout, -1).cpu().numpy(), b.cpu().numpy())
    got = y[rows].cpu().numpy()
    assert np.array_equal(got.view(np.int16), orc.view(np.int16)), what + ": oracle rows differ"
    if n > 1:                                          # one launch per picture: the same bits
        for i in range(n):
            yi = torch.empty((Ho * Wo, cout), dtype=torch.half, device=dev)
            _lib.check(ops.conv_kxk(_vp(xb[i], OFF), cin + 2 * OFF, _vp(wt), _vp(b), _vp(yi), cout, H, W, cin, cout, k, s, p,
                                    _strm()))
            assert torch.equal(yi.view(torch.int16), y[i * Ho * Wo:(i + 1) * Ho * Wo].view(torch.int16)), what + " picture %d" % i
    _record(c, dist, st)


def _run_upsample(ops, c, dist, seed):
    from dcvc_amd import _lib
    from oracle import nn
    dev = "cuda"
    n, H, W, cin, cout = (c[f] for f in ("n", "H", "W", "K", "N"))
    M, N, K, _ = _geom(c)
    x, w2, _ = R.inputs(dist, (n, H, W, cin), 4 * cout, seed)
    xb, xv = _put(x, dev)
    w2 = w2.to(dev)
    if dist == "near_overflow":
        peak = R.conv1x1(xv.reshape(-1, cin), w2, None).t.abs().amax(0)
        w2, _ = R.fit_overflow(w2, torch.zeros(4 * cout, dtype=torch.half, device=dev), peak)
    wq = w2.view(4, cout, cin).contiguous()
    yb = torch.empty((n, 2 * H, 2 * W, cout + 2 * OFF), dtype=torch.half, device=dev)
    yb.view(torch.int16).fill_(SENT)
    what = "%s %s" % (_name(c), dist)

    def go():
        _lib.check(ops.tconv2x2_b(_vp(xb, OFF), cin + 2 * OFF, _vp(wq), _vp(yb, OFF), cout + 2 * OFF, H, W, cin, cout, n, _strm()))
    bits = _tile_ran(_profiled(ops, go), c, what)
    assert bits == 64, (what, bits)
    _untouched(yb, cout, what)
    y = yb[..., OFF:OFF + cout]
    st = R.check(y, R.tconv2x2(xv, wq), what)
    rows = _rows(M, c["tile"][0], [i * H * W for i in range(1, n)])
    xr = xv.reshape(-1, cin)[rows].cpu().numpy()
    for qd in range(4):
        orc = nn.conv1x1(xr, wq[qd].cpu().numpy())
        bi, rr = np.divmod(np.array(rows), H * W)
        yy, xx = np.divmod(rr, W)
        got = y[torch.from_numpy(bi), torch.from_numpy(2 * yy + (qd >> 1)), torch.from_numpy(2 * xx + (qd & 1))].cpu().numpy()
        assert np.array_equal(got.view(np.int16), orc.view(np.int16)), what + ": oracle rows differ (quad %d)" % qd
    if n > 1:
        for i in range(n):
            yi = torch.empty((2 * H, 2 * W, cout), dtype=torch.half, device=dev)
            _lib.check(ops.tconv2x2(_vp(xb[i], OFF), cin + 2 * OFF, _vp(wq), _vp(yi), cout, H, W, cin, cout, _strm()))
            assert torch.equal(yi.view(torch.int16), y[i].contiguous().view(torch.int16)), what + " picture %d" % i
    _record(c, dist, st)


def test_tconv2x2_rejects_cout_192(ops):
    """a 128-wide channel tile would straddle two output pixels at cout = 192 (include/dcvc_amd_ops.h)"""
    from dcvc_amd import _lib
    x = torch.zeros((4, 4, 64), dtype=torch.half, device="cuda")
    w = torch.zeros((4, 192, 64), dtype=torch.half, device="cuda")
    y = torch.full((8, 8, 192), 7.0, dtype=torch.half, device="cuda")
    rc = ops.tconv2x2(_vp(x), 64, _vp(w), _vp(y), 192, 4, 4, 64, 192, _strm())
    torch.cuda.synchronize()
    assert rc < 0 and "multiple of 128" in _lib.lib().dcvc_last_error().decode()
    assert bool((y == 7.0).all())


# ---------------------------------------------------------------------------------------------- WSiLU edges
def _edge_values():
    v = []
    for i in range(257):
        bd = -4.0 + i / 32.0
        v += [bd, float(np.nextafter(np.float16(bd), np.float16(-np.inf))), float(np.nextafter(np.float16(bd), np.float16(np.inf)))]
        if abs(bd) < 0.5:                      # the rounded-sum sliver: 2^-12 below a boundary (exact in fp16 here)
            v += [bd - 2.0 ** -12, bd - 2.0 ** -13, bd + 2.0 ** -12]
    v += [3.998046875, -3.998046875, 4.0, -4.0, 8.0, -8.0, 1000.0, -1000.0, 65504.0, -65504.0, 0.0]
    return np.unique(np.array(v, dtype=np.float16))


EDGE_TILES = [(T256, 14400, 1024, 64, False), (T192, 19300, 576, 64, False), (T64, 1000, 128, 512, False),
              (T64x128, 1000, 256, 64, False), (T128, 20600, 512, 64, False),
              (T256, 14400, 1024, 64, True), (T64x128, 1000, 256, 64, True), (T128, 20600, 512, 64, True)]


@pytest.mark.parametrize("tile,M,N,K,chunk", EDGE_TILES, ids=["%dx%d-%s" % (t[0] + ("wsilu_chunk" if t[4] else "wsilu",))
                                                              for t in EDGE_TILES])
def test_wsilu_edges_gpu(ops, tile, M, N, K, chunk):
    from dcvc_amd import _lib
    from oracle import nn
    dev = "cuda"
    vals = _edge_values()
    per = N
    nout = N // 4 if chunk else N
    # rows: the accumulator of channel n is bias[n] + pat[row] * u[n], u[n] = one float32 ulp of bias[n] (an fp16 weight)
    pat = torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0]).half()
    x = torch.zeros((M, K), dtype=torch.half)
    x[:, 0] = pat[torch.arange(M) % 5]
    xd = x.to(dev)
    rows = list(range(10)) + list(range(M - 10, M))
    worst = 0.0
    for c0 in range(0, len(vals), per):
        chunk_vals = np.zeros(N, dtype=np.float16)
        part = vals[c0:c0 + per]
        chunk_vals[:len(part)] = part
        if chunk:                               # mix the groups of four: every value next to others of other segments
            chunk_vals = chunk_vals.reshape(4, N // 4).T.reshape(-1).copy()
        b = torch.from_numpy(chunk_vals)
        bf = b.float().abs()
        ulp = torch.where(bf > 0, torch.pow(2.0, torch.floor(torch.log2(torch.where(bf > 0, bf, torch.ones_like(bf)))) - 23),
                          torch.zeros_like(bf))
        w = torch.zeros((N, K), dtype=torch.half)
        w[:, 0] = ulp.clamp(min=2.0 ** -24).half()
        wd, bd = w.to(dev), b.to(dev)
        yb = torch.empty((M, nout + 2 * OFF), dtype=torch.half, device=dev)
        yb.view(torch.int16).fill_(SENT)

        def go():
            _lib.check(ops.conv1x1(_vp(xd), K, _vp(wd), _vp(bd), None, nout, None, nout, None, None, _vp(yb, OFF), nout + 2 * OFF,
                                   M, K, N, 1 | (2 if chunk else 0), _strm()))
        recs = _profiled(ops, go)
        assert (recs[0][3], recs[0][4]) == tile, recs
        _untouched(yb, nout, "wsilu edges")
        y = yb[:, OFF:OFF + nout]
        # every row of a pattern holds the same numbers: check five rows against fp64 and oracle, the rest for equality
        y5 = y[:5]
        assert torch.equal(y.view(torch.int16).reshape(-1)[:(M // 5) * 5 * nout].view(M // 5, 5, nout),
                           y5.view(torch.int16).expand(M // 5, 5, nout)), "rows of one pattern differ"
        ap = R.conv1x1(xd[:5], wd, bd, wsilu=True, chunk_add=chunk)
        st = R.stats(y5, ap)          # (no rounding-bias statistic: these inputs are chosen, not random)
        assert st["bad"] == 0, "wsilu edges %dx%d: %r" % (tile + (st,))
        worst = max(worst, st["max_ulp"])
        orc = nn.conv1x1(x[rows].numpy(), w.numpy(), b.numpy(), wsilu=True, chunk_add=chunk)
        assert np.array_equal(y[rows].cpu().numpy().view(np.int16), orc.view(np.int16)), "wsilu edges: oracle differs"
    RESULTS.setdefault((tile, "wsilu_chunk" if chunk else "wsilu"), []).append(("edges", "edge values", worst, float("nan")))


def test_zz_coverage_report():
    """(tile, family) -> cases and their worst error in fp16 ulps, as measured above; every reachable pair ran"""
    if not RESULTS:
        print("no matrix case ran in this process: nothing to report")
        return
    lines = []
    for key in sorted(RESULTS):
        for name, dist, ulp, exact in RESULTS[key]:
            lines.append("%7s %-12s %-52s %-14s max %5.1f ulp  exact %.4f" % ("%dx%d" % key[0], key[1], name, dist, ulp, exact))
    print("\n" + "\n".join(lines))
    missing = sorted(REACHABLE - set(RESULTS))
    print("missing (tile, family) pairs: %s" % (missing or "none"))
    assert not missing
