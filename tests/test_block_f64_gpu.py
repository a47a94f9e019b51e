"""The fused DepthConvBlock kernels against the chained float64 reference (-m gpu).

dcb_nsplit8 (every block shape, both workgroup sizes, every NEXT slot, the depthwise conv inside), dcb_pair8, dcb_tail (single
and batched) and ffn_fused through their C entry points, case tables in tests/block_cases.py (test_block_f64_cpu.py shows they
reach every compiled instantiation). Every case runs the three input distributions of f64_ref.DISTS and checks:

* every stored output against f64_ref.dcb / pair / ffn - each element inside its interval, no rounding bias, and a share of
  elements equal to reference16 of the chained midpoints of at least block_cases.EXACT_FLOOR (derived on the CPU from the
  oracle chain, test_block_f64_cpu.py): behind every ambiguous fp16 intermediate the interval widens, the share does not;
* up to 16 rows bit-exact against the oracle chain (oracle.nn: conv1x1 / dwconv3x3 in the launch order): the first and last
  rows, both sides of the ragged last tile, the rows either side of a tile that spans picture rows;
* the launch record names the instantiation the case is for (ops.h variant bits);
* NaN-payload sentinels in the channels either side of every output slice and in three rows past the last pixel;
* batched dcb_tail per picture, and a reference whose halo reads the neighbouring picture is rejected."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_cases as B  # noqa: E402
import f64_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7E5A                       # a NaN payload no kernel produces
OFF = 8                             # operands and outputs are channel slices 8 channels (16 bytes) into their rows
RESULTS = {}                        # instantiation key -> [(case, dist, output, max ulp, exact share)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "needs the MI355X"
    from gpu_util import Ops
    from dcvc_amd import _lib
    from dcvc_amd.plugin import MLCodec_extensions_cpp  # noqa: F401  (loads the library)
    o = Ops()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    o.dcb_tail_b = _lib.fn("dcvc_dcb_tail_b", ci, [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci,
                                                   ci, ci, ci, ci, ci, ci, ci, vp])
    o.dwconv3x3_b = _lib.fn("dcvc_dwconv3x3_b", ci, [vp, ci, vp, vp, ci, ci, ci, ci, ci, vp])
    o.prof_en = _lib.fn("dcvc_gemm_profile_enable", ci, [ci])
    o.prof_reset = _lib.fn("dcvc_gemm_profile_reset", ci, [])
    o.prof_get = _lib.fn("dcvc_gemm_profile_launches", ctypes.c_longlong, [vp, ctypes.c_longlong])
    return o


REC = np.dtype([("M", np.int32), ("N", np.int32), ("K", np.int32), ("variant", np.int32), ("ms", np.float32)])


def _profiled(ops, fn):
    """runs fn() with the launch records on; returns the variant words of its launches"""
    from dcvc_amd import _lib
    _lib.check(ops.prof_reset())
    _lib.check(ops.prof_en(1))
    try:
        fn()
        torch.cuda.synchronize()
        buf = np.zeros(16, dtype=REC)
        n = int(ops.prof_get(buf.ctypes.data, len(buf)))
        return [int(v) & 0xFFFFFFFF for v in buf["variant"][:n]]
    finally:
        ops.prof_en(0)
        ops.prof_reset()


def _vp(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 2 * off)


def _strm():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(P, C):
    """sentinel-filled buffer [P + 3, C + 2 OFF]; the output is its slice [:P, OFF:OFF + C]"""
    buf = torch.empty((P + 3, C + 2 * OFF), dtype=torch.half, device="cuda")
    buf.view(torch.int16).fill_(SENT)
    return buf


def _put(src):
    buf = _out(src.shape[0], src.shape[1])
    buf[:src.shape[0], OFF:OFF + src.shape[1]].copy_(src)
    return buf


def _view(buf, P, C):
    return buf[:P, OFF:OFF + C]


def _untouched(buf, P, C, what):
    bits = buf.view(torch.int16)
    assert bool((bits[:P, :OFF] == SENT).all()) and bool((bits[:P, OFF + C:] == SENT).all()), what + ": wrote outside the channel slice"
    assert bool((bits[P:] == SENT).all()), what + ": wrote rows past the last pixel"


def _check(got, ap, key, what, out, dist):
    st = R.check(got, ap, what, sharp_bias=True)
    floor = B.EXACT_FLOOR[dist]
    assert st["exact"] >= floor, "%s: %.4f of the elements equal the chained reference (floor %.4f, worst %.1f ulp)" % (
        what, st["exact"], floor, st["max_ulp"])
    RESULTS.setdefault(key, []).append((what, out, st["max_ulp"], st["exact"]))


def _ran(recs, key, what):
    want = B.variant_bits(key)
    assert len(recs) == 1 and recs[0] == want, "%s: launch records %s, the case is for %s (0x%08x)" % (
        what, ["0x%08x" % v for v in recs], B.key_name(key), want)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _oracle_rows(M, PX, W=None, extra=()):
    s = {0, 1, M - 2, M - 1}
    last = (M - 1) // PX * PX
    s |= {last - 1, last, PX - 1, PX}
    if W is not None and W > 1:
        s |= {W - 1, W, PX - W, PX + W - 1}           # a tile that spans picture rows, and the row boundary inside it
    s |= set(extra)
    return sorted(r for r in s if 0 <= r < M)[:16]


def _orc_dw(t1_rows_fn, taps, n, H, W, rows):
    """oracle depthwise output of chosen pixels: the oracle runs on the (at most) three picture rows around each one"""
    from oracle import nn
    CI = taps.shape[1]
    wpt = np.ascontiguousarray(taps.reshape(3, 3, CI).transpose(2, 0, 1)[:, None])
    out = np.zeros((len(rows), CI), dtype=np.float16)
    for i, m in enumerate(rows):
        b, r = divmod(m, H * W)
        h, w = divmod(r, W)
        h0, h1 = max(0, h - 1), min(H, h + 2)
        win = t1_rows_fn(b * H * W + h0 * W, b * H * W + h1 * W).reshape(h1 - h0, W, CI)
        out[i] = nn.dwconv3x3(win, wpt)[h - h0, w]
    return out


def _orc_block(op, rows, t2r):
    from oracle import nn
    xr = _np(op["x"])[rows]
    y1 = nn.conv1x1(t2r, _np(op["w3"]), _np(op["b3"]), r1=xr)
    t = nn.conv1x1(y1, _np(op["w0"]), _np(op["b0"]), wsilu=True, chunk_add=True)
    y = nn.conv1x1(t, _np(op["w2"]), _np(op["b2"]), r1=y1, r2=xr if op["sc"] else None, q=_np(op["q"]), q2=_np(op["q2"]))
    nx = None
    if op.get("w1n") is not None:
        nx = nn.conv1x1(y, _np(op["w1n"]), _np(op["b1n"]), wsilu=True)
    elif op.get("wfin") is not None:
        nx = nn.conv1x1(y, _np(op["wfin"]), _np(op["bfin"]), q=_np(op.get("qfin")))
    return y, nx


def _same(got, want, what):
    g = got.cpu().numpy().view(np.int16)
    w = np.ascontiguousarray(want).view(np.int16)
    assert np.array_equal(g, w), "%s: %d of %d oracle rows' elements differ" % (what, int((g != w).sum()), g.size)


# ---------------------------------------------------------------------------------------------- dcb_nsplit8
@pytest.mark.parametrize("case", B.NSPLIT_CASES, ids=[B.name(c) for c in B.NSPLIT_CASES])
def test_dcb_nsplit8_f64(ops, case):
    for i, dist in enumerate(R.DISTS):
        _run_nsplit(ops, case, dist, 100 + i)


def _run_nsplit(ops, c, dist, seed):
    from dcvc_amd import _lib
    C, CI, H, W, nx = c["C"], c["CI"], c["H"], c["W"], c["next"]
    P = H * W
    key = B.predict(c)
    what = "%s %s [%s]" % (B.name(c), dist, B.key_name(key))
    op = B.block_operands(dist, seed, P, C, CI, entry="t1" if c["dw"] else "t2", geom=(1, H, W), nxt=nx, sc=c["sc"],
                          q=c["q"], q2=c["q2"], qf=nx > 1 and c["q"], dev="cuda")
    ent = op["t1"] if c["dw"] else op["t2"]
    eb = _put(ent)
    xb = _put(op["x"])
    x_orig = op["x"]
    yb = xb if c["inplace"] else _out(P, C)
    NW = CI if nx == 1 else nx
    nb = _out(P, NW) if nx else None
    ld = lambda n: n + 2 * OFF       # noqa: E731
    g = lambda k: op.get(k)          # noqa: E731

    def go():
        if c["dw"]:
            _lib.check(ops.dcb_nsplit_dw(_vp(eb, OFF), ld(CI), _vp(op["taps"]), W, _vp(xb, OFF), ld(C), _vp(g("w3")), _vp(g("b3")),
                                         _vp(g("w0")), _vp(g("b0")), _vp(g("w2")), _vp(g("b2")), _vp(g("q")), _vp(g("q2")),
                                         _vp(g("w1n")), _vp(g("b1n")), _vp(nb, OFF) if nx == 1 else None, ld(CI),
                                         _vp(g("wfin")), _vp(g("bfin")), _vp(g("qfin")), _vp(nb, OFF) if nx > 1 else None,
                                         ld(NW), nx if nx > 1 else 0, _vp(yb, OFF), ld(C), P, C, CI, int(c["sc"]), _strm()))
        elif nx > 1:
            _lib.check(ops.dcb_nsplit_fin(_vp(eb, OFF), ld(CI), _vp(xb, OFF), ld(C), _vp(g("w3")), _vp(g("b3")), _vp(g("w0")),
                                          _vp(g("b0")), _vp(g("w2")), _vp(g("b2")), _vp(g("q")), _vp(g("q2")), _vp(g("wfin")),
                                          _vp(g("bfin")), _vp(g("qfin")), _vp(nb, OFF), ld(NW), nx, _vp(yb, OFF), ld(C), P, C,
                                          CI, int(c["sc"]), _strm()))
        else:
            _lib.check(ops.dcb_nsplit(_vp(eb, OFF), ld(CI), _vp(xb, OFF), ld(C), _vp(g("w3")), _vp(g("b3")), _vp(g("w0")),
                                      _vp(g("b0")), _vp(g("w2")), _vp(g("b2")), _vp(g("q")), _vp(g("q2")), _vp(g("w1n")),
                                      _vp(g("b1n")), _vp(nb, OFF) if nx else None, ld(CI), _vp(yb, OFF), ld(C), P, C, CI,
                                      int(c["sc"]), _strm()))
    _ran(_profiled(ops, go), key, what)
    _untouched(yb, P, C, what + " y")
    if nb is not None:
        _untouched(nb, P, NW, what + " NEXT slot")
    op["x"] = x_orig
    ref = B.block_ref(R, op)
    y = _view(yb, P, C)
    _check(y, ref["y"], key, what + " y", "y", dist)
    if nx:
        _check(_view(nb, P, NW), ref["next"], key, what + " NEXT slot", "next", dist)
    # oracle rows
    PX = 64 if key[3] == 2 else 32
    rows = _oracle_rows(P, PX, W if c["dw"] else None)
    if c["dw"]:
        en = _np(ent)
        t2r = _orc_dw(lambda a, b: en[a:b], _np(op["taps"]), 1, H, W, rows)
    else:
        t2r = _np(ent)[rows]
    oy, onx = _orc_block(op, rows, t2r)
    _same(y[rows], oy, what + " y")
    if nx:
        _same(_view(nb, P, NW)[rows], onx, what + " NEXT slot")


# ---------------------------------------------------------------------------------------------- dcb_pair8
@pytest.mark.parametrize("case", B.PAIR_CASES, ids=[B.name(c) for c in B.PAIR_CASES])
def test_dcb_pair8_f64(ops, case):
    from dcvc_amd import _lib
    from oracle import nn
    CIN, C, CI, P = case["CIN"], case["C"], case["CI"], case["P"]
    key = B.predict(case)
    for i, dist in enumerate(R.DISTS):
        what = "%s %s [%s]" % (B.name(case), dist, B.key_name(key))
        op = B.pair_operands(dist, 200 + i, P, CIN, C, CI, dev="cuda")
        xb = _put(op["x"])
        yb, tb = _out(P, C), _out(P, CI)

        def go():
            _lib.check(ops.dcb_pair(_vp(xb, OFF), CIN + 2 * OFF, _vp(op["wa"]), _vp(op["ba"]), _vp(op["w1"]), _vp(op["b1"]),
                                    _vp(yb, OFF), C + 2 * OFF, _vp(tb, OFF), CI + 2 * OFF, P, CIN, C, CI, _strm()))
        _ran(_profiled(ops, go), key, what)
        _untouched(yb, P, C, what + " y")
        _untouched(tb, P, CI, what + " t1")
        ref = R.pair(op["x"], op["wa"], op["ba"], op["w1"], op["b1"])
        y, t1 = _view(yb, P, C), _view(tb, P, CI)
        _check(y, ref["y"], key, what + " y", "y", dist)
        _check(t1, ref["t1"], key, what + " t1", "t1", dist)
        rows = _oracle_rows(P, 64 if key[4] == 2 else 32)
        oy = nn.conv1x1(_np(op["x"])[rows], _np(op["wa"]), _np(op["ba"]))
        _same(y[rows], oy, what + " y")
        _same(t1[rows], nn.conv1x1(oy, _np(op["w1"]), _np(op["b1"]), wsilu=True), what + " t1")


# ---------------------------------------------------------------------------------------------- dcb_tail
@pytest.mark.parametrize("case", B.TAIL_CASES, ids=[B.name(c) for c in B.TAIL_CASES])
def test_dcb_tail_f64(ops, case):
    for i, dist in enumerate(R.DISTS):
        _run_tail(ops, case, dist, 300 + i)


def _run_tail(ops, c, dist, seed):
    from dcvc_amd import _lib
    from oracle import nn
    C, CD, CF, H, W, n = c["C"], c["CD"], c["CF"], c["H"], c["W"], c["n"]
    P = n * H * W
    key = B.predict(c)
    what = "%s %s [%s]" % (B.name(c), dist, B.key_name(key))
    entry = "x" if c["dc0"] else "t1" if c["dw"] else "t2"
    op = B.block_operands(dist, seed, P, C, CD, CF=CF, entry=entry, geom=(n, H, W), sc=c["sc"], q=c["q"], q2=c["q2"],
                          dev="cuda")
    xb = _put(op["x"])
    tb = _put(op[entry]) if entry != "x" else None
    inplace = not c["dc0"] and n == 1
    yb = xb.clone() if inplace else _out(P, C)
    xin = yb if inplace else xb
    ld = lambda k: k + 2 * OFF       # noqa: E731
    g = op.get
    args = lambda y_b, x_b, t_b, HH, NN: (                                                             # noqa: E731
        _vp(g("w1")), _vp(g("b1")), _vp(t_b, OFF) if t_b is not None else None, ld(CD), _vp(g("taps")), _vp(x_b, OFF), ld(C),
        _vp(g("w3")), _vp(g("b3")), _vp(g("w0")), _vp(g("b0")), _vp(g("w2")), _vp(g("b2")), _vp(g("q")), _vp(g("q2")),
        _vp(y_b, OFF), ld(C), HH, W, C, CD, CF, int(c["sc"]))

    def go():
        if n == 1:
            _lib.check(ops.dcb_tail(*args(yb, xin, tb, H, 1), _strm()))
        else:
            _lib.check(ops.dcb_tail_b(*args(yb, xin, tb, H, n), n, _strm()))
    _ran(_profiled(ops, go), key, what)
    _untouched(yb, P, C, what + " y")
    ref = B.block_ref(R, op)
    y = _view(yb, P, C)
    _check(y, ref["y"], key, what + " y", "y", dist)
    if n > 1:
        # one launch per picture: the same bits; a halo that reads the neighbouring picture is not what the kernel computes
        for b in range(n):
            sl = slice(b * H * W, (b + 1) * H * W)
            xi = _put(op["x"][sl])
            ti = _put(op[entry][sl]) if entry != "x" else None
            yi = _out(H * W, C)
            _lib.check(ops.dcb_tail(*args(yi, xi, ti, H, 1), _strm()))
            torch.cuda.synchronize()
            assert torch.equal(_view(yi, H * W, C).view(torch.int16), y[sl].view(torch.int16)), what + " picture %d" % b
        if c["dw"] or c["dc0"]:
            op2 = dict(op, geom=(1, n * H, W))
            assert not R.accepts(y, B.block_ref(R, op2)["y"]), what + ": a halo across pictures would pass the check"
    # oracle rows: the first and last pixels, the last patch's rows, and the rows either side of every picture boundary
    rows = _oracle_rows(P, 16, W, [b * H * W + d for b in range(1, n) for d in (-1, 0)])
    xn = _np(op["x"])
    if entry == "t2":
        t2r = _np(op["t2"])[rows]
    elif entry == "t1":
        en = _np(op["t1"])
        t2r = _orc_dw(lambda a, b: en[a:b], _np(op["taps"]), n, H, W, rows)
    else:
        w1, b1 = _np(op["w1"]), _np(op["b1"])
        t2r = _orc_dw(lambda a, b: nn.conv1x1(xn[a:b], w1, b1, wsilu=True), _np(op["taps"]), n, H, W, rows)
    oy, _ = _orc_block(op, rows, t2r)
    _same(y[rows], oy, what + " y")


# ---------------------------------------------------------------------------------------------- ffn_fused
@pytest.mark.parametrize("case", B.FFN_CASES, ids=[B.name(c) for c in B.FFN_CASES])
def test_ffn_fused_f64(ops, case):
    from dcvc_amd import _lib
    from oracle import nn
    C, CF, P = case["C"], case["CF"], case["P"]
    key = B.predict(case)
    for i, dist in enumerate(R.DISTS):
        what = "%s %s [%s]" % (B.name(case), dist, B.key_name(key))
        op = B.ffn_operands(dist, 400 + i, P, C, CF, case["r2"], case["q"], case["q2"], dev="cuda")
        xb = _put(op["x"])
        rb = _put(op["r2"]) if case["r2"] else None
        yb = xb.clone() if case["inplace"] else _out(P, C)
        xin = yb if case["inplace"] else xb

        def go():
            _lib.check(ops.ffn_fused(_vp(xin, OFF), C + 2 * OFF, _vp(op["w0"]), _vp(op["b0"]), _vp(op["w2"]), _vp(op["b2"]),
                                     _vp(rb, OFF), C + 2 * OFF, _vp(op["q"]), _vp(op["q2"]), _vp(yb, OFF), C + 2 * OFF, P, C, CF,
                                     _strm()))
        _ran(_profiled(ops, go), key, what)
        _untouched(yb, P, C, what + " y")
        ref = R.ffn(op["x"], op["w0"], op["b0"], op["w2"], op["b2"], r2=op["r2"], q=op["q"], q2=op["q2"])
        y = _view(yb, P, C)
        _check(y, ref["y"], key, what + " y", "y", dist)
        rows = _oracle_rows(P, 128)
        xr = _np(op["x"])[rows]
        t = nn.conv1x1(xr, _np(op["w0"]), _np(op["b0"]), wsilu=True, chunk_add=True)
        oy = nn.conv1x1(t, _np(op["w2"]), _np(op["b2"]), r1=xr, r2=None if rb is None else _np(op["r2"])[rows], q=_np(op["q"]),
                        q2=_np(op["q2"]))
        _same(y[rows], oy, what + " y")


# ---------------------------------------------------------------------------------------------- dwconv3x3
DW_GEOMS = [(1, 1, 40, 64), (1, 40, 1, 128), (1, 9, 7, 64), (1, 67, 121, 128), (2, 13, 37, 64), (3, 1, 33, 128)]


@pytest.mark.parametrize("n,H,W,C", DW_GEOMS, ids=["n%d-%dx%d-C%d" % g for g in DW_GEOMS])
def test_dwconv3x3_f64(ops, n, H, W, C):
    from dcvc_amd import _lib
    P = n * H * W
    for i, dist in enumerate(R.DISTS):
        x, _, _ = R.inputs(dist, (P, C), 1, 500 + i, "cuda")
        taps = (torch.randn((9, C), generator=torch.Generator().manual_seed(510 + i)) * 0.3).half().cuda()
        if dist == "near_overflow":
            x = (x.double() * 5e3).clamp(-6e4, 6e4).half()
        xb, yb = _put(x), _out(P, C)
        if n == 1:
            _lib.check(ops.dwconv3x3(_vp(xb, OFF), C + 2 * OFF, _vp(taps), _vp(yb, OFF), C + 2 * OFF, H, W, C, _strm()))
        else:
            _lib.check(ops.dwconv3x3_b(_vp(xb, OFF), C + 2 * OFF, _vp(taps), _vp(yb, OFF), C + 2 * OFF, H, W, C, n, _strm()))
        torch.cuda.synchronize()
        what = "dwconv3x3 n%d %dx%d C%d %s" % (n, H, W, C, dist)
        _untouched(yb, P, C, what)
        st = R.check(_view(yb, P, C), R.dwconv3x3(x, taps, n, H, W), what)
        assert st["exact"] >= B.EXACT_FLOOR[dist], (what, st)


# ---------------------------------------------------------------------------------------------- WSiLU edges
def _edge_values():
    v = []
    for i in range(257):
        bd = -4.0 + i / 32.0
        v += [bd, float(np.nextafter(np.float16(bd), np.float16(-np.inf))), float(np.nextafter(np.float16(bd), np.float16(np.inf)))]
        if abs(bd) < 0.5:                      # the rounded-sum sliver: 2^-12 below a boundary (exact in fp16 here)
            v += [bd - 2.0 ** -12, bd - 2.0 ** -13, bd + 2.0 ** -12]
    v += [3.998046875, -3.998046875, 4.0, -4.0, 8.0, -8.0, 1000.0, -1000.0, 0.0]
    return np.unique(np.array(v, dtype=np.float16))


def _edge_operands(N):
    """bias [N] of edge values and the weight column that moves each accumulator by 0, +-1, +-2 float32 ulps: with input
    column 0 = pattern[row % 5] (and every other input channel zero) the accumulator of channel j in row r is
    bias[j] + pattern[r % 5] * ulp32(bias[j])"""
    vals = _edge_values()
    chunks = []
    for c0 in range(0, len(vals), N):
        part = np.zeros(N, dtype=np.float16)
        p = vals[c0:c0 + N]
        part[:len(p)] = p
        b = torch.from_numpy(part)
        bf = b.float().abs()
        ulp = torch.where(bf > 0, torch.pow(2.0, torch.floor(torch.log2(torch.where(bf > 0, bf, torch.ones_like(bf)))) - 23),
                          torch.zeros_like(bf))
        chunks.append((b.cuda(), ulp.clamp(min=2.0 ** -24).half().cuda()))
    return chunks


PAT = torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0]).half()


def _pattern_x(P, C):
    x = torch.zeros((P, C), dtype=torch.half)
    x[:, 0] = PAT[torch.arange(P) % 5]
    return x.cuda()


def _onehot(nout, nin, skip_first=True):
    """[nout][nin]: output channel j + 1 takes input channel j (output 0 keeps the pattern column)"""
    w = torch.zeros((nout, nin), dtype=torch.half)
    for j in range(min(nin, nout - 1)):
        w[j + 1, j] = 1.0
    return w.cuda()


def _edge_check(got, ap, key, what):
    st = R.stats(got, ap)            # (no rounding-bias statistic: these inputs are chosen, not random)
    assert st["bad"] == 0, "%s: %r" % (what, st)
    RESULTS.setdefault(key, []).append((what, "edges", st["max_ulp"], st["exact"]))


EDGE_NSPLIT = [(256, 128), (384, 384)]          # Lay<>::RT = 4 and RT = 1 (test_block_f64_cpu.py restates Lay<>)


@pytest.mark.parametrize("C,CI", EDGE_NSPLIT, ids=["%d-%d" % s for s in EDGE_NSPLIT])
def test_wsilu_edges_dcb_nsplit8(ops, C, CI):
    """ffn.0's chunk epilogue (y1 = x: t2 = 0, w3 = b3 = 0; a one-hot ffn.2 puts t on the output) and the NEXT-slot dc.0
    epilogue (t = 0, ffn.2 = 0: y = x) of dcb_nsplit8, 32-pixel workgroups"""
    from dcvc_amd import _lib
    P = 40
    x = _pattern_x(P, C)
    z = lambda *s: torch.zeros(s, dtype=torch.half, device="cuda")     # noqa: E731
    t2 = z(P, CI)
    for stage, N in (("ffn.0", 4 * CI), ("dc.0", CI)):
        for b, u in _edge_operands(N):
            w = z(N, C)
            w[:, 0] = u
            if stage == "ffn.0":
                op = dict(x=x, w3=z(C, CI), b3=z(C), w0=w, b0=b, w2=_onehot(C, CI), b2=z(C), w1n=z(CI, C), b1n=z(CI))
            else:
                op = dict(x=x, w3=z(C, CI), b3=z(C), w0=z(4 * CI, C), b0=z(4 * CI), w2=z(C, CI), b2=z(C), w1n=w, b1n=b)
            yb, nb = _out(P, C), _out(P, CI)

            def go():
                _lib.check(ops.dcb_nsplit(_vp(t2), CI, _vp(x), C, _vp(op["w3"]), _vp(op["b3"]), _vp(op["w0"]), _vp(op["b0"]),
                                          _vp(op["w2"]), _vp(op["b2"]), None, None, _vp(op["w1n"]), _vp(op["b1n"]), _vp(nb, OFF),
                                          CI + 2 * OFF, _vp(yb, OFF), C + 2 * OFF, P, C, CI, 0, _strm()))
            key = ("nsplit8", C, CI, 1, 1, 0)
            _ran(_profiled(ops, go), key, "edges")
            ref = R.dcb(x, op["w3"], op["b3"], op["w0"], op["b0"], op["w2"], op["b2"], t2=t2, w1n=op["w1n"], b1n=op["b1n"])
            _edge_check(_view(yb, P, C), ref["y"], key, "edges %s %d-%d y" % (stage, C, CI))
            _edge_check(_view(nb, P, CI), ref["next"], key, "edges %s %d-%d dc.0" % (stage, C, CI))


def test_wsilu_edges_dcb_pair8(ops):
    from dcvc_amd import _lib
    CIN, C, CI, P = 512, 256, 128, 40
    x = _pattern_x(P, CIN)
    wa = torch.zeros((C, CIN), dtype=torch.half, device="cuda")
    wa[0, 0] = 1.0
    ba = torch.zeros(C, dtype=torch.half, device="cuda")
    key = ("pair8", CIN, C, CI, 1)
    for b, u in _edge_operands(CI):
        w1 = torch.zeros((CI, C), dtype=torch.half, device="cuda")
        w1[:, 0] = u
        yb, tb = _out(P, C), _out(P, CI)

        def go():
            _lib.check(ops.dcb_pair(_vp(x), CIN, _vp(wa), _vp(ba), _vp(w1), _vp(b), _vp(yb, OFF), C + 2 * OFF, _vp(tb, OFF),
                                    CI + 2 * OFF, P, CIN, C, CI, _strm()))
        _ran(_profiled(ops, go), key, "edges")
        _edge_check(_view(tb, P, CI), R.pair(x, wa, ba, w1, b)["t1"], key, "edges pair8 dc.0")


@pytest.mark.parametrize("C", [128, 256])
def test_wsilu_edges_dcb_tail(ops, C):
    """dc.0 inside (centre tap 1: t2 = t1; one-hot dc.3 puts it on y1, ffn.0 = 0 so y = y1) and ffn.0 (t = 0, dc.3 = 0:
    y1 = x; one-hot ffn.2)"""
    from dcvc_amd import _lib
    CD = CF = 128 if C == 256 else 64
    H, W = 8, 5
    P = H * W
    x = _pattern_x(P, C)
    z = lambda *s: torch.zeros(s, dtype=torch.half, device="cuda")     # noqa: E731
    taps = z(9, CD)
    taps[4] = 1.0
    for stage, N in (("dc.0", CD), ("ffn.0", 4 * CF)):
        for b, u in _edge_operands(N):
            w = z(N, C)
            w[:, 0] = u
            if stage == "dc.0":
                op = dict(x=x, w1=w, b1=b, taps=taps, geom=(1, H, W), w3=_onehot(C, CD), b3=z(C), w0=z(4 * CF, C),
                          b0=z(4 * CF), w2=z(C, CF), b2=z(C), sc=False, q=None, q2=None)
                key = ("tail", C, True, False, True)
            else:
                op = dict(x=x, t2=z(P, CD), w3=z(C, CD), b3=z(C), w0=w, b0=b, w2=_onehot(C, CF), b2=z(C), sc=False, q=None,
                          q2=None)
                key = ("tail", C, False, False, False)
            yb = _out(P, C)
            g = op.get

            def go():
                _lib.check(ops.dcb_tail(_vp(g("w1")), _vp(g("b1")), _vp(g("t2")), CD, _vp(g("taps")), _vp(x), C, _vp(g("w3")),
                                        _vp(g("b3")), _vp(g("w0")), _vp(g("b0")), _vp(g("w2")), _vp(g("b2")), None, None,
                                        _vp(yb, OFF), C + 2 * OFF, H, W, C, CD, CF, 0, _strm()))
            _ran(_profiled(ops, go), key, "edges")
            _edge_check(_view(yb, P, C), B.block_ref(R, op)["y"], key, "edges tail %d %s" % (C, stage))


@pytest.mark.parametrize("C", [128, 256, 384])
def test_wsilu_edges_ffn_fused(ops, C):
    from dcvc_amd import _lib
    CF, P = 64 if C == 128 else 128, 40
    x = _pattern_x(P, C)
    w2 = _onehot(C, CF)
    b2 = torch.zeros(C, dtype=torch.half, device="cuda")
    key = ("ffn", C, False, False)
    for b, u in _edge_operands(4 * CF):
        w0 = torch.zeros((4 * CF, C), dtype=torch.half, device="cuda")
        w0[:, 0] = u
        yb = _out(P, C)

        def go():
            _lib.check(ops.ffn_fused(_vp(x), C, _vp(w0), _vp(b), _vp(w2), _vp(b2), None, C, None, None, _vp(yb, OFF), C + 2 * OFF,
                                     P, C, CF, _strm()))
        _ran(_profiled(ops, go), key, "edges")
        _edge_check(_view(yb, P, C), R.ffn(x, w0, b, w2, b2)["y"], key, "edges ffn %d" % C)


def test_zz_coverage_report():
    """instantiation -> its worst error in fp16 ulps and its exact share, as measured above; every compiled instantiation ran"""
    if not RESULTS:
        print("no case ran in this process: nothing to report")
        return
    lines = []
    for key in sorted(RESULTS, key=B.key_name):
        rs = RESULTS[key]
        worst = max(r[2] for r in rs)
        ex = [r[3] for r in rs if r[1] != "edges"]
        lines.append("%-34s %3d checks  max %6.1f ulp  min exact %s" % (B.key_name(key), len(rs), worst,
                                                                         "%.4f" % min(ex) if ex else "  -   "))
    print("\n" + "\n".join(lines))
    missing = sorted(B.all_instantiations() - set(RESULTS), key=B.key_name)
    print("missing: %s" % (", ".join(B.key_name(k) for k in missing) or "none"))
    assert not missing
