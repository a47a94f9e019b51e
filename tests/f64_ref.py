"""float64 references of the conv_gemm operations (dcvc_amd/csrc/kernels/conv_gemm.hip) and the error model that says
how far the kernel may lie from them. TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).

Every reference returns an `Approx`: the float64 value `t` of the op BEFORE its fp16 rounding, a float64 bound `e` on how far
the kernel's fp32 value of the same quantity may lie from it, and the per-channel fp16 `q2` applied after that rounding.
The arithmetic policy (arith.h) rounds to fp16 once at the output and, with q2, once more after the fp16 product, so

    got in [ round16(t - e), round16(t + e) ]                       (round16 is monotone)
    got in [ round16(round16(t - e) * q2), round16(round16(t + e) * q2) ]          with q2 (bounds swapped for q2 < 0)

This is the element-wise bound |got - ref64| <= ulp16(ref64) + e stated exactly: a result one ulp off is accepted only where
t lies within e of the rounding boundary between the two fp16 values - a kernel off by one ulp elsewhere is caught.

The bound e, stage by stage:
  contraction  e = c_acc(K) * (|bias| + sum_k |x_k w_k|)
               c_acc(K) = 2^-24 (31 + K / 8): one v_mfma_f32_32x32x16_f16 step errs by at most 2^-24 (31 sum|ab| + 2 |c|)
               (tests/golden/mfma_probe.npz, 26 141 recorded MI355X results; test_f64_ref_cpu.py); over K / 16 steps the
               running accumulator |c| stays below |bias| + sum|ab|.
  WSiLU        e -> L_WSILU e + C_ACT    (L_WSILU = max |d/dv v sigmoid(4 v)|; C_ACT = max |wsilu_spec(v) - v sigmoid(4 v)|
               over every float32 v, product rounding included: test_f64_ref_cpu.py sweeps it)
  chunk-add    sum of the four bounds + 6 * 2^-24 * sum of the four magnitudes (one fp32 product and three fma / adds)
  + r1, + r2   e -> e + 2^-24 (|t| + e)          (one fp32 add each)
  * q          e -> |q| e + 2^-24 |q| (|t| + e)  (one fp32 multiply)
All references are plain torch float64 on whatever device the inputs are on (the GPU in the -m gpu tests).

Chains (the fused DepthConvBlock kernels: dcb_nsplit8, dcb_pair8, dcb_tail, ffn_fused): an fp16 intermediate the kernel
stores (in memory or in LDS) enters the next stage as `Mid`: mid = reference16(ap) and a radius rad = max(hi - mid, mid - lo)
over its interval - 0 wherever the kernel's rounding is forced, one fp16 ulp where t lies within e of a rounding boundary.
  contraction  t = mid @ w + b,  e = c_acc(K) ((|mid| + rad) @ |w| + |b|) + rad @ |w|
  residual     an fp16 intermediate adds its own rad to e before the 2^-24 add term
  depthwise    fp32 fmaf chain over at most 9 taps (orc_dwconv3x3's and dwconv.hip's order), zero padding:
               t = sum mid w,  e = 9 2^-24 sum (|mid| + rad) |w| + sum rad |w|
`dcb()`, `pair()` and `ffn()` return an Approx for every stored output of those launches."""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                 # unit roundoff of float32 (round to nearest)
MFMA_ALPHA = 31.0                # per 16-product step: error <= U32 * (MFMA_ALPHA * sum|ab| + MFMA_BETA * |c|)
MFMA_BETA = 2.0
C_ACT = 5.1e-7                   # WSiLU approximation, absolute: the figure arith.h claims (checked over the float32 line)
L_WSILU = 1.0999                 # max over v of |sigma(4v) + 4 v sigma(4v) (1 - sigma(4v))| = 1.09984...
FP16_MAX = 65504.0
BIAS_LIMIT = 0.1                 # |mean(sign(ref) (got - ref) / ulp16(ref))|: a truncating kernel scores about 0.5


def c_acc(K):
    """relative bound of the fp32 MFMA contraction over K (plus the float64 reference's own summation error)"""
    return U32 * (MFMA_ALPHA + MFMA_BETA * K / 16.0) + K * 2.0 ** -52


class Approx:
    __slots__ = ("t", "e", "q2")

    def __init__(self, t, e, q2=None):
        self.t, self.e, self.q2 = t, e, q2


def _d(a):
    return None if a is None else a.to(torch.float64)


# ---------------------------------------------------------------------------------------------- fp16 rounding in float64
def _binade(a):
    """exponent e with 2^e <= a < 2^(e+1) for a >= 0 (-1023 for zero and float64 subnormals, all far below fp16's range),
    read from the bit pattern: exact on every device"""
    return ((a.contiguous().view(torch.int64) >> 52) & 0x7FF) - 1023


def _pow2(k):
    """2^k as float64 for integer tensors k in the normal range, built from the bit pattern (torch.pow with a float64
    exponent is not exact on every device)"""
    return ((k + 1023) << 52).view(torch.float64)


def ulp16(v):
    """spacing of the fp16 grid at |v| (2^-24 floor for subnormals and zero)"""
    a = v.to(torch.float64).abs()
    return _pow2(torch.clamp(_binade(a), min=-14) - 10)


def round16(t):
    """float64 -> the fp16 grid, round to nearest even, subnormals kept, overflow to +-inf. Exact (one rounding): the
    scaling by the ulp is a power of two, torch.round is half-to-even. Returned as float64."""
    t = t.to(torch.float64)
    u = ulp16(t)
    r = torch.round(t / u) * u
    return torch.where(r.abs() > FP16_MAX, torch.sign(r) * math.inf, r)


def wsilu64(v):
    return v * torch.sigmoid(4.0 * v)


# ---------------------------------------------------------------------------------------------- references
def _contract(x, w, bias, rad=None):
    """x [P, K], w [N, K] (fp16 or float64, any device); returns (acc, bound). rad [P, K]: the radius of an fp16 intermediate x
    (see `Mid`)"""
    x64, w64 = _d(x), _d(w)
    K = x64.shape[-1]
    acc = x64 @ w64.t()
    wa = w64.abs().t()
    mag = (x64.abs() if rad is None else x64.abs() + rad) @ wa
    if bias is not None:
        b = _d(bias)
        acc = acc + b
        mag = mag + b.abs()
    e = c_acc(K) * mag
    return acc, e if rad is None else e + rad @ wa


def epilogue(acc, e, wsilu=False, chunk_add=False, r1=None, r2=None, q=None, q2=None, r1_rad=None, r2_rad=None):
    """the conv1x1 epilogue family on a float64 accumulator with bound e (order of arith.h / conv_gemm.hip); r1_rad / r2_rad:
    radii of residuals that are themselves fp16 intermediates"""
    if wsilu:
        v = wsilu64(acc)
        e = L_WSILU * e + C_ACT
        acc = v
    if chunk_add:
        P, N = acc.shape
        g = acc.view(P, N // 4, 4)
        eg = e.view(P, N // 4, 4)
        m = (g.abs() + eg).sum(-1)
        return Approx(g.sum(-1), eg.sum(-1) + 6 * U32 * m, None)
    for r, rr in ((r1, r1_rad), (r2, r2_rad)):
        if r is not None:
            acc = acc + _d(r)
            if rr is not None:
                e = e + rr
            e = e + U32 * (acc.abs() + e)
    if q is not None:
        qa = _d(q)
        acc = acc * qa
        e = qa.abs() * e + U32 * (acc.abs() + qa.abs() * e)
    return Approx(acc, e, None if q2 is None else _d(q2))


def conv1x1(x, w, bias=None, r1=None, r2=None, q=None, q2=None, wsilu=False, chunk_add=False):
    """x [P, K] (a view is fine), w [N, K]; r1 / r2 [P, Nout]; q / q2 [Nout]. x, r1 and r2 may be `Mid`s (chained
    intermediates)."""
    xm, xr = (x.mid, x.rad) if isinstance(x, Mid) else (x, None)
    r1m, r1r = (r1.mid, r1.rad) if isinstance(r1, Mid) else (r1, None)
    r2m, r2r = (r2.mid, r2.rad) if isinstance(r2, Mid) else (r2, None)
    acc, e = _contract(xm, w, bias, xr)
    return epilogue(acc, e, wsilu, chunk_add, r1m, r2m, q, q2, r1r, r2r)


def _cols(x64, k, s, p, rows=None):
    """im2col of ONE picture x64 [H, W, C] (float64) -> [Ho * Wo, C * k * k] (rows = an optional slice of output pixels)"""
    cols = F.unfold(x64.permute(2, 0, 1).unsqueeze(0), k, padding=p, stride=s)[0].t()
    return cols if rows is None else cols[rows]


def conv_kxk(x, w, bias, k, s, p, band=16384):
    """x [n, H, W, Cin] fp16, w PyTorch layout [Cout, Cin, k, k]; returns Approx over [n * Ho * Wo, Cout]. MIOpen has no fp64
    convolution: unfold + matmul, one picture and at most `band` output pixels at a time."""
    n, H, W, C = x.shape
    w2 = _d(w).reshape(w.shape[0], -1)                     # (cin, ky, kx) order: unfold's order
    K = w2.shape[1]
    ts, es = [], []
    for b in range(n):
        cols = _cols(_d(x[b]), k, s, p)
        for r0 in range(0, cols.shape[0], band):
            acc, e = _contract(cols[r0:r0 + band], w2, bias)
            ts.append(acc)
            es.append(e)
    assert K == C * k * k
    return Approx(torch.cat(ts), torch.cat(es))


def tconv2x2(x, w):
    """x [n, H, W, Cin] fp16, w [4 = dy * 2 + dx, Cout, Cin]; returns Approx over [n, 2H, 2W, Cout] (no bias)"""
    n, H, W, C = x.shape
    cout = w.shape[1]
    x2 = x.reshape(-1, C)
    t = torch.empty((n, 2 * H, 2 * W, cout), dtype=torch.float64, device=x.device)
    e = torch.empty_like(t)
    for qd in range(4):
        dy, dx = qd >> 1, qd & 1
        acc, ee = _contract(x2, w[qd], None)
        t[:, dy::2, dx::2, :] = acc.view(n, H, W, cout)
        e[:, dy::2, dx::2, :] = ee.view(n, H, W, cout)
    return Approx(t, e)


# ---------------------------------------------------------------------------------------------- chains
class Mid:
    """an fp16 value a kernel stores and reads back: `mid` (float64 on the fp16 grid) and the radius `rad` of the interval
    the stored value may take; an exact input has rad = 0"""
    __slots__ = ("mid", "rad")

    def __init__(self, mid, rad):
        self.mid, self.rad = mid, rad

    @staticmethod
    def exact(x):
        x = _d(x)
        return Mid(x, torch.zeros_like(x))

    @staticmethod
    def of(ap):
        lo, hi = interval(ap)
        mid = reference16(ap)
        return Mid(mid, torch.maximum(hi - mid, mid - lo))

    def rows(self, sl):
        return Mid(self.mid[sl], self.rad[sl])


def _mid(x):
    return x if isinstance(x, Mid) else Mid.exact(x)


def dwconv3x3(x, taps, n, H, W):
    """depthwise 3x3, zero padding: x [n * H * W, C] (fp16 or `Mid`), taps [9][C] (tap = ky * 3 + kx); returns Approx over
    [n * H * W, C]. Shifted float64 slices, one picture at a time."""
    xm = _mid(x)
    C = xm.mid.shape[-1]
    w = _d(taps)
    ts, es = [], []
    for b in range(n):
        sl = slice(b * H * W, (b + 1) * H * W)
        m = F.pad(xm.mid[sl].reshape(H, W, C), (0, 0, 1, 1, 1, 1))
        r = F.pad(xm.rad[sl].reshape(H, W, C), (0, 0, 1, 1, 1, 1))
        t = torch.zeros((H, W, C), dtype=torch.float64, device=m.device)
        mag = torch.zeros_like(t)
        rr = torch.zeros_like(t)
        for ky in range(3):
            for kx in range(3):
                wk = w[ky * 3 + kx]
                s, sr = m[ky:ky + H, kx:kx + W], r[ky:ky + H, kx:kx + W]
                t += s * wk
                mag += (s.abs() + sr) * wk.abs()
                rr += sr * wk.abs()
        ts.append(t.reshape(H * W, C))
        es.append(((9 * U32 + 9 * 2.0 ** -52) * mag + rr).reshape(H * W, C))
    return Approx(torch.cat(ts), torch.cat(es))


def ffn(y1, w0, b0, w2, b2, r2=None, q=None, q2=None):
    """ffn.0 + ffn.2: t = chunk_add(WSiLU(W0 y1 + b0)) -> fp16; y = (W2 t + b2 + y1 [+ r2]) [* q] -> fp16 [* q2].
    y1 [P, C] fp16 or `Mid`; returns {"t": Approx, "y": Approx}"""
    y1 = _mid(y1)
    t = conv1x1(y1, w0, b0, wsilu=True, chunk_add=True)
    y = conv1x1(Mid.of(t), w2, b2, r1=y1, r2=r2, q=q, q2=q2)
    return {"t": t, "y": y}


def pair(x, wa, ba, w1, b1):
    """a block's adaptor and its dc.0: y = Wa x + ba -> fp16; t1 = WSiLU(W1 y + b1) -> fp16"""
    y = conv1x1(x, wa, ba)
    return {"y": y, "t1": conv1x1(Mid.of(y), w1, b1, wsilu=True)}


def dcb(x, w3, b3, w0, b0, w2, b2, t2=None, t1=None, taps=None, geom=None, w1=None, b1=None, shortcut=False, q=None, q2=None,
        w1n=None, b1n=None, wfin=None, bfin=None, qfin=None, band=1 << 15):
    """every stored output of one DepthConvBlock behind its dc.0, in the launch order of the fused kernels:
         [t1 = WSiLU(W1 x + b1)]          dc.0 inside (dcb_tail with w1)              -> fp16
         [t2 = depthwise3x3(t1)]          taps [9][CI], geom = (n, H, W)              -> fp16
         y1 = W3 t2 + b3 + x                                                          -> fp16
         t  = chunk_add(WSiLU(W0 y1 + b0))                                            -> fp16
         y  = (W2 t + b2 + y1 [+ x]) [* q] -> fp16 [* q2]
         then t1n = WSiLU(W1n y + b1n) (the next block's dc.0) or yfin = (Wfin y + bfin) [* qfin] (the closing conv)
    entering at t2 (given), at t1 (t1 + taps + geom) or at x (w1 / b1 + taps + geom). x and the entry operand are fp16 inputs.
    Returns {name: Approx} over [P, width] for t1 (dc.0 inside), t2 (depthwise), y1, t, y and "next" (when there is a NEXT
    slot). The 1x1 chain runs in bands of `band` pixels."""
    out = {}
    if w1 is not None:
        out["t1"] = conv1x1(x, w1, b1, wsilu=True)
        t1 = Mid.of(out["t1"])
    if t1 is not None:
        n, H, W = geom
        out["t2"] = dwconv3x3(t1, taps, n, H, W)
        t2 = Mid.of(out["t2"])
    t2 = _mid(t2)
    P = t2.mid.shape[0]
    parts = {}
    for r0 in range(0, P, band):
        sl = slice(r0, min(P, r0 + band))
        xs = x[sl]
        y1 = conv1x1(t2.rows(sl), w3, b3, r1=xs)
        y1m = Mid.of(y1)
        f = ffn(y1m, w0, b0, w2, b2, r2=xs if shortcut else None, q=q, q2=q2)
        st = {"y1": y1, "t": f["t"], "y": f["y"]}
        if w1n is not None:
            st["next"] = conv1x1(Mid.of(f["y"]), w1n, b1n, wsilu=True)
        elif wfin is not None:
            st["next"] = conv1x1(Mid.of(f["y"]), wfin, bfin, q=qfin)
        for k, v in st.items():
            parts.setdefault(k, []).append(v)
    for k, vs in parts.items():
        out[k] = Approx(torch.cat([v.t for v in vs]), torch.cat([v.e for v in vs]),
                        vs[0].q2 if vs[0].q2 is not None else None)
    return out


def rows_of(ap, sl):
    """the Approx of a slice of pixels"""
    return Approx(ap.t[sl], ap.e[sl], ap.q2)


# ---------------------------------------------------------------------------------------------- checks
def interval(ap):
    """[lo, hi] (float64 on the fp16 grid) that the kernel's fp16 result must lie in"""
    lo = round16(ap.t - ap.e)
    hi = round16(ap.t + ap.e)
    if ap.q2 is not None:
        a, b = round16(lo * ap.q2), round16(hi * ap.q2)
        lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    return lo, hi


def reference16(ap):
    r = round16(ap.t)
    return r if ap.q2 is None else round16(r * ap.q2)


def check(got, ap, what="", sharp_bias=False):
    """got: the kernel's fp16 tensor, same shape as ap.t. Returns a dict of statistics; raises AssertionError on any element
    outside its interval, any non-finite result where the reference is finite, or a rounding bias."""
    st = stats(got, ap, sharp_bias)
    assert st["bad"] == 0, "%s: %d of %d elements outside the fp64 bound (worst %.2f ulp, first at %s: got %r, ref %r, "\
        "interval [%r, %r])" % (what, st["bad"], st["n"], st["max_ulp"], st["first"], st["first_got"], st["first_ref"],
                                st["first_lo"], st["first_hi"])
    assert abs(st["bias"]) <= BIAS_LIMIT, "%s: rounding bias %.3f ulp (limit %.2f)" % (what, st["bias"], BIAS_LIMIT)
    return st


def stats(got, ap, sharp_bias=False):
    """sharp_bias: the rounding-bias statistic over the elements whose interval holds at most two fp16 values only (chained
    references: behind an ambiguous intermediate the distance to reference16 of the midpoints says nothing about rounding)"""
    g = got.to(ap.t.device).to(torch.float64)
    lo, hi = interval(ap)
    ref = reference16(ap)
    ok = (g >= lo) & (g <= hi)
    bad = ~ok
    nb = int(bad.sum())
    u = ulp16(ref)
    fin = torch.isfinite(ref) & torch.isfinite(g)
    d = torch.where(fin, (g - ref) / u, torch.zeros_like(g))
    sgn = torch.sign(ref)
    nz = fin & (sgn != 0)
    if sharp_bias:
        nz = nz & (hi - lo <= torch.maximum(ulp16(lo), ulp16(hi)))
    bias = float((sgn[nz] * d[nz]).mean()) if bool(nz.any()) else 0.0
    out = dict(n=g.numel(), bad=nb, max_ulp=float(d.abs().max()) if g.numel() else 0.0, bias=bias,
               exact=float((g == ref).double().mean()) if g.numel() else 1.0)
    if nb:
        idx = tuple(int(i) for i in torch.nonzero(bad)[0])
        out.update(first=idx, first_got=float(g[idx]), first_ref=float(ref[idx]), first_lo=float(lo[idx]),
                   first_hi=float(hi[idx]))
    return out


def accepts(got, ap, sharp_bias=False, exact_floor=0.0):
    """True when `got` passes both checks (for the CPU tests that show the helper rejects wrong outputs) and, for chained
    references, at least `exact_floor` of its elements equal reference16"""
    st = stats(got, ap, sharp_bias)
    return st["bad"] == 0 and abs(st["bias"]) <= BIAS_LIMIT and st["exact"] >= exact_floor


# ---------------------------------------------------------------------------------------------- input distributions
DISTS = ("normal", "wide", "near_overflow")


def inputs(kind, xshape, N, seed, device="cpu"):
    """activations [..., K], weights [N, K], bias [N] (fp16) of one of DISTS:
      normal         x ~ N(0, 1), w ~ N(0, 1 / K), bias ~ N(0, 0.25)
      wide           x channels scaled by 2^-10 .. 2^6, every 7th pixel row exactly zero, 1 % subnormal entries, every 5th
                     output channel's weights zero
      near_overflow  like normal, each output channel's weights and bias scaled so that |x w + bias| reaches ~ 2.4e4
                     (see `fit_overflow`, which the caller applies with its own K-contraction)"""
    g = torch.Generator().manual_seed(seed)
    K = xshape[-1]
    x = torch.randn(xshape, generator=g)
    w = torch.randn((N, K), generator=g) / math.sqrt(K)
    b = torch.randn((N,), generator=g) * 0.5
    if kind == "wide":
        sc = torch.pow(2.0, torch.randint(-10, 7, (K,), generator=g).double()).float()
        x = x * sc
        w = w / torch.sqrt(sc) / 4.0
        x2 = x.reshape(-1, K)
        x2[::7] = 0.0
        sub = torch.rand(x2.shape, generator=g) < 0.01
        x2[sub] = (torch.randint(-1023, 1024, (int(sub.sum()),), generator=g).float() * 2.0 ** -24)
        x = x2.reshape(xshape)
        w[::5] = 0.0
    elif kind != "normal" and kind != "near_overflow":
        raise ValueError(kind)
    return x.half().to(device), w.half().to(device), b.half().to(device)


def fit_overflow(w, b, peak, target=2.4e4):
    """scale output channel n of (w, b) by target / peak[n] (peak: max |acc| of the channel with the unscaled operands)"""
    s = (target / peak.double().clamp(min=1e-3)).clamp(max=2.0 ** 14)
    w2 = (w.double() * s[:, None]).half()
    b2 = (b.double() * s).half()
    return w2, b2
