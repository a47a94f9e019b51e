"""The float64 reference and its tolerance model (tests/f64_ref.py), fixed and checked on the CPU before any GPU run uses them:

* the per-step MFMA constants hold on every result recorded on MI355X (tests/golden/mfma_probe.npz) and are tight there;
* the oracle (bit-exact to the hardware, test_oracle_cpu.py / test_kernels_gpu.py) stays inside the bound for the K values
  and input distributions of test_gemm_matrix_gpu.py, for every epilogue, the k x k convs and the transposed conv;
* the check REJECTS deliberately wrong outputs: rounded toward zero, one ulp off on 1 % of the elements, the bias shifted by
  one channel, q2 applied before the fp16 rounding, chunk-add summed in another order of magnitude;
* the WSiLU table (arith.h, tools/gen_wsilu_table.py) meets its claimed figures against float64 v * sigmoid(4 v) on every
  segment boundary's neighbourhood, the clamp points, a dense sweep of [-8, 8] and large values up to 65504."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_ref as R  # noqa: E402
from oracle import nn  # noqa: E402

KS = (64, 192, 576, 3456)


def _np(t):
    return None if t is None else t.cpu().numpy()


# ---------------------------------------------------------------------------------------------- fp16 grid helpers
def test_round16_is_fp16_rounding():
    g = torch.Generator().manual_seed(1)
    v = torch.cat([torch.randn(200000, generator=g) * s for s in (1e-7, 1e-5, 1e-2, 1.0, 300.0, 2e4)]
                  + [torch.tensor([0.0, -0.0, 65504.0, 65519.0, 65520.0, -65520.0, 2.0 ** -25, 3 * 2.0 ** -26])])
    r = R.round16(v.double())
    want = v.half().double()                 # float32 -> fp16: one rounding, the reference semantics
    assert torch.equal(r, want)
    u = R.ulp16(want[torch.isfinite(want)])
    assert float(u.min()) == 2.0 ** -24 and float(R.ulp16(torch.tensor([1.0]))) == 2.0 ** -10


# ---------------------------------------------------------------------------------------------- MFMA step constants
def test_mfma_step_bound_on_probe_data(golden_dir):
    d = np.load(os.path.join(golden_dir, "mfma_probe.npz"))
    ab = d["a"].astype(np.float64) * d["b"].astype(np.float64)
    c = d["c"].astype(np.float64)
    got = d["d"].astype(np.float64)
    exact = c + ab.sum(1)                    # exact: 16 products of fp16 and one float32 fit float64's 53 bits here
    G, C = np.abs(ab).sum(1), np.abs(c)
    err = np.abs(got - exact)
    bound = R.U32 * (R.MFMA_ALPHA * G + R.MFMA_BETA * C)
    print("MFMA probe: %d results, worst err / bound %.4f, worst err / (|c| + sum|ab|) = 2^%.2f" %
          (len(c), float((err / np.maximum(bound, 1e-300)).max()), np.log2((err / np.maximum(G + C, 1e-300)).max())))
    assert (err <= bound).all()
    # tight: one unit less on either constant and the recorded hardware breaks it
    assert (err > R.U32 * ((R.MFMA_ALPHA - 1) * G + R.MFMA_BETA * C)).any()
    assert (err > R.U32 * (R.MFMA_ALPHA * G + (R.MFMA_BETA - 0.5) * C)).any()
    # c_acc of one 16-product step covers it too (|c| <= |c| + sum|ab|)
    assert (err <= R.c_acc(16) * (G + C)).all()


# ---------------------------------------------------------------------------------------------- the oracle inside the bound
def _case(kind, P, K, N, seed, chunk=False):
    x, w, b = R.inputs(kind, (P, K), N, seed)
    if kind == "near_overflow":
        peak = (x.float() @ w.float().t() + b.float()).abs().amax(0)
        w, b = R.fit_overflow(w, b, peak, 6e3 if chunk else 2.4e4)
    return x, w, b


EPILOGUES = [dict(), dict(wsilu=True), dict(wsilu=True, chunk_add=True), dict(chunk_add=True), dict(r1=1), dict(r1=1, r2=1),
             dict(q=1), dict(r1=1, q=1), dict(q2=1), dict(r1=1, r2=1, q2=1), dict(wsilu=True, q2=1)]


def _epi_name(e):
    return "+".join(sorted(e)) or "bias"


def _operands(ep, x, N, seed):
    g = torch.Generator().manual_seed(seed + 99)
    P = x.shape[0]
    nout = N // 4 if ep.get("chunk_add") else N
    big = float(x.abs().max()) > 1e3
    rs = 100.0 if big else 1.0
    r1 = (torch.randn((P, nout), generator=g) * rs).half() if ep.get("r1") else None
    r2 = (torch.randn((P, nout), generator=g) * rs).half() if ep.get("r2") else None
    q = (torch.randn((nout,), generator=g) * 0.25 + 1).half() if ep.get("q") else None
    q2 = (torch.randn((nout,), generator=g) * 0.25 + 1).half() if ep.get("q2") else None
    return r1, r2, q, q2


@pytest.mark.parametrize("kind", R.DISTS)
@pytest.mark.parametrize("K", KS)
def test_oracle_conv1x1_inside_bound(kind, K):
    P, N = 48, 256
    worst = []
    for i, ep in enumerate(EPILOGUES):
        x, w, b = _case(kind, P, K, N, 10 * K + i, bool(ep.get("chunk_add")))
        r1, r2, q, q2 = _operands(ep, x, N, i)
        orc = nn.conv1x1(_np(x), _np(w), _np(b), r1=_np(r1), r2=_np(r2), q=_np(q), q2=_np(q2), wsilu=bool(ep.get("wsilu")),
                         chunk_add=bool(ep.get("chunk_add")))
        assert np.isfinite(orc).all()
        ap = R.conv1x1(x, w, b, r1=r1, r2=r2, q=q, q2=q2, wsilu=bool(ep.get("wsilu")), chunk_add=bool(ep.get("chunk_add")))
        st = R.check(torch.from_numpy(orc), ap, "oracle conv1x1 %s K=%d %s" % (kind, K, _epi_name(ep)))
        worst.append((_epi_name(ep), st["max_ulp"], st["exact"]))
    print("K=%d %s: %s" % (K, kind, ", ".join("%s %.1f ulp (%.3f exact)" % t for t in worst)))


def test_oracle_near_overflow_reaches_fp16_range():
    x, w, b = _case("near_overflow", 256, 192, 64, 5)
    orc = nn.conv1x1(_np(x), _np(w), _np(b))
    assert np.isfinite(orc).all() and 1.5e4 < float(np.abs(orc.astype(np.float32)).max()) < 65504


@pytest.mark.parametrize("kind", R.DISTS)
@pytest.mark.parametrize("k,s,p,n,H,W,cin", [(3, 2, 1, 2, 9, 13, 64), (2, 2, 0, 1, 8, 10, 128), (3, 1, 1, 3, 5, 7, 64)])
def test_oracle_conv_kxk_inside_bound(kind, k, s, p, n, H, W, cin):
    cout = 128
    x, w2, b = R.inputs(kind, (n, H, W, cin), cout, 7 + k + cin)
    w = w2.float().reshape(cout, 1, 1, cin).expand(cout, k * k, 1, cin).clone()
    g = torch.Generator().manual_seed(3)
    w = (w.reshape(cout, k, k, cin) * (1 + 0.1 * torch.randn((cout, k, k, cin), generator=g))).permute(0, 3, 1, 2) / k
    w = w.half()
    if kind == "near_overflow":
        ap0 = R.conv_kxk(x, w, b, k, s, p)
        w, b = R.fit_overflow(w.reshape(cout, -1), b, ap0.t.abs().amax(0))
        w = w.reshape(cout, cin, k, k)
    ap = R.conv_kxk(x, w, b, k, s, p)
    orc = np.concatenate([nn.conv_kxk(_np(x[i]), _np(w), _np(b), k, s, p).reshape(-1, cout) for i in range(n)])
    R.check(torch.from_numpy(orc), ap, "oracle conv_kxk k%d s%d %s" % (k, s, kind))


@pytest.mark.parametrize("kind", R.DISTS)
def test_oracle_tconv2x2_inside_bound(kind):
    n, H, W, cin, cout = 2, 5, 6, 192, 128
    x, w2, _ = R.inputs(kind, (n, H, W, cin), 4 * cout, 17)
    if kind == "near_overflow":
        w2, _ = R.fit_overflow(w2, torch.zeros(4 * cout).half(), (x.reshape(-1, cin).float() @ w2.float().t()).abs().amax(0))
    wq = w2.view(4, cout, cin)
    ap = R.tconv2x2(x, wq)
    wpt = wq.permute(1, 0, 2).reshape(4 * cout, cin)           # PyTorch SubpelConv2x order: channel = co * 4 + q
    orc = np.stack([nn.subpel_conv1x1(_np(x[i]), _np(wpt)) for i in range(n)])
    R.check(torch.from_numpy(orc), ap, "oracle tconv2x2 %s" % kind)


# ---------------------------------------------------------------------------------------------- the check rejects wrong outputs
def _rtz16(t):
    u = R.ulp16(t)
    return torch.sign(t) * torch.floor(t.abs() / u) * u


@pytest.mark.parametrize("K", (64, 576, 3456))
def test_check_rejects_wrong_outputs(K):
    P, N = 64, 256
    x, w, b = _case("normal", P, K, N, 400 + K)
    q2 = (torch.randn((N,), generator=torch.Generator().manual_seed(4)) * 0.3 + 1).half()
    ap = R.conv1x1(x, w, b)
    orc = torch.from_numpy(nn.conv1x1(_np(x), _np(w), _np(b)))
    assert R.accepts(orc, ap)
    # (1) rounded toward zero instead of to nearest
    assert not R.accepts(_rtz16(ap.t), ap)
    # (2) one ulp off on 1 % of the elements
    g = torch.Generator().manual_seed(K)
    sel = torch.rand(orc.shape, generator=g) < 0.01
    sgn = torch.where(torch.rand(orc.shape, generator=g) < 0.5, -1.0, 1.0).double()
    o64 = orc.double()
    off = torch.where(sel, o64 + sgn * R.ulp16(o64), o64)
    st = R.stats(off, ap)
    print("K=%d: one-ulp mutation on %d elements, %d rejected" % (K, int(sel.sum()), st["bad"]))
    # every element the mutation moves out of its interval is caught; at small |y| the contraction bound spans an ulp, so
    # only a share of the one-ulp moves leave it (about 3 in 4 at K = 576, 1 in 14 at K = 3456)
    assert not R.accepts(off, ap) and st["bad"] >= (0.5 if K <= 64 else 0.25 if K <= 576 else 0.04) * int(sel.sum())
    # (3) the bias of the neighbouring channel
    orc_b = torch.from_numpy(nn.conv1x1(_np(x), _np(w), _np(torch.roll(b, 1))))
    assert not R.accepts(orc_b, ap)
    # (4) q2 folded into the fused multiply (one rounding) instead of applied to the rounded output
    ap2 = R.conv1x1(x, w, b, q2=q2)
    orc2 = torch.from_numpy(nn.conv1x1(_np(x), _np(w), _np(b), q2=_np(q2)))
    assert R.accepts(orc2, ap2)
    fused = torch.from_numpy(nn.conv1x1(_np(x), _np(w), _np(b), q=_np(q2)))
    st = R.stats(fused, ap2)
    print("K=%d: q2 before rounding: %d of %d rejected" % (K, st["bad"], st["n"]))
    # (the two differ by an ulp where the product lands near a rounding boundary: at K = 3456 the contraction's own bound
    # covers that, so it is seen only at the smaller K)
    assert st["bad"] > 0 or K > 576


def test_check_rejects_chunk_and_wsilu_mutations():
    P, K, N = 64, 192, 512
    x, w, b = _case("normal", P, K, N, 77)
    ap = R.conv1x1(x, w, b, wsilu=True, chunk_add=True)
    assert R.accepts(torch.from_numpy(nn.conv1x1(_np(x), _np(w), _np(b), wsilu=True, chunk_add=True)), ap)
    # chunk-add of the wrong four channels (groups shifted by one channel)
    acc = x.double() @ w.double().t() + b.double()
    v = R.wsilu64(acc)
    shifted = torch.roll(v, 1, dims=1).view(P, N // 4, 4).sum(-1)
    assert not R.accepts(R.round16(shifted), ap)
    # SiLU instead of WSiLU (sigmoid(v) for sigmoid(4 v))
    silu = (acc * torch.sigmoid(acc)).view(P, N // 4, 4).sum(-1)
    assert not R.accepts(R.round16(silu), ap)
    # one table row off: segment 140's coefficients perturbed by 1e-4 relative on c0
    vv = acc.float().numpy()
    ref = nn.wsilu(vv).astype(np.float64)
    seg = ((np.minimum(np.maximum(vv, -4.0), 3.998046875) + np.float32(4100.0)).view(np.uint32) >> 6) & 0xFF
    mut = np.where(seg == 140, ref * (1 + 2e-3), ref)
    mut_sum = torch.from_numpy(mut).view(P, N // 4, 4).sum(-1)
    hit = int((seg == 140).sum())
    assert hit > 0 and not R.accepts(R.round16(mut_sum), ap)


# ---------------------------------------------------------------------------------------------- WSiLU figures
SEG_W = 1.0 / 32


def _f32_neighbours(c, n):
    """the n float32 values on each side of float32 c, c included"""
    c = np.float32(c)
    up, dn = [c], [c]
    for _ in range(n):
        up.append(np.nextafter(up[-1], np.float32(np.inf)))
        dn.append(np.nextafter(dn[-1], np.float32(-np.inf)))
    return np.array(dn[::-1] + up[1:], dtype=np.float32)


def _f32_run(c, n):
    """2n + 1 consecutive float32 around c (vectorised nextafter via the bit pattern; c != 0)"""
    c = np.float32(c)
    bits = np.array([c], dtype=np.float32).view(np.int32)[0]
    k = np.arange(-n, n + 1, dtype=np.int64)
    if c > 0:
        b = bits + k
    else:
        b = bits - k
    return np.sort(b.astype(np.int32).view(np.float32))


def _wsilu_sweep():
    vals = []
    for i in range(257):
        bnd = -4.0 + i * SEG_W
        # the 2^-11 neighbourhood: sampled evenly, plus every float32 within 4096 ulps of the boundary and of both 2^-12
        # ties (the segment of v comes from ROUNDING v + 4100, whose ulp is 2^-11: the polynomial of the segment above is
        # used down to 2^-12 below the boundary)
        vals.append(np.linspace(bnd - 2.0 ** -11, bnd + 2.0 ** -11, 8193).astype(np.float32))
        for c in (bnd, bnd - 2.0 ** -12, bnd + 2.0 ** -12):
            if c == 0.0:
                vals.append(np.concatenate([_f32_run(2.0 ** -40, 4096), -_f32_run(2.0 ** -40, 4096), [0.0]]).astype(np.float32))
            else:
                vals.append(_f32_run(c, 4096))
    for c in (-4.0, 3.998046875, 4.0):
        vals.append(_f32_run(c, 200000))
    vals.append(np.arange(-8.0, 8.0, 2.0 ** -15, dtype=np.float64).astype(np.float32))
    big = np.exp(np.linspace(np.log(8.0), np.log(65504.0), 100000)).astype(np.float32)
    vals += [big, -big, np.array([65504.0, -65504.0, 1000.0, -1000.0, 8.0, -8.0], np.float32)]
    return np.concatenate(vals)


def test_wsilu_figures_hold():
    v = _wsilu_sweep()
    got = nn.wsilu(v).astype(np.float64)
    t = torch.from_numpy(v.astype(np.float64))
    exact = R.wsilu64(t).numpy()
    err = np.abs(got - exact)
    i = int(err.argmax())
    m = np.abs(v) >= 2.0 ** -10                 # sigma4 recovered as wsilu(v) / v (one float32 rounding: 2^-24 relative)
    sig_err = np.abs(got[m] / v[m].astype(np.float64) - torch.sigmoid(4 * t).numpy()[m]) - 2.0 ** -24
    print("WSiLU over %d float32 values: max |err| %.4e at v = %r; sigma4 max |err| %.4e" % (v.size, err[i], float(v[i]),
                                                                                               sig_err.max()))
    assert err.max() <= R.C_ACT                 # arith.h / gen_wsilu_table.py: 5.1e-7
    assert sig_err.max() <= 1.5e-6              # arith.h: 1.5e-6
    assert err.max() > 0.9 * R.C_ACT            # and the constant is not loose
    # the Lipschitz constant the tolerance carries the accumulator's error through
    s = torch.sigmoid(4 * t)
    assert float((s + 4 * t * s * (1 - s)).abs().max()) <= R.L_WSILU
    # outside [-4, 4) the constant rows: exactly v above, exactly zero below
    hi = v >= 4.0
    lo = v < -4.0
    assert np.array_equal(got[hi], v[hi].astype(np.float64)) and not np.any(got[lo])


def test_wsilu_segment_choice_matches_table_generator():
    """the segment index nn.wsilu (the oracle) uses is the generator's: the polynomial of segment i reproduces wsilu at a
    value inside segment i and in the rounded-sum sliver just below it"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gen_wsilu_table as gen
    bnd = np.array([-4.0 + i * SEG_W for i in range(1, 256)], dtype=np.float32)
    for v in (bnd, bnd - np.float32(2.0 ** -12), bnd - np.float32(2.0 ** -12) - np.float32(2.0 ** -13)):
        seg = gen.segment(v)
        x = (np.minimum(np.maximum(v, np.float32(-4)), np.float32(3.998046875)) + np.float32(4100)).astype(np.float32)
        assert np.array_equal(seg, (x.view(np.uint32) >> 6) & 0xFF)
    # the tie at boundary - 2^-12 rounds to even: upward into the next segment exactly when the sum's last bit is even
    sl = gen.segment(bnd - np.float32(2.0 ** -12))
    assert set(np.unique(sl - gen.segment(bnd - np.float32(2.0 ** -11)))) <= {0, 1}
