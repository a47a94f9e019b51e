"""The chained float64 references of the fused DepthConvBlock kernels (f64_ref.dcb / pair / ffn) on the CPU: the oracle chain
(oracle.nn conv1x1 / dwconv3x3 in the fused kernels' launch order) stays inside the chained bound, near-overflow operands
fitted stage by stage keep every intermediate interval finite, the check rejects wrong blocks, and the GPU case table
(tests/block_cases.py) reaches every instantiation compiled in kernels/dcb_nsplit8_*.hip, dcb_pair8_*.hip, dcb_tail.hip and
ffn_fused.hip."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_cases as B  # noqa: E402
import f64_ref as R  # noqa: E402


def _n(t):
    return None if t is None else t.numpy()


def _wpt(taps):
    CI = taps.shape[1]
    return np.ascontiguousarray(_n(taps).reshape(3, 3, CI).transpose(2, 0, 1)[:, None])


def oracle_chain(op, taps_fn=None, t2_fn=None, sc=None, next_from=None, fin_from=None):
    """the oracle's launch sequence of one block; the keyword arguments build the mutations below"""
    from oracle import nn
    x = _n(op["x"])
    t1 = nn.conv1x1(x, _n(op["w1"]), _n(op["b1"]), wsilu=True) if op.get("w1") is not None else _n(op.get("t1"))
    if t1 is not None:
        n, H, W = op["geom"]
        CI = t1.shape[1]
        if t2_fn is not None:
            t2 = t2_fn(t1)
        else:
            wpt = taps_fn(_wpt(op["taps"])) if taps_fn else _wpt(op["taps"])
            t2 = np.concatenate([nn.dwconv3x3(t1[b * H * W:(b + 1) * H * W].reshape(H, W, CI), wpt).reshape(H * W, CI)
                                 for b in range(n)])
    else:
        t2 = _n(op["t2"])
    y1 = nn.conv1x1(t2, _n(op["w3"]), _n(op["b3"]), r1=x)
    t = nn.conv1x1(y1, _n(op["w0"]), _n(op["b0"]), wsilu=True, chunk_add=True)
    shortcut = op["sc"] if sc is None else sc
    y_pre = nn.conv1x1(t, _n(op["w2"]), _n(op["b2"]), r1=y1, r2=x if shortcut else None, q=_n(op["q"]))
    y = nn.conv1x1(t, _n(op["w2"]), _n(op["b2"]), r1=y1, r2=x if shortcut else None, q=_n(op["q"]), q2=_n(op["q2"]))
    out = {"t2": t2, "y1": y1, "t": t, "y": y}
    src = {"y": y, "y_pre": y_pre, "y1": y1}
    if op.get("w1n") is not None:
        out["next"] = nn.conv1x1(src[next_from or "y"], _n(op["w1n"]), _n(op["b1n"]), wsilu=True)
    elif op.get("wfin") is not None:
        out["next"] = nn.conv1x1(src[fin_from or "y"], _n(op["wfin"]), _n(op["bfin"]), q=_n(op.get("qfin")))
    return out


def _st(got, ap):
    return R.stats(torch.from_numpy(np.asarray(got)) if isinstance(got, np.ndarray) else got, ap, sharp_bias=True)


def _accepts(got, ap, dist):
    got = torch.from_numpy(np.asarray(got)) if isinstance(got, np.ndarray) else got
    return R.accepts(got, ap, sharp_bias=True, exact_floor=B.EXACT_FLOOR[dist])


# ---------------------------------------------------------------------------------------------- the case table
def test_case_table_covers_every_instantiation():
    inst = B.all_instantiations()
    ns = B.nsplit8_instantiations()
    assert len(ns) == 58 and len([k for k in ns if k[5]]) == 13          # 45 block launches + 13 with the depthwise conv inside
    assert len(B.pair8_instantiations()) >= 11 and len(B.tail_instantiations()) == 12 and len(B.ffn_instantiations()) == 12
    got = {}
    for c in B.ALL_CASES:
        k = B.predict(c)
        got.setdefault(k, []).append(B.name(c))
        if c["kind"] == "nsplit8":
            P = c["H"] * c["W"]
            assert c["next"] in (0, 1) or B.fin_supported(c["C"], c["CI"], c["next"]), B.name(c)
            assert not c["dw"] or B.dw_supported(c["C"], c["CI"], P), B.name(c)
            assert not (c["sc"] and c["q"]), "shortcut with q is not a reference op"
        if c["kind"] == "pair8":
            assert B.pair_supported(c["CIN"], c["C"], c["CI"])
    missing = sorted(inst - set(got), key=B.key_name)
    for k in sorted(inst, key=B.key_name):
        print("%-34s %s" % (B.key_name(k), ", ".join(got.get(k, ["-"]))))
    print("instantiations %d, reached %d, missing: %s" % (len(inst), len(inst & set(got)), missing or "none"))
    assert not missing and set(got) <= inst
    # every option at least once per block shape, ragged tiles and the depthwise geometries
    for C, CI in B.NSPLIT_SHAPES:
        cs = [c for c in B.NSPLIT_CASES if (c["C"], c["CI"]) == (C, CI)]
        assert all(any(c[o] for c in cs) for o in ("sc", "q", "q2")), (C, CI)
    assert any(c["H"] * c["W"] == 12801 for c in B.NSPLIT_CASES) and any(c["H"] * c["W"] < 64 for c in B.NSPLIT_CASES)
    dws = [(c["H"], c["W"]) for c in B.NSPLIT_CASES if c["dw"]]
    assert any(h == 1 for h, _ in dws) and any(w == 1 for _, w in dws) and any(w < 64 for _, w in dws)
    assert {2, 3} <= {c["n"] for c in B.TAIL_CASES} and any(c["n"] > 1 and c["H"] % 2 for c in B.TAIL_CASES)
    assert max(c["H"] * c["W"] for c in B.NSPLIT_CASES) <= 1920 * 1088 // 64


def test_wsilu_table_copies_restated():
    """Lay<>::RT: the 384-wide blocks keep a single table copy (NS8_TRIPLE), the others four; the WSiLU edge tests run one
    layout of each kind (test_block_f64_gpu.py EDGE_NSPLIT)"""
    assert B.nsplit8_rt(256, 128, 1) == 4 and B.nsplit8_rt(384, 384, 1) == 1 and B.nsplit8_rt(384, 384, 2) == 1
    assert B.nsplit8_rt(384, 192, 1) == 1 and B.nsplit8_rt(512, 512, 2) == 4
    assert all(B.pair_lay_fits(*s, 1) for s in B.PAIR_SHAPES)


# ---------------------------------------------------------------------------------------------- the oracle chain in the bound
NEXTS = [(C, CI, nx) for C, CI in B.NSPLIT_SHAPES for nx in [0, 1] + list(B.FINS.get((C, CI), ()))]


@pytest.mark.parametrize("dist", R.DISTS)
@pytest.mark.parametrize("C,CI,nx", NEXTS, ids=["%d-%d-%s" % (C, CI, {0: "none", 1: "dc0"}.get(n, "fin%d" % n))
                                                for C, CI, n in NEXTS])
def test_oracle_chain_inside_bound(C, CI, nx, dist):
    """every stored output of the oracle chain inside the chained bound, with the depthwise conv, the shortcut, q or q2 and
    qfin; prints the worst ulp error and the exact share (block_cases.EXACT_FLOOR comes from these lines)"""
    i = NEXTS.index((C, CI, nx))
    sc, q, q2 = i % 2 == 0, i % 2 == 1, i % 3 != 2
    op = B.block_operands(dist, 11 + i, 96, C, CI, entry="t1", geom=(1, 8, 12), nxt=nx, sc=sc and not q, q=q, q2=q2,
                          qf=nx > 1 and q)
    ref = B.block_ref(R, op)
    orc = oracle_chain(op)
    line = []
    for k in ("t2", "y1", "t", "y", "next"):
        if k not in ref:
            continue
        st = _st(orc[k], ref[k])
        assert st["bad"] == 0 and abs(st["bias"]) <= R.BIAS_LIMIT, (k, st)
        if k in ("y", "next"):
            assert st["exact"] >= B.EXACT_FLOOR[dist], (k, st)
        line.append("%s %.1f ulp exact %.4f" % (k, st["max_ulp"], st["exact"]))
    print("%d-%d next %d %-13s %s" % (C, CI, nx, dist, " | ".join(line)))


@pytest.mark.parametrize("dist", R.DISTS)
def test_oracle_pair_tail_ffn_inside_bound(dist):
    from oracle import nn
    for cin, c, ci in B.PAIR_SHAPES:
        op = B.pair_operands(dist, 21, 64, cin, c, ci)
        ref = R.pair(op["x"], op["wa"], op["ba"], op["w1"], op["b1"])
        y = nn.conv1x1(_n(op["x"]), _n(op["wa"]), _n(op["ba"]))
        for k, got in (("y", y), ("t1", nn.conv1x1(y, _n(op["w1"]), _n(op["b1"]), wsilu=True))):
            assert _accepts(got, ref[k], dist), (cin, c, ci, k, _st(got, ref[k]))
    for C, CD, CF in ((128, 64, 64), (256, 128, 128)):           # dcb_tail: dc.0 inside, two pictures
        op = B.block_operands(dist, 22, 2 * 48, C, CD, CF=CF, entry="x", geom=(2, 6, 8), sc=True, q2=True)
        ref = B.block_ref(R, op)
        assert _accepts(oracle_chain(op)["y"], ref["y"], dist)
    for C, CF in ((128, 64), (256, 128), (384, 384)):
        op = B.ffn_operands(dist, 23, 64, C, CF, r2=True, q=True, q2=True)
        ref = R.ffn(op["x"], op["w0"], op["b0"], op["w2"], op["b2"], r2=op["r2"], q=op["q"], q2=op["q2"])
        t = nn.conv1x1(_n(op["x"]), _n(op["w0"]), _n(op["b0"]), wsilu=True, chunk_add=True)
        y = nn.conv1x1(t, _n(op["w2"]), _n(op["b2"]), r1=_n(op["x"]), r2=_n(op["r2"]), q=_n(op["q"]), q2=_n(op["q2"]))
        assert _accepts(y, ref["y"], dist), (C, _st(y, ref["y"]))


@pytest.mark.parametrize("C,CI,nx", [(256, 128, 1), (384, 192, 384), (768, 768, 768), (512, 512, 256)])
def test_near_overflow_fitted_stage_by_stage(C, CI, nx):
    """near_overflow operands: each stage fitted against its float64 value with the earlier stages fitted; every intermediate
    interval stays finite and the chain reaches the upper part of the fp16 range"""
    op = B.block_operands("near_overflow", 31, 96, C, CI, entry="t1", geom=(1, 8, 12), nxt=nx, q=True, q2=True)
    ref = B.block_ref(R, op)
    for k in ("t2", "y1", "t", "y"):
        lo, hi = R.interval(ref[k])
        assert bool(torch.isfinite(lo).all()) and bool(torch.isfinite(hi).all()), k
    assert float(ref["y1"].t.abs().max()) > 1e4 and float(ref["t"].t.abs().max()) > 5e3 and float(ref["y"].t.abs().max()) > 1e4


# ---------------------------------------------------------------------------------------------- the check rejects wrong blocks
def _f64_tail(op, y1, t=None, q2_before=False, shift_chunk=False, seg_perturb=None):
    """ffn.0 + ffn.2 in float64 from a given y1 (fp32 or fp16 values), rounding t (unless given) and y to fp16"""
    x = op["x"].double()
    y1 = torch.as_tensor(np.asarray(y1, dtype=np.float64)) if not torch.is_tensor(y1) else y1.double()
    if t is None:
        acc = y1 @ op["w0"].double().t() + op["b0"].double()
        v = R.wsilu64(acc)
        if seg_perturb is not None:
            from oracle import nn
            vv = acc.float().numpy()
            ref = nn.wsilu(vv).astype(np.float64)
            seg = ((np.minimum(np.maximum(vv, -4.0), 3.998046875) + np.float32(4100.0)).view(np.uint32) >> 6) & 0xFF
            v = torch.from_numpy(np.where(seg == seg_perturb, ref * (1 + 2e-3), ref))
        if shift_chunk:
            v = torch.roll(v, 1, dims=1)
        t = R.round16(v.view(v.shape[0], -1, 4).sum(-1))
    acc = t @ op["w2"].double().t() + op["b2"].double() + y1
    if op["sc"]:
        acc = acc + x
    if op["q"] is not None:
        acc = acc * op["q"].double()
    if op["q2"] is not None:
        return R.round16(acc * op["q2"].double()) if q2_before else R.round16(R.round16(acc) * op["q2"].double())
    return R.round16(acc)


@pytest.mark.parametrize("dist", R.DISTS)
def test_chain_check_rejects_wrong_blocks(dist):
    from oracle import nn
    P, C, CI, H, W = 96, 256, 128, 8, 12
    op = B.block_operands(dist, 41, P, C, CI, entry="t1", geom=(1, H, W), nxt=1, q2=True)
    ref = B.block_ref(R, op)
    good = oracle_chain(op)
    assert _accepts(good["y"], ref["y"], dist) and _accepts(good["next"], ref["next"], dist)
    y1 = good["y1"]
    rejected = {}
    # y1 kept in fp32 (unrounded) / t kept in fp32
    y1f = torch.from_numpy(good["t2"]).double() @ op["w3"].double().t() + op["b3"].double() + op["x"].double()
    rejected["y1 in fp32"] = _f64_tail(op, y1f)
    tf = R.wsilu64(torch.from_numpy(y1).double() @ op["w0"].double().t() + op["b0"].double())
    rejected["t in fp32"] = _f64_tail(op, y1, t=tf.view(P, -1, 4).sum(-1))
    rejected["chunk groups shifted"] = _f64_tail(op, y1, shift_chunk=True)
    rejected["shortcut added when off"] = oracle_chain(op, sc=True)["y"]
    rejected["q2 before rounding"] = _f64_tail(op, y1, q2_before=True)
    rejected["depthwise taps transposed"] = oracle_chain(op, taps_fn=lambda w: np.ascontiguousarray(w.transpose(0, 1, 3, 2)))["y"]

    def wrap(t1):
        """the right neighbour of (r, W-1) is (r + 1, 0): the halo taken from the flat pixel order"""
        t = torch.from_numpy(t1).double()
        taps = op["taps"].double()
        acc = torch.zeros_like(t)
        for ky in range(3):
            for kx in range(3):
                d = (ky - 1) * W + (kx - 1)
                s = torch.zeros_like(t)
                lo, hi = max(0, -d), min(P, P - d)
                s[lo:hi] = t[lo + d:hi + d]
                h = torch.arange(P) // W + ky - 1
                s[(h < 0) | (h >= H)] = 0.0
                acc += s * taps[ky * 3 + kx]
        return R.round16(acc).half().numpy()
    rejected["depthwise halo wraps across a row"] = oracle_chain(op, t2_fn=wrap)["y"]
    for k, got in rejected.items():
        assert not _accepts(got, ref["y"], dist), "%s %s: accepted (%r)" % (dist, k, _st(got, ref["y"]))
    # NEXT slot: dc.0 from y before q2; the closing conv fed y1 instead of y
    assert not _accepts(oracle_chain(op, next_from="y_pre")["next"], ref["next"], dist), "next dc.0 from y before q2"
    opf = B.block_operands(dist, 42, P, C, CI, entry="t2", nxt=192, sc=True)
    reff = B.block_ref(R, opf)
    assert _accepts(oracle_chain(opf)["next"], reff["next"], dist)
    assert not _accepts(oracle_chain(opf, fin_from="y1")["next"], reff["next"], dist), "closing conv fed y1"
    assert not _accepts(oracle_chain(opf, sc=False)["y"], reff["y"], dist), "shortcut left out when on"
    print("%s: rejected %s, next dc.0 before q2, closing conv fed y1, shortcut left out" % (dist, ", ".join(rejected)))
