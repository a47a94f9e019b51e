"""The symbol kernels (kernels/symbols.hip) at their edges, on a real MI355X (-m gpu), through the C ABI and bit-exact against
oracle/symbols_np.py: the int8 clamp and the infinities, every fp16 bit pattern as a scale on both sides of the skip threshold,
block-count geometries around the 2048-symbol workgroup, operands as channel slices of wider rows, the decoder's own compaction
layout, batches, and the closure through the product's rANS coder. tests/symbol_cases.py builds the inputs and
tests/test_symbol_cases_cpu.py proves that they reach those edges. No refusal is tried here (tests/test_ops_refusals_cpu.py)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symbol_cases as S  # noqa: E402
from gpu_util import SENT8, Rows, at as _at, guarded as _guarded, tail_intact as _tail_intact  # noqa: E402
from gpu_util import call as _call, stream as _stream  # noqa: E402

pytestmark = pytest.mark.gpu

F16 = np.float16
SENT = S.SENT


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "needs the MI355X"
    from gpu_util import Ops
    return Ops()


# ------------------------------------------------------------------------------------------------------------ the y steps
def _lds(C, wide):
    """ldy, lds, ldm, ldacc: all C, or all different from C and from each other"""
    return (C + 8, C + 16, C + 24, C + 32) if wide else (C, C, C, C)


def run_y_enc(ops, pics, H, W, C, thres, wide=False, batched=None):
    """The four encoder steps over n pictures (pics: list of {"y", "scales": [4], "means": [4]}). n = 1 goes through the single
    entry point unless batched. -> per step {"sym" [n][cnt], "cond", "count", "acc"}, totals [n][4], compacted [n][4 cnt],
    and whether every sentinel survived."""
    n = len(pics)
    batched = n > 1 if batched is None else batched
    cnt = S.geometry_count(H, W, C)
    nb = S.symbol_blocks(cnt)
    ldy, lds, ldm, ldacc = _lds(C, wide)
    y = Rows(np.concatenate([p["y"].reshape(-1, C) for p in pics]), C, ldy)
    acc = Rows(None, C, ldacc, fill=(n * H * W, 7.0))
    sym = _guarded(n * cnt, torch.int16)
    cond = _guarded(n * cnt // 8, torch.uint8)
    count = _guarded(n * nb, torch.int32)
    comp = _guarded(n * 4 * cnt, torch.int16)
    totals = _guarded(n * 4, torch.int32)
    steps = []
    intact = True
    for k in range(4):
        sc = Rows(np.concatenate([p["scales"][k].reshape(-1, C) for p in pics]), C, lds)
        mn = Rows(np.concatenate([p["means"][k].reshape(-1, C) for p in pics]), C, ldm)
        if batched:
            _call(ops.y_step_enc_b, y.ptr(), ldy, sc.ptr(), lds, mn.ptr(), ldm, acc.ptr(), ldacc, _at(sym), _at(cond), _at(count),
                  _at(comp), 4 * cnt, _at(totals), 4, k, H, W, C, k, thres, n, _stream())
        else:
            _call(ops.y_step_enc, y.ptr(), ldy, sc.ptr(), lds, mn.ptr(), ldm, acc.ptr(), ldacc, _at(sym), _at(cond), _at(count),
                  _at(comp), _at(totals), H, W, C, k, thres, _stream())
        torch.cuda.synchronize()
        intact = intact and sc.around_intact() and mn.around_intact()
        steps.append({"sym": sym[:n * cnt].cpu().numpy().reshape(n, cnt), "cond": cond[:n * cnt // 8].cpu().numpy().reshape(n, -1),
                      "count": count[:n * nb].cpu().numpy().reshape(n, nb), "acc": acc.get().reshape(n, H, W, C)})
    intact = (intact and y.around_intact() and acc.around_intact() and _tail_intact(sym, n * cnt) and _tail_intact(cond, n * cnt // 8)
              and _tail_intact(count, n * nb) and _tail_intact(comp, n * 4 * cnt) and _tail_intact(totals, n * 4))
    return {"steps": steps, "totals": totals[:n * 4].cpu().numpy().reshape(n, 4),
            "comp": comp[:n * 4 * cnt].cpu().numpy().reshape(n, 4 * cnt), "intact": intact}


def run_y_dec(ops, pics, H, W, C, thres, decode, wide=False, batched=None, own_layout=False):
    """The decoder's four steps: index + compaction, decode(b, k, compacted indexes) -> int8 symbols, restore.
    own_layout: the intra decoder's buffers (dmci.hip) - one region per (picture, step), the step's count in the region's first
    16 bytes, the indexes behind them, slot 0 - otherwise one buffer per picture that the steps fill one after the other
    (slot = step), as the encoder's."""
    n = len(pics)
    batched = (n > 1 or own_layout) if batched is None else batched
    assert batched or not own_layout
    cnt = S.geometry_count(H, W, C)
    nb = S.symbol_blocks(cnt)
    _, lds, ldm, ldacc = _lds(C, wide)
    acc = Rows(None, C, ldacc, fill=(n * H * W, -3.0))
    index = _guarded(n * cnt, torch.uint8)
    cond = _guarded(n * cnt // 8, torch.uint8)
    count = _guarded(n * nb, torch.int32)
    region = (16 + cnt + 15) // 16 * 16
    cidx = _guarded(n * 4 * region if own_layout else n * 4 * cnt, torch.uint8)
    totals = _guarded(n * 4, torch.int32)
    decoded = _guarded(n * 4 * cnt, torch.int8)
    steps = []
    intact = True
    kept = np.zeros((n, 4), np.int64)
    for k in range(4):
        sc = Rows(np.concatenate([p["scales"][k].reshape(-1, C) for p in pics]), C, lds)
        mn = Rows(np.concatenate([p["means"][k].reshape(-1, C) for p in pics]), C, ldm)
        if own_layout:
            _call(ops.y_step_dec_index_b, sc.ptr(), lds, _at(index), _at(cond), _at(count), _at(cidx, k * region + 16), 4 * region,
                  _at(cidx, k * region), region, 0, H, W, C, k, thres, n, _stream())
        elif batched:
            _call(ops.y_step_dec_index_b, sc.ptr(), lds, _at(index), _at(cond), _at(count), _at(cidx), 4 * cnt, _at(totals), 4, k,
                  H, W, C, k, thres, n, _stream())
        else:
            _call(ops.y_step_dec_index, sc.ptr(), lds, _at(index), _at(cond), _at(count), _at(cidx), _at(totals), H, W, C, k, thres,
                  _stream())
        torch.cuda.synchronize()
        host = cidx.cpu().numpy()
        compacted = []
        for b in range(n):
            if own_layout:
                at = (b * 4 + k) * region
                kept[b, k] = int(host[at:at + 4].view(np.int32)[0])
                assert (host[at + 4:at + 16] == SENT8).all(), "the 12 bytes between count and indexes"
                ci = host[at + 16:at + 16 + kept[b, k]]
                to = (b * 4 + k) * cnt
            else:
                kept[b, k] = int(totals[b * 4 + k])
                base = int(kept[b, :k].sum())
                ci = host[b * 4 * cnt + base:b * 4 * cnt + base + kept[b, k]]
                to = b * 4 * cnt + base
            compacted.append(ci.copy())
            dec = decode(b, k, compacted[-1])
            assert dec.dtype == np.int8 and dec.size == kept[b, k]
            if dec.size:
                decoded[to:to + dec.size] = torch.from_numpy(dec).cuda()
        if own_layout:
            _call(ops.y_step_dec_restore_b, _at(decoded, k * cnt), 4 * cnt, _at(cond), _at(count), _at(cidx, k * region), region, 0,
                  mn.ptr(), ldm, acc.ptr(), ldacc, H, W, C, k, n, _stream())
        elif batched:
            _call(ops.y_step_dec_restore_b, _at(decoded), 4 * cnt, _at(cond), _at(count), _at(totals), 4, k,
                  mn.ptr(), ldm, acc.ptr(), ldacc, H, W, C, k, n, _stream())
        else:
            _call(ops.y_step_dec_restore, _at(decoded), _at(cond), _at(count), _at(totals), mn.ptr(), ldm, acc.ptr(), ldacc,
                  H, W, C, k, _stream())
        torch.cuda.synchronize()
        intact = intact and sc.around_intact() and mn.around_intact()
        steps.append({"idx": index[:n * cnt].cpu().numpy().reshape(n, cnt), "cond": cond[:n * cnt // 8].cpu().numpy().reshape(n, -1),
                      "count": count[:n * nb].cpu().numpy().reshape(n, nb), "acc": acc.get().reshape(n, H, W, C),
                      "compacted": compacted})
    host = cidx.cpu().numpy()
    if own_layout:
        for r in range(n * 4):          # behind each region's indexes
            intact = intact and bool((host[r * region + 16 + kept[r // 4, r % 4]:(r + 1) * region] == SENT8).all())
    else:
        for b in range(n):
            intact = intact and bool((host[b * 4 * cnt + kept[b].sum():(b + 1) * 4 * cnt] == SENT8).all())
    intact = (intact and acc.around_intact() and _tail_intact(index, n * cnt) and _tail_intact(cond, n * cnt // 8)
              and _tail_intact(count, n * nb) and _tail_intact(cidx, cidx.numel() - 16) and _tail_intact(decoded, n * 4 * cnt))
    return {"steps": steps, "kept": kept, "intact": intact}


def _block_sums(keep):
    nb = S.symbol_blocks(keep.size)
    padded = np.zeros(nb * S.BLOCK, np.int32)
    padded[:keep.size] = keep
    return padded.reshape(nb, S.BLOCK).sum(axis=1)


def check_enc(got, want, what=""):
    """got: run_y_enc's result, want: one oracle chain (symbol_cases.y_steps) per picture"""
    assert got["intact"], "a sentinel was overwritten " + what
    for b, chain in enumerate(want):
        base = 0
        cnt = chain[0]["sym"].size
        for k in range(4):
            g, w = got["steps"][k], chain[k]
            tag = "%s picture %d step %d" % (what, b, k)
            assert np.array_equal(g["sym"][b], w["sym"]), "symbols " + tag
            assert np.array_equal(g["cond"][b], np.packbits(w["keep"], bitorder="little")), "keep bytes " + tag
            assert np.array_equal(g["count"][b], _block_sums(w["keep"])), "block counts " + tag
            assert not np.isnan(g["acc"][b]).any() and np.array_equal(g["acc"][b], w["acc"]), "y_hat_so_far " + tag
            kept = int(w["keep"].sum())
            assert got["totals"][b, k] == kept, "total " + tag
            assert np.array_equal(got["comp"][b, base:base + kept], w["sym"][w["keep"]]), "compacted symbols " + tag
            base += kept
        assert (got["comp"][b, base:].view(np.uint16) == SENT).all(), "behind the compacted symbols " + what
        assert base <= 4 * cnt


def check_dec(got, want, what=""):
    assert got["intact"], "a sentinel was overwritten " + what
    for b, chain in enumerate(want):
        for k in range(4):
            g, w = got["steps"][k], chain[k]
            tag = "%s picture %d step %d" % (what, b, k)
            assert np.array_equal(g["idx"][b], w["idx"]), "indexes " + tag
            assert np.array_equal(g["cond"][b], np.packbits(w["keep"], bitorder="little")), "keep bytes " + tag
            assert np.array_equal(g["count"][b], _block_sums(w["keep"])), "block counts " + tag
            assert got["kept"][b, k] == int(w["keep"].sum()), "total " + tag
            assert np.array_equal(g["compacted"][b], w["idx"][w["keep"]]), "compacted indexes " + tag
            assert not np.isnan(g["acc"][b]).any() and np.array_equal(g["acc"][b], w["acc"]), "decoder y_hat_so_far " + tag


def _from_oracle(want):
    """decode(b, k, indexes): the symbols that the oracle's encoder kept"""
    def decode(b, k, idx):
        w = want[b][k]
        return (w["sym"][w["keep"]] >> 8).astype(np.int8)
    return decode


def _pic(y, scales, means):
    return {"y": y, "scales": scales if isinstance(scales, list) else [scales] * 4,
            "means": means if isinstance(means, list) else [means] * 4}


def _oracle(pic, thres):
    return S.y_steps(pic["y"], pic["scales"], pic["means"], thres)


def _both_sides(ops, pics, H, W, C, thres, what="", **how):
    want = [_oracle(p, thres) for p in pics]
    enc = run_y_enc(ops, pics, H, W, C, thres, wide=how.get("wide", False), batched=how.get("batched"))
    check_enc(enc, want, what)
    dec = run_y_dec(ops, pics, H, W, C, thres, _from_oracle(want), **how)
    check_dec(dec, want, what)
    return want, enc, dec


# ------------------------------------------------------------------------------------------------------------ the sweeps
@functools.lru_cache(maxsize=None)
def _scale_sweep():
    return S.scale_sweep()


@functools.lru_cache(maxsize=None)
def _quant_sweep():
    return S.quant_sweep()


@functools.lru_cache(maxsize=None)
def _quant_oracle(thres):
    c = _quant_sweep()
    return _oracle(_pic(c["y"], c["scales"], c["means"]), thres)


@pytest.mark.parametrize("thres", S.THRESHOLDS)
def test_scale_sweep_y_steps(ops, thres):
    """every fp16 bit pattern as a scale, in every step: table index, packed symbol, keep flag, counts, compaction"""
    c = _scale_sweep()
    _both_sides(ops, [_pic(c["y"], c["scales"], c["means"])], c["H"], c["W"], c["C"], thres)


@pytest.mark.parametrize("thres", S.THRESHOLDS)
def test_quant_sweep_y_steps(ops, thres):
    """every non-NaN fp16 pattern as y against six means: the clamp at -128 and +127, the packing there, ties, +-Inf, an
    overflowing y - mean; encoder and both decoder kernels"""
    c = _quant_sweep()
    pic = _pic(c["y"], c["scales"], c["means"])
    want = [_quant_oracle(thres)]
    check_enc(run_y_enc(ops, [pic], c["H"], c["W"], c["C"], thres), want)
    check_dec(run_y_dec(ops, [pic], c["H"], c["W"], c["C"], thres, _from_oracle(want)), want)


def run_mask_steps(ops, y, q_dec, scales, means, nsteps, thres):
    """encoder and decoder of the full-tensor steps, operands as channel slices of wider rows -> what symbol_cases.mask_steps
    returns, once from the encoder and once from the decoder"""
    H, W, C = y.shape
    n = H * W * C
    nb = S.symbol_blocks(n)
    yd, qd, sd = Rows(y, C, C + 8), Rows(q_dec, C, C + 16), Rows(scales, C, C + 24)
    md = [Rows(m, C, C + 32) for m in means]
    yh = Rows(None, C, 2 * C, fill=(H * W, 5.0))
    sym, cond, count = _guarded(n, torch.int16), _guarded(n // 8, torch.uint8), _guarded(nb, torch.int32)
    comp, totals = _guarded(n, torch.int16), _guarded(1, torch.int32)
    for k in range(nsteps):
        _call(ops.mask_step_enc, yd.ptr(), yd.ld, qd.ptr(), qd.ld, sd.ptr(), sd.ld, md[k].ptr(), md[k].ld, yh.ptr(), yh.ld,
              _at(sym), _at(cond), _at(count), _at(comp), _at(totals), H, W, C, nsteps, k, thres, _stream())
    torch.cuda.synchronize()
    kept = int(totals[0])
    enc = {"y_div": yd.get().reshape(H, W, C), "sym": sym[:n].cpu().numpy(), "cond": cond[:n // 8].cpu().numpy(),
           "count": count[:nb].cpu().numpy(), "y_hat": yh.get().reshape(H, W, C), "kept": kept, "comp": comp[:n].cpu().numpy(),
           "intact": all(r.around_intact() for r in [yd, qd, sd, yh] + md) and _tail_intact(sym, n) and _tail_intact(cond, n // 8)
           and _tail_intact(count, nb) and _tail_intact(comp, n) and _tail_intact(totals, 1)}
    index, cidx, totals_d = _guarded(n, torch.uint8), _guarded(n, torch.uint8), _guarded(1, torch.int32)
    cond_d, count_d = _guarded(n // 8, torch.uint8), _guarded(nb, torch.int32)
    _call(ops.mask_dec_index, sd.ptr(), sd.ld, _at(index), _at(cond_d), _at(count_d), _at(cidx), _at(totals_d), H, W, C, thres, _stream())
    torch.cuda.synchronize()
    kept_d = int(totals_d[0])
    decoded = _guarded(n, torch.int8)
    if kept_d == kept and kept:
        decoded[:kept] = (comp[:kept] >> 8).to(torch.int8)
    yq = _guarded(n, torch.int8)
    yh_d = Rows(None, C, 2 * C, fill=(H * W, -3.0))
    for k in range(nsteps):
        _call(ops.mask_step_dec, _at(decoded), _at(cond_d), _at(count_d), _at(totals_d), _at(yq), md[k].ptr(), md[k].ld, qd.ptr(), qd.ld,
              yh_d.ptr(), yh_d.ld, H, W, C, nsteps, k, _stream())
    torch.cuda.synchronize()
    dec = {"idx": index[:n].cpu().numpy(), "cond": cond_d[:n // 8].cpu().numpy(), "count": count_d[:nb].cpu().numpy(), "kept": kept_d,
           "cidx": cidx[:n].cpu().numpy(), "y_hat": yh_d.get().reshape(H, W, C),
           "intact": yh_d.around_intact() and all(_tail_intact(t, c) for t, c in ((index, n), (cidx, n), (cond_d, n // 8), (count_d, nb),
                                                                                    (yq, n), (totals_d, 1)))}
    return enc, dec


def check_mask_steps(enc, dec, want):
    keep = want["keep"]
    kept = int(keep.sum())
    assert enc["intact"] and dec["intact"], "a sentinel was overwritten"
    assert np.array_equal(enc["y_div"], want["y_div"]), "y / max(q, 0.5)"
    assert np.array_equal(enc["sym"], want["sym"]), "symbols"
    for side in (enc, dec):
        assert np.array_equal(side["cond"], np.packbits(keep, bitorder="little")), "keep bytes"
        assert np.array_equal(side["count"], _block_sums(keep)), "block counts"
        assert side["kept"] == kept, "total"
        assert not np.isnan(side["y_hat"]).any() and np.array_equal(side["y_hat"], want["y_hat"]), "y_hat"
    assert np.array_equal(enc["comp"][:kept], want["sym"][keep]) and (enc["comp"][kept:].view(np.uint16) == SENT).all()
    assert np.array_equal(dec["idx"], want["idx"]), "indexes"
    assert np.array_equal(dec["cidx"][:kept], want["idx"][keep]) and (dec["cidx"][kept:] == SENT8).all()


@pytest.mark.parametrize("nsteps", [2, 4])
@pytest.mark.parametrize("thres", S.THRESHOLDS)
def test_scale_sweep_mask_steps(ops, nsteps, thres):
    c = _scale_sweep()
    means = c["means"][:nsteps]
    enc, dec = run_mask_steps(ops, c["y"], c["q_dec"], c["scales"], means, nsteps, thres)
    check_mask_steps(enc, dec, S.mask_steps(c["y"], c["q_dec"], c["scales"], means, nsteps, thres))


@pytest.mark.parametrize("nsteps,thres", [(2, 0.15), (4, 0.0)])
def test_quant_sweep_mask_steps(ops, nsteps, thres):
    """the clamps, the infinities and q_dec below 0.5 and at 65504 through the inter models' encoder and decoder steps"""
    c = _quant_sweep()
    means = [c["means"]] * nsteps
    enc, dec = run_mask_steps(ops, c["y"], c["q_dec"], c["scales"], means, nsteps, thres)
    want = S.mask_steps(c["y"], c["q_dec"], c["scales"], means, nsteps, thres)
    sym = want["sym"].astype(np.int32) >> 8
    assert (sym[want["keep"]] == 127).sum() >= 1000 and (sym[want["keep"]] == -128).sum() >= 1000 and np.isinf(want["y_div"]).any()
    check_mask_steps(enc, dec, want)


# ------------------------------------------------------------------------------------------------------------ through the coder
@pytest.mark.parametrize("own_layout,parallel", [(False, 1), (True, 4), (False, 4), (True, 1)])
def test_closure_through_the_coder(ops, golden_dir, own_layout, parallel):
    """encoder kernels -> RansEncoder -> RansDecoder on the indexes that y_step_dec_index compacted -> y_step_dec_restore: the
    decoder's y_hat_so_far equals the encoder's and the oracle's, with the clamped symbols and all 128 tables in the stream"""
    import dcvc_amd
    dcvc_amd.install_plugin()
    import MLCodec_extensions_cpp as mine
    g = np.load(os.path.join(golden_dir, "rans_golden.npz"))
    assert g["y_len"].size == 128
    thres = 0.0                                   # every scale of the sweep is kept: all 128 tables code symbols
    c = _quant_sweep()
    H, W, C = c["H"], c["W"], c["C"]
    pic = _pic(c["y"], c["scales"], c["means"])
    want = [_quant_oracle(thres)]
    enc = run_y_enc(ops, [pic], H, W, C, thres)
    check_enc(enc, want)
    tot = enc["totals"][0]
    base = np.concatenate([[0], np.cumsum(tot)])
    coded = [enc["comp"][0, base[k]:base[k + 1]] for k in range(4)]
    every = np.concatenate(coded)
    assert len(set(every & 0xff)) == 128 and (every >> 8).min() == -128 and (every >> 8).max() == 127
    z = np.array([-64, 63, 0, 1, -1], dtype=np.int8)
    e = mine.RansEncoder()
    e.set_cdf(g["z_cdf"], g["z_len"], 0)
    e.set_cdf(g["y_cdf"], g["y_len"], 1)
    e.reset()
    e.set_entropy_coder_parallel(parallel)
    for k in (3, 2, 1, 0):                        # the decoder reads them back first to last (dmci.hip pushes them this way)
        e.encode_y(np.ascontiguousarray(coded[k]))
    e.encode_z(z, 128, 128)
    e.flush()
    d = mine.RansDecoder()
    d.set_cdf(g["z_cdf"], g["z_len"], 0)
    d.set_cdf(g["y_cdf"], g["y_len"], 1)
    d.set_entropy_coder_parallel(parallel)
    d.set_stream(e.get_encoded_stream())
    d.decode_z(z.size, 128, 128)
    assert np.array_equal(d.get_decoded_tensor(), z)

    def decode(b, k, idx):
        if idx.size == 0:
            return np.zeros(0, np.int8)
        d.decode_y(np.ascontiguousarray(idx))
        return np.array(d.get_decoded_tensor(), dtype=np.int8).reshape(-1)

    dec = run_y_dec(ops, [pic], H, W, C, thres, decode, own_layout=own_layout)
    check_dec(dec, want)
    assert np.array_equal(dec["steps"][3]["acc"], enc["steps"][3]["acc"])


# ------------------------------------------------------------------------------------------------------------ keep patterns
@pytest.mark.parametrize("pattern", ["nothing", "everything", "last"])
def test_keep_patterns(ops, pattern):
    H, W, C = 17, 30, 128
    cq = C // 4
    y, means = S.mild((H, W, C), 6.0, 201), S.mild((H, W, C), 2.0, 202)
    scales = S.mild_scales((H, W, C), 203)
    if pattern == "nothing":
        scales = np.minimum(scales, F16(0.15))                 # at the threshold is not above it
    elif pattern == "everything":
        scales = np.maximum(scales, F16(0.1501))
    else:
        scales = np.minimum(scales, F16(0.15))
        scales[H - 1, W - 1, cq - 1::cq] = F16(2.0)            # the last symbol of every step, whichever group is active
    want, enc, dec = _both_sides(ops, [_pic(y, scales, means)], H, W, C, 0.15, pattern)
    expect = {"nothing": 0, "everything": H * W * cq, "last": 1}[pattern]
    assert (enc["totals"] == expect).all() and (dec["kept"] == expect).all()
    if pattern == "nothing":
        assert (enc["comp"].view(np.uint16) == SENT).all()
    if pattern == "last":
        assert all(w["keep"][-1] and w["keep"].sum() == 1 for w in want[0])


# ------------------------------------------------------------------------------------------------------------ geometries
@pytest.mark.parametrize("H,W,C", [g[:3] for g in S.GEOMETRIES], ids=["%dx%dx%d" % g[:3] for g in S.GEOMETRIES])
def test_geometry(ops, H, W, C):
    """block counts around the workgroup size, ragged last blocks, a second pass over the earlier blocks' counts; operands as
    channel slices of wider rows with sentinels around every output"""
    pic = _pic(S.mild((H, W, C), 6.0, 401), [S.mild_scales((H, W, C), 410 + k) for k in range(4)],
               [S.mild((H, W, C), 2.0, 420 + k) for k in range(4)])
    _both_sides(ops, [pic], H, W, C, 0.15, wide=True)


def test_own_layout_across_blocks(ops):
    """the decoder's own layout where the rank of a symbol needs the counts of earlier blocks"""
    H, W, C = 17, 30, 128
    pic = _pic(S.mild((H, W, C), 6.0, 431), [S.mild_scales((H, W, C), 440 + k) for k in range(4)],
               [S.mild((H, W, C), 2.0, 450 + k) for k in range(4)])
    _both_sides(ops, [pic], H, W, C, 0.15, wide=True, own_layout=True)


# ------------------------------------------------------------------------------------------------------------ batches
def _batch(n, H, W, C):
    skipped = _pic(S.mild((H, W, C), 6.0, 501), np.minimum(S.mild_scales((H, W, C), 502), F16(0.15)), S.mild((H, W, C), 2.0, 503))
    kept = _pic(S.mild((H, W, C), 6.0, 511), [np.maximum(S.mild_scales((H, W, C), 512 + k), F16(0.1501)) for k in range(4)],
                [S.mild((H, W, C), 2.0, 520 + k) for k in range(4)])
    q = S.quant_picture(H, W, C)
    quant = _pic(q["y"], q["scales"], q["means"])
    if n == 2:                                  # the swept picture doubles as the one that keeps everything
        return [skipped, _pic(q["y"], np.maximum(q["scales"], F16(0.1501)), q["means"])]
    return [kept, skipped, quant]


@pytest.mark.parametrize("own_layout", [False, True])
@pytest.mark.parametrize("n,H,W", [(2, 5, 3), (3, 5, 3), (2, 17, 30), (3, 17, 30)])
def test_batches(ops, n, H, W, own_layout):
    """blockIdx.y = picture: every picture of a batch gets what a launch of its own gives it, bit for bit, and what the oracle
    gives it; its masks follow its own rows (an odd height: stacking would shift them)"""
    C = 128
    thres = 0.15
    pics = _batch(n, H, W, C)
    want, enc, dec = _both_sides(ops, pics, H, W, C, thres, "batch", wide=True, own_layout=own_layout)
    for b, p in enumerate(pics):
        one_e = run_y_enc(ops, [p], H, W, C, thres, wide=True)
        one_d = run_y_dec(ops, [p], H, W, C, thres, _from_oracle([want[b]]), wide=True)
        assert one_e["intact"] and one_d["intact"]
        assert np.array_equal(one_e["totals"][0], enc["totals"][b]) and np.array_equal(one_d["kept"][0], dec["kept"][b])
        assert np.array_equal(one_e["comp"][0].view(np.uint16), enc["comp"][b].view(np.uint16))
        for k in range(4):
            for a in ("sym", "cond", "count"):
                assert np.array_equal(one_e["steps"][k][a][0], enc["steps"][k][a][b]), (a, b, k)
            for a in ("idx", "cond", "count"):
                assert np.array_equal(one_d["steps"][k][a][0], dec["steps"][k][a][b]), (a, b, k)
            assert np.array_equal(one_d["steps"][k]["compacted"][0], dec["steps"][k]["compacted"][b])
            assert np.array_equal(one_e["steps"][k]["acc"][0].view(np.uint16), enc["steps"][k]["acc"][b].view(np.uint16))
            assert np.array_equal(one_d["steps"][k]["acc"][0].view(np.uint16), dec["steps"][k]["acc"][b].view(np.uint16))
    assert (enc["totals"][n - 2] == 0).all() and (enc["totals"][0 if n == 3 else 1] == H * W * C // 4).all()
