"""tests/module_cases.py checked without a GPU: the table names every place the codecs call the module layer, its grids sit on
both sides of each launch choice (the thresholds restated here and compared with the sources), the float64 block reference
agrees with a plain nn-style float64 forward, and the numpy restatement of DcbW::load's bias fold gives the hand-computed
values of a three-channel example (tests/test_modules_gpu.py runs the same example through DcbW::load on the device, which
load() needs for its uploads)."""
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_cases as B  # noqa: E402
import f64_ref as R  # noqa: E402
import module_cases as M  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dcvc_amd", "csrc")


def _src(*parts):
    with open(os.path.join(CSRC, *parts)) as f:
        return f.read()


def _site_functions(site):
    f, rest = site.split(" ", 1)
    return f, [n.strip() for n in re.sub(r"\(.*?\)", "", rest).split(",")]


# ---------------------------------------------------------------------------------------------- call sites
def test_table_names_every_call_site():
    sites = {c["site"] for c in M.CASES}
    assert not [s for s in M.CALL_SITES if s not in sites], "call sites without a case"
    assert not [s for s in sites if s not in M.CALL_SITES and not s.startswith("none")], "cases with an unknown call site"
    for c in M.CASES:
        assert c["site"].startswith("none") or c["site"] in M.CALL_SITES


def test_call_sites_are_the_codecs():
    """every member function of the three codecs that calls the module layer is named by the table, and every name exists"""
    named = {}
    for site in M.CALL_SITES:
        f, fns = _site_functions(site)
        named.setdefault(f, set()).update(fns)
    for f in ("dmci.hip", "dmc_ld.hip", "dmc_ht.hip"):
        src = re.sub(r"//[^\n]*", "", _src("codec", f))
        defs = list(re.finditer(r"^\w[\w \*]*\b\w+Codec::(\w+)\(", src, re.M))
        calling = set()
        for i, m in enumerate(defs):
            body = src[m.end():defs[i + 1].start() if i + 1 < len(defs) else len(src)]
            if re.search(r"\bm_\w+(\[[^\]]*\])?\.forward\(|\brun_dcb_chain\(", body):
                calling.add(m.group(1))
        assert calling, f
        assert calling == named[f], "%s: functions that call the layer %s, named by the table %s" % (f, sorted(calling), sorted(named[f]))


def test_shapes_are_what_the_codecs_load():
    """the block shapes of the table against dcvc_amd/arch.py (the checkpoints' inventory, itself held to the kCh* constants)"""
    from dcvc_amd import arch
    found = set()
    for spec in (arch.dmci_spec(), arch.dmc_ld_spec(), arch.dmc_ht_spec(True), arch.dmc_ht_spec(False)):
        for name, shape in spec.items():
            if name.endswith(".dc.0.weight"):
                p = name[:-len("dc.0.weight")]
                cin = spec[p + "adaptor.weight"][1] if p + "adaptor.weight" in spec else 0
                found.add((shape[1], shape[0], spec[p + "ffn.0.weight"][0] // 4, cin))
    table = {v for k, v in M.SHAPES.items() if not k.startswith("x_")}
    assert table <= found, "shapes no codec loads: %s" % sorted(table - found)
    # the adaptors differ only in their input width; every (c, cdc, cffn) of the codecs is in the table
    assert {s[:3] for s in found} == {s[:3] for s in table}
    for k, v in M.SHAPES.items():
        if k.startswith("x_"):
            assert v[:3] not in {s[:3] for s in found}, k
    fins = set()
    for spec in (arch.dmci_spec(), arch.dmc_ld_spec(), arch.dmc_ht_spec(True), arch.dmc_ht_spec(False)):
        for name in ("y_prior_fusion.conv.3", "y_spatial_prior.conv.3", "y_spatial_prior.conv.2", "decoder.conv2", "recon_head.head",
                     "recon_head.conv2.0.3", "recon_head.conv.0.5"):
            if name + ".weight" in spec and len(spec[name + ".weight"]) == 4 and name + ".dc.0.weight" not in spec:
                fins.add((spec[name + ".weight"][1], spec[name + ".weight"][0]))
    assert {v for k, v in M.FINS.items() if not k.startswith("x_")} <= fins


# ---------------------------------------------------------------------------------------------- thresholds
def test_thresholds_match_the_sources():
    tail = _src("kernels", "dcb_tail.hip")
    assert re.search(r"constexpr int PH = %d\b" % M.PATCH_H, tail) or re.search(r"\bPH = %d\b" % M.PATCH_H, tail)
    assert re.search(r"\bPW = %d\b" % M.PATCH_W, tail)
    assert "patches >= %d" % M.TAIL_PATCHES in tail
    assert "pixels >= 128 * 192" in _src("kernels", "ffn_fused.hip") and M.FFN_PIXELS == 128 * 192
    assert M.WIDE_PIXELS == 64 * 200 and re.search(r"64 \* 200", _src("kernels", "dcb_nsplit.hip") + _src("kernels", "dcb_nsplit_common.h"))


def _block_grids():
    """(shape, H, W, batch, in place, closing conv width) of every block the table runs"""
    out = []
    for c in M.CASES:
        for call in c["calls"]:
            if call["op"] == "subpel":
                continue
            H, W = M.call_grid(c, call)
            shapes = M.block_shapes(c, call["mod"])
            if call["op"] == "block":
                shapes = [shapes[call["i"]]]
            elif call["op"] == "chain":
                shapes = shapes[call["first"]:call["first"] + call["n"]] if call["n"] else shapes[call["first"]:]
            for i, s in enumerate(shapes):
                last = i == len(shapes) - 1
                if call["op"] == "block":
                    inpl = call["x"][:2] == call["y"][:2]
                elif call["op"] == "chain":
                    src = call["x"] if i == 0 else call["tmp"]
                    dst = call["y"] if last else call["tmp"]
                    inpl = call["tmp2"] is None and src[:2] == dst[:2]
                else:
                    inpl = False            # (tmp == y is redirected for the one-launch blocks)
                fn = call.get("fin") if last else None
                out.append((s, H, W, c["batch"], inpl, M.FINS[c["mods"][fn["mod"]][1]][1] if fn else None))
    return out


def test_grids_sit_on_both_sides_of_each_flip():
    grids = _block_grids()
    # 64-pixel workgroups: an N-split block below and at 64 * 200 pixels; the (384, 192) depthwise flips with it
    for pick in (lambda s: M.is_nsplit(*s[:3]) and s[0] < 768, lambda s: s[:3] == (384, 192, 192)):
        ps = {H * W for s, H, W, n, _, _ in grids if pick(s)}
        assert any(p < M.WIDE_PIXELS for p in ps) and any(p >= M.WIDE_PIXELS for p in ps)
        assert max(p for p in ps if p < M.WIDE_PIXELS) == 99 * 128 and min(p for p in ps if p >= M.WIDE_PIXELS) == 100 * 128
    # 192 patches: a 256-wide block that is not an N-split block
    pt = {(M.patches(H, W), H * W) for s, H, W, n, _, _ in grids if s[0] == 256 and not M.is_nsplit(*s[:3]) and s[1] <= 128}
    assert (180, 96 * 240) in pt and (192, 96 * 256) in pt
    assert any(p >= M.TAIL_PATCHES and px < M.FFN_PIXELS for p, px in pt), "no ragged grid at 192 patches under 128 * 192 pixels"
    # 128 * 192 pixels: a block that is neither (ffn_fused or the plain launches)
    px = {H * W for s, H, W, n, _, _ in grids if s[:3] == M.SHAPES["x_ffn"][:3]}
    assert max(p for p in px if p < M.FFN_PIXELS) == 96 * 240 and min(p for p in px if p >= M.FFN_PIXELS) == 96 * 256
    # partial patches / tiles and the minimum
    hw = {(H, W) for _, H, W, _, _, _ in grids}
    assert {(9, 17), (5, 3), (1, 1)} <= hw
    assert {n for _, _, _, n, _, _ in grids} == {1, 2, 3}
    assert max(M.pixels_of(c, b) * c["bufs"][b][0] for c in M.CASES for b in c["bufs"]) <= 100 * 128 * 768


def test_table_predicts_every_branch():
    reached = set()
    for c in M.CASES:
        for call in c["calls"]:
            reached |= M.predict_call(c, call)
    assert reached | set(M.UNREACHABLE) >= set(M.BRANCHES), sorted(set(M.BRANCHES) - reached)
    one = lambda name: [c for c in M.CASES if c["name"] == name][0]
    # the in-place adaptor keeps out of the pair launch; Stride2W with tmp == y keeps the one-launch block
    assert "pair" not in M.predict_call(one("ld-fa_m-one-block-9x17"), one("ld-fa_m-one-block-9x17")["calls"][0])
    assert "pair" in M.predict_call(one("ld-fa_m-9x17"), one("ld-fa_m-9x17")["calls"][0])
    assert M.predict_call(one("ld-hyper-enc-18x34"), one("ld-hyper-enc-18x34")["calls"][1]) == {"tail+dc0"}
    assert M.predict_call(one("x-tail256-96x256"), one("x-tail256-96x256")["calls"][0]) == {"tail+dc0", "tail", "fin_behind"}
    assert M.predict_call(one("x-tail256-96x240"), one("x-tail256-96x240")["calls"][0]) == {"plain", "fin_behind"}


def test_classify_reads_the_variant_words():
    v = B.variant_bits
    assert M.classify([v(("nsplit8", 384, 192, 1, 1, 1))], True, False) == {"nsplit32", "dw_inside"}
    assert M.classify([v(("pair8", 192, 384, 384, 2)), 0x2, v(("nsplit8", 384, 384, 2, 512, 0))], True, True) == \
        {"pair", "nsplit64", "dw_outside", "fin_inside"}
    assert M.classify([v(("tail", 256, True, False, True)), 0x0], True, True) == {"tail+dc0", "fin_behind"}
    assert M.classify([v(("tail", 128, True, True, False))], True, False) == {"tail"}
    assert M.classify([0x2, 0x8, v(("ffn", 256, True, False))], True, False) == {"ffn_fused"}
    assert M.classify([0x2, 0x8, 0x6, 0x18], True, False) == {"plain"}
    assert M.classify([0x0], False, False) == set()


def test_cases_are_well_formed():
    for c in M.CASES:
        sd = None
        for call in c["calls"]:
            for k in ("x", "y", "tmp", "tmp2", "alt"):
                v = call.get(k)
                if v is not None:
                    assert v[0] in c["bufs"] and v[1] % 8 == 0 and v[1] + v[2] <= c["bufs"][v[0]][0], (c["name"], k, v)
            for q in (call.get("qf"), call.get("qa"), (call.get("fin") or {}).get("q")):
                assert q is None or q in c["qs"], (c["name"], q)
        assert set(c["temps"]) <= set(c["bufs"]), c["name"]
        # every operand has the rows its call touches
        for call in c["calls"]:
            hi, wi = M.call_in_grid(c, call)
            ho, wo = (2 * hi, 2 * wi) if call["op"] == "subpel" else M.call_grid(c, call)
            need = {"x": hi * wi, "y": ho * wo, "tmp": ho * wo, "tmp2": ho * wo, "alt": ho * wo}
            for k, px in need.items():
                if call.get(k) is not None:
                    assert M.pixels_of(c, call[k][0]) == c["batch"] * px, (c["name"], k)
            if call.get("fin"):
                v = call["fin"]["y"]
                assert M.pixels_of(c, v[0]) == c["batch"] * ho * wo and v[1] + v[2] <= c["bufs"][v[0]][0], (c["name"], "fin")
                assert v[2] == M.FINS[c["mods"][call["fin"]["mod"]][1]][1]
            if call.get("up_tmp"):
                m = c["mods"][call["mod"]]
                cout = M.SHAPES[m[2]][0] if m[0] == "upsample" else m[2]
                assert M.pixels_of(c, call["up_tmp"]) >= hi * wi and c["bufs"][call["up_tmp"]][0] == 4 * cout, c["name"]
            if call["op"] == "stride2":
                assert hi % 2 == 0 and wi % 2 == 0, c["name"]
            # the views are as wide as the modules read and write them
            shapes = M.block_shapes(c, call["mod"])
            if call["op"] == "block":
                s = shapes[call["i"]]
                assert call["x"][2] == (s[3] or s[0]) and call["y"][2] == s[0], c["name"]
            elif call["op"] == "chain":
                sub = shapes[call["first"]:call["first"] + call["n"]] if call["n"] else shapes[call["first"]:]
                assert call["x"][2] == (sub[0][3] or sub[0][0]) and call["y"][2] == sub[-1][0] and call["tmp"][2] == sub[-1][0], c["name"]
            elif call["op"] in ("stride2", "upsample"):
                m = c["mods"][call["mod"]]
                assert call["x"][2] == m[1] and call["y"][2] == shapes[0][0] and call["tmp"][2] == shapes[0][0], c["name"]
            else:
                m = c["mods"][call["mod"]]
                assert call["x"][2] == m[1] and call["y"][2] == m[2], c["name"]
        if c["f64"]:
            assert len(c["calls"]) == 1 and c["calls"][0].get("fin") is None
        del sd
    assert len(M.F64_CASES) >= 20


# ---------------------------------------------------------------------------------------------- the float64 reference
def _nn_case(shape, n, H, W, sc, seed):
    sd = {}
    M.block_weights(sd, "B.", M.SHAPES[shape])
    c, _, _, cin = M.SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, H, W, cin or c), generator=g).half()
    q = (torch.randn((c,), generator=g) * 0.25 + 1).clamp(0.5, 1.5).half()
    return sd, x, q


def test_f64_block_agrees_with_nn_forward():
    """f64_block rounds its five intermediates (adaptor, dc.0, depthwise, dc.3, chunk-add) to fp16, 2^-11 relative each, and
    every stage passes a perturbation on with a gain of order one (weights of variance 1 / K, residual branches halved): the two
    agree to a few 2^-11 of the output's norm. 2^-8 allows eight of them; a structural difference (tap order, chunk order, a
    missing residual) is of order one."""
    for shape, n, H, W, sc in (("l_fai0", 1, 5, 3, False), ("i_128", 2, 4, 5, True), ("x_tail256", 1, 3, 3, True), ("l_128", 1, 9, 4, False)):
        sd, x, q = _nn_case(shape, n, H, W, sc, 7)
        ap = M.f64_block(R, sd, "B.", x.reshape(-1, x.shape[-1]), (n, H, W), sc=sc, q=q)
        want = M.nn_block64(sd, "B.", x.double().permute(0, 3, 1, 2), sc=sc, q=q).permute(0, 2, 3, 1).reshape(ap.t.shape)
        rel = float((ap.t - want).norm() / want.norm())
        assert rel < 2.0 ** -8, (shape, rel)
        assert bool((ap.e > 0).all()) and bool(torch.isfinite(ap.e).all()), shape
        # teeth: the taps in checkpoint order (not transposed) are another block
        sd2 = dict(sd)
        sd2["B.dc.2.weight"] = sd["B.dc.2.weight"].flip(-1)
        other = M.nn_block64(sd2, "B.", x.double().permute(0, 3, 1, 2), sc=sc, q=q).permute(0, 2, 3, 1).reshape(ap.t.shape)
        assert float((ap.t - other).norm() / want.norm()) > 2.0 ** -4, shape


def test_f64_stride2_and_upsample_agree_with_nn_forward():
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    # Stride2: pixel_unshuffle(2) + 1x1 conv + block
    c = M.case("t", "none", 6, 4, {"S": ("stride2", 16, "l_128", True)}, {}, [], [M.s2("S", None, None, None)])
    sd = M.case_weights(c)
    x = torch.randn((1, 6, 4, 16), generator=g).half()
    ap = M.f64_call(R, c, sd, x, {})
    t = F.conv2d(F.pixel_unshuffle(x.double().permute(0, 3, 1, 2), 2), sd["S.down.weight"].double(), sd["S.down.bias"].double())
    want = M.nn_block64(sd, "S.conv.", t, sc=True).permute(0, 2, 3, 1).reshape(ap.t.shape)
    assert float((ap.t - want).norm() / want.norm()) < 2.0 ** -8
    # Upsample: 1x1 conv + pixel_shuffle(2) + block
    c = M.case("t", "none", 3, 5, {"U": ("upsample", 16, "l_128", False, 1, False)}, {}, [], [M.ups("U", None, None, None)])
    sd = M.case_weights(c)
    x = torch.randn((1, 3, 5, 16), generator=g).half()
    ap = M.f64_call(R, c, sd, x, {})
    t = F.pixel_shuffle(F.conv2d(x.double().permute(0, 3, 1, 2), sd["U.up.conv.0.weight"].double()), 2)
    want = M.nn_block64(sd, "U.conv.", t).permute(0, 2, 3, 1).reshape(ap.t.shape)
    assert float((ap.t - want).norm() / want.norm()) < 2.0 ** -8


# ---------------------------------------------------------------------------------------------- weight preparation
def test_fold_hand_example():
    h = M.hand_example()
    got = M.fold_bias(h["B.dc.3.weight"], h["B.dc.2.bias"], h["B.dc.3.bias"])
    assert got.dtype == np.float16 and got.tolist() == M.HAND_FOLDED
    # one rounding of the exact sum keeps row 0's last bit: the example tells the two roundings from one
    w, b2, b3 = (h[k].astype(np.float64) for k in ("B.dc.3.weight", "B.dc.2.bias", "B.dc.3.bias"))
    once = (w.reshape(3, 3) @ b2 + b3).astype(np.float16)
    assert once.tolist() == [1.0009765625, 1.0009765625, 0.75]
    taps = M.prep_taps(h["B.dc.2.weight"])
    assert taps.shape == (9, 3) and taps[4, 1] == h["B.dc.2.weight"][1, 0, 1, 1] and taps[2, 0] == h["B.dc.2.weight"][0, 0, 0, 2]


def test_fold_allowance_covers_the_fold():
    """|fold_bias - (W3 b2 + b3)| <= e_fold on the table's weights, and e_fold is of the order of an fp16 ulp of the bias"""
    for shape in ("l_128", "l_fus", "i_384", "h_768", "x_ffn"):
        sd = {}
        M.block_weights(sd, "B.", M.SHAPES[shape])
        got = torch.from_numpy(M.fold_bias(sd["B.dc.3.weight"], sd["B.dc.2.bias"], sd["B.dc.3.bias"]).astype(np.float64))
        s, e = M.fold_bias64(R, sd["B.dc.3.weight"], sd["B.dc.2.bias"], sd["B.dc.3.bias"])
        assert bool(((got - s).abs() <= e).all()), shape
        assert bool((e <= 1.5 * R.ulp16(s.abs() + 1.0)).all()), shape
        assert float(((got - s).abs() / R.ulp16(s)).max()) > 0.25, "the fold's roundings do not show on these weights"


def test_layout_restatements():
    w = np.arange(2 * 12, dtype=np.float16).reshape(2, 12, 1, 1)          # cout 2, cin 3: channel = c * 4 + dy * 2 + dx
    r = M.prep_stride2(w)
    assert r.shape == (2, 4, 3) and r[1, 2, 1] == w[1, 1 * 4 + 2, 0, 0]
    w = np.arange(8 * 3, dtype=np.float16).reshape(8, 3, 1, 1)            # cout 2: row = co * 4 + dy * 2 + dx
    r = M.prep_subpel(w)
    assert r.shape == (4, 2, 3) and r[3, 1, 2] == w[1 * 4 + 3, 2, 0, 0]
    w = np.arange(2 * 3 * 9, dtype=np.float16).reshape(2, 3, 3, 3)
    r = M.prep_convk(w)
    assert r.shape == (2, 3, 3, 3) and r[1, 2, 0, 1] == w[1, 1, 2, 0]


def test_library_exports_the_test_surface():
    import ctypes
    from dcvc_amd import _lib
    for name in ("create", "destroy", "set_param", "load_blocks", "load_stride2", "load_upsample", "load_subpel", "load_fin",
                 "block_info", "read", "scratch", "block_forward", "chain_forward", "chain_forward_qa", "stride2_forward", "upsample_forward",
                 "subpel_forward"):
        _lib.fn("dcvc_modtest_" + name, ctypes.c_int, [])
