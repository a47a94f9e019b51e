"""The module layer (dcvc_amd/csrc/codec/modules.{h,hip}) against plain launch sequences and float64 (-m gpu).

DcbW::load / forward, run_dcb_chain / DcbChain, Stride2W, SubpelW, UpsampleW and FinCall, reached through the test surface
include/dcvc_amd_modtest.h with the case table of tests/module_cases.py (one case per way the three codecs call the layer, at
grids either side of every launch choice):

* the prepared weights (taps, folded dc.3 bias, stride-2 and sub-pixel layouts) equal the numpy restatement bit for bit;
* every case equals its plain launch sequence with torch.equal on every buffer the layer defines, sentinels around every
  operand included, and leaves its inputs alone;
* single modules and short chains lie inside the float64 bound of f64_ref (the folded bias as W3 b2 + b3 in float64);
* state: the same call twice, a chain behind one that left Scratch::hand set, a captured and replayed call;
* every refusal of DcbW::forward and run_dcb_chain with its message;
* the launch records of the cases reach every branch of DcbW::forward (test_zz_coverage_report prints them).

Default mode only: the dispatch switches are read once per process, the A/B modes stay with test_fullsize_gpu.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_ref as R  # noqa: E402
import gpu_util as U  # noqa: E402
import module_cases as M  # noqa: E402

SWITCHES = [k for k in os.environ if k.startswith("DCVC_NSPLIT") or k in ("DCVC_DCB_TAIL", "DCVC_FFN_FUSED", "DCVC_PAIR",
                                                                           "DCVC_NO_DCB_CORE")]
pytestmark = [pytest.mark.gpu] + ([pytest.mark.skip(reason="dispatch switches set (%s): these tests pin the default mode"
                                                    % ", ".join(SWITCHES))] if SWITCHES else [])

SENT = U.SENT
COVER = {}                          # case name -> [branches of call 0, of call 1, ...]
vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
REC = np.dtype([("M", np.int32), ("N", np.int32), ("K", np.int32), ("variant", np.int32), ("ms", np.float32)])


class Surface:
    def __init__(self):
        from dcvc_amd import _lib
        f = _lib.fn
        view = [vp, ci, ci]
        self.create = f("dcvc_modtest_create", vp, [cll, ci])
        self.destroy = f("dcvc_modtest_destroy", None, [vp])
        self.set_param = f("dcvc_modtest_set_param", ci, [vp, ctypes.c_char_p, vp, ci, vp, ci])
        self.load_blocks = f("dcvc_modtest_load_blocks", ci, [vp, ctypes.c_char_p, ci])
        self.load_stride2 = f("dcvc_modtest_load_stride2", ci, [vp, ctypes.c_char_p, ci])
        self.load_upsample = f("dcvc_modtest_load_upsample", ci, [vp, ctypes.c_char_p, ci])
        self.load_subpel = f("dcvc_modtest_load_subpel", ci, [vp, ctypes.c_char_p])
        self.load_fin = f("dcvc_modtest_load_fin", ci, [vp, ctypes.c_char_p])
        self.blocks = f("dcvc_modtest_blocks", ci, [vp, ci])
        self.block_info = f("dcvc_modtest_block_info", ci, [vp, ci, ci, ci, ci, ci, ci, vp])
        self.fin_info = f("dcvc_modtest_fin_info", ci, [vp, ci, vp])
        self.read = f("dcvc_modtest_read", cll, [vp, ci, ci, ci, vp, cll])
        self.scratch = f("dcvc_modtest_scratch", ci, [vp, vp, vp, vp, vp])
        self.block_forward = f("dcvc_modtest_block_forward", ci, [vp, ci, ci] + view + view + [ci, ci, ci, vp, vp] + view +
                               [ci, ci, ci, ci, vp, vp, ci, ci, vp])
        self.chain_forward = f("dcvc_modtest_chain_forward", ci, [vp, ci, ci, ci] + view + view + view + [ci, ci, vp] + view +
                               [ci, vp, vp, ci, ci, ci, ci, ci, vp])
        self.chain_forward_qa = f("dcvc_modtest_chain_forward_qa", ci, [vp, ci, ci, ci] + view + view + view + [ci, ci, vp, vp] +
                                  view + [ci, vp, vp, ci, ci, ci, ci, ci, vp])
        self.stride2_forward = f("dcvc_modtest_stride2_forward", ci, [vp, ci] + view + view + view + [ci, ci, vp])
        self.upsample_forward = f("dcvc_modtest_upsample_forward", ci, [vp, ci] + view + view + view + [ci, ci, vp, ci, ci, ci, vp])
        self.subpel_forward = f("dcvc_modtest_subpel_forward", ci, [vp, ci] + view + view + [ci, ci, vp, ci, ci, vp])
        self.prof_en = f("dcvc_gemm_profile_enable", ci, [ci])
        self.prof_reset = f("dcvc_gemm_profile_reset", ci, [])
        self.prof_get = f("dcvc_gemm_profile_launches", cll, [vp, cll])


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "needs the MI355X"
    from dcvc_amd import _lib
    from dcvc_amd.plugin import MLCodec_extensions_cpp  # noqa: F401  (loads the library)
    ops = U.Ops()
    ops.dwconv3x3_b = _lib.fn("dcvc_dwconv3x3_b", ci, [vp, ci, vp, vp, ci, ci, ci, ci, ci, vp])
    ops.conv_kxk_b = _lib.fn("dcvc_conv_kxk_b", ci, [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp])
    ops.tconv2x2_b = _lib.fn("dcvc_tconv2x2_b", ci, [vp, ci, vp, vp, ci, ci, ci, ci, ci, ci, vp])
    return Surface(), ops


class Handle:
    """a test-surface handle with the modules of one or more cases loaded"""

    def __init__(self, mt, cases, elems=None, batch=None, sd=None):
        from dcvc_amd import _lib
        cases = cases if isinstance(cases, (list, tuple)) else [cases]
        self.mt = mt
        self.h = mt.create(elems if elems is not None else max(M.scratch_elems(c) for c in cases),
                           batch if batch is not None else cases[0]["batch"])
        if not self.h:
            raise _lib.DcvcError(_lib.lib().dcvc_last_error().decode())
        self.sd, self.ids = {}, {}
        try:
            for c in cases:
                self.sd.update(sd if sd is not None else M.case_weights(c))
            for name, t in self.sd.items():
                a = M.f16(t)
                dims = (ctypes.c_int64 * a.ndim)(*a.shape)
                _lib.check(mt.set_param(self.h, name.encode(), a.ctypes.data, 0, dims, a.ndim))
            for c in cases:
                for name, mod in c["mods"].items():
                    self.ids[name] = self.load(name, mod)
        except Exception:
            self.close()
            raise

    def load(self, name, mod):
        from dcvc_amd import _lib
        mt, p, kind = self.mt, (name + ".").encode(), mod[0]
        if kind == "block":
            rc = mt.load_blocks(self.h, p, -1)
        elif kind == "blocks":
            rc = mt.load_blocks(self.h, p, len(mod[1]))
        elif kind == "chain":
            rc = mt.load_blocks(self.h, p, 0)
        elif kind == "stride2":
            rc = mt.load_stride2(self.h, p, int(mod[3]))
        elif kind == "upsample":
            rc = mt.load_upsample(self.h, p, int(mod[3]))
        elif kind == "subpel":
            rc = mt.load_subpel(self.h, p)
        else:
            rc = mt.load_fin(self.h, p)
        return _lib.check(rc)

    def hand(self):
        from dcvc_amd import _lib
        v = ctypes.c_int(-1)
        _lib.check(self.mt.scratch(self.h, None, None, None, ctypes.byref(v)))
        return v.value

    def close(self):
        if self.h:
            torch.cuda.synchronize()
            self.mt.destroy(self.h)
            self.h = None


def make_bufs(case):
    """name -> int16 [pixels + 1][ld], NaN-payload sentinels everywhere except the input views (N(0, 1) data)"""
    bufs = {}
    for name, (ld, _) in case["bufs"].items():
        bufs[name] = torch.full((M.pixels_of(case, name) + 1, ld), SENT, dtype=torch.int16)
    for buf, off, c in case["init"]:
        g = torch.Generator().manual_seed(M._seed("%s/%s/%d" % (case["name"], buf, off)))
        P = M.pixels_of(case, buf)
        bufs[buf][:P, off:off + c] = torch.randn((P, c), generator=g).half().view(torch.int16)
    return {k: v.cuda() for k, v in bufs.items()}


def clone(bufs):
    return {k: v.clone() for k, v in bufs.items()}


def half_view(case, bufs, view):
    buf, off, c = view
    return bufs[buf][:M.pixels_of(case, buf), off:off + c].contiguous().view(torch.half)


def _profile_begin(mt):
    U.call(mt.prof_reset)
    U.call(mt.prof_en, 1)


def _profile_end(mt):
    torch.cuda.synchronize()
    buf = np.zeros(64, dtype=REC)
    n = int(mt.prof_get(buf.ctypes.data, len(buf)))
    mt.prof_en(0)
    mt.prof_reset()
    return [int(v) & 0xFFFFFFFF for v in buf["variant"][:n]]


def run_module(mt, hd, case, bufs, qs, record=None, calls=None, sync=True):
    """the calls of `case` through the test surface; record: a list that receives the launch records of every call"""
    st = U.stream()

    def vw(view):
        if view is None:
            return (None, 0, 0)
        buf, off, c = view
        return (U.at(bufs[buf], off), bufs[buf].shape[1], c)

    def blk_of(ref):
        return (-1, 0) if ref is None else (hd.ids[ref[0]], ref[1])

    def fin_of(fn):
        if fn is None:
            return (-1, None, None, 0, 0)
        y, ld, _ = vw(fn["y"])
        return (hd.ids[fn["mod"]], U.ptr(qs.get(fn["q"])), y, ld, int(fn["keep"]))

    for call in (case["calls"] if calls is None else calls):
        op, m = call["op"], hd.ids[call["mod"]]
        H, W = M.call_in_grid(case, call)
        if record is not None:
            _profile_begin(mt)
        try:
            if op == "block":
                U.call(mt.block_forward, hd.h, m, call["i"], *vw(call["x"]), *vw(call["y"]), H, W, int(call["sc"]),
                       U.ptr(qs.get(call["qf"])), U.ptr(qs.get(call["qa"])), *vw(call["alt"]), *blk_of(call["next"]),
                       int(call["done"]), *fin_of(call["fin"]), st)
            elif op == "chain":
                qa = () if call["qa"] is None else (U.ptr(qs[call["qa"]]),)
                U.call(mt.chain_forward_qa if qa else mt.chain_forward, hd.h, m, call["first"], call["n"], *vw(call["x"]),
                       *vw(call["tmp"]), *vw(call["y"]), H, W, U.ptr(qs.get(call["qf"])), *qa, *vw(call["tmp2"]),
                       *fin_of(call["fin"]), *blk_of(call["after"]), int(call["done"]), st)
            elif op == "stride2":
                U.call(mt.stride2_forward, hd.h, m, *vw(call["x"]), *vw(call["tmp"]), *vw(call["y"]), H, W, st)
            elif op == "upsample":
                ut = call["up_tmp"]
                U.call(mt.upsample_forward, hd.h, m, *vw(call["x"]), *vw(call["tmp"]), *vw(call["y"]), H, W,
                       U.ptr(bufs[ut]) if ut else None, int(ut is not None), *blk_of(call["next"]), st)
            else:
                ut = call["up_tmp"]
                U.call(mt.subpel_forward, hd.h, m, *vw(call["x"]), *vw(call["y"]), H, W, U.ptr(bufs[ut]) if ut else None,
                       int(ut is not None), case["batch"], st)
        finally:
            if record is not None:
                record.append(_profile_end(mt))
    if sync:
        torch.cuda.synchronize()


def written(case):
    """the buffers some call may write"""
    out = set()
    for call in case["calls"]:
        for k in ("y", "tmp", "tmp2", "alt"):
            if call.get(k) is not None:
                out.add(call[k][0])
        if call.get("fin") is not None:
            out.add(call["fin"]["y"][0])
        if call.get("up_tmp"):
            out.add(call["up_tmp"])
    return out


def compare(case, got, want, start, what):
    for name in case["bufs"]:
        P = M.pixels_of(case, name)
        if name in case["temps"]:
            assert bool((got[name][P:] == SENT).all()), "%s: rows past the last pixel of %s were written" % (what, name)
            continue
        if not torch.equal(got[name], want[name]):
            d = torch.nonzero(got[name] != want[name])
            r, c = int(d[0][0]), int(d[0][1])
            where = "past the last pixel" if r >= P else "pixel %d channel %d" % (r, c)
            raise AssertionError("%s: buffer %s differs from the launch sequence in %d elements, first at %s (got 0x%04x, "
                                 "want 0x%04x)" % (what, name, d.shape[0], where, int(got[name][r, c]) & 0xFFFF,
                                                   int(want[name][r, c]) & 0xFFFF))
    for name in set(case["bufs"]) - written(case):
        assert torch.equal(got[name], start[name]), "%s: input buffer %s was written" % (what, name)


def outputs_finite(case, bufs):
    for call in case["calls"]:
        views = [call["y"]] + ([call["fin"]["y"]] if call.get("fin") else [])
        for v in views:
            assert bool(torch.isfinite(half_view(case, bufs, v)).all()), "%s: the reference output %r is not finite" % (case["name"], v)


def ids(cases):
    return [c["name"] for c in cases]


# ---------------------------------------------------------------------------------------------- prepared weights
def _read(mt, hd, module, index, what, count):
    a = np.zeros(count + 8, dtype=np.float16)
    n = int(mt.read(hd.h, module, index, what, a.ctypes.data, a.size))
    assert n == count, (n, count)
    return a[:count]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int16).ravel(), np.ascontiguousarray(b).view(np.int16).ravel())


@pytest.mark.parametrize("shape", sorted(M.SHAPES))
def test_prepared_block_weights(env, shape):
    """taps transposed to [9][cdc], the depthwise bias folded through dc.3 (fp32 chain, two fp16 roundings), and what load()
    decided, for every block shape"""
    mt, _ = env
    c, cdc, cffn, cin = M.SHAPES[shape]
    case = M.x_single(shape, 4, 4)
    hd = Handle(mt, case)
    try:
        m = hd.ids["B"]
        taps = _read(mt, hd, m, 0, 0, 9 * cdc)
        assert _same_bits(taps, M.prep_taps(hd.sd["B.dc.2.weight"])), "taps are not [9][cdc] of dc.2.weight"
        assert not _same_bits(taps, M.f16(hd.sd["B.dc.2.weight"])), "the taps' transpose cannot be told from the checkpoint layout"
        folded = _read(mt, hd, m, 0, 1, c)
        want = M.fold_bias(hd.sd["B.dc.3.weight"], hd.sd["B.dc.2.bias"], hd.sd["B.dc.3.bias"])
        assert _same_bits(folded, want), "folded dc.3 bias: %d of %d channels differ" % (int((folded != want).sum()), c)
        info = (ctypes.c_int * 8)()
        U.call(mt.block_info, hd.h, m, 0, 96, 256, -1, 0, info)
        assert list(info)[4:] == [c, cdc, cffn, cin]
        assert bool(info[0]) == M.is_nsplit(c, cdc, cffn)
        assert bool(info[1]) == bool(cin and M.is_nsplit(c, cdc, cffn) and M.B.pair_supported(cin, c, cdc))
        assert bool(info[2]) == ((not M.is_nsplit(c, cdc, cffn)) and not cin and M.tail_supported(96, 256, c, cdc, cffn))
        U.call(mt.block_info, hd.h, m, 0, 96, 240, m, 0, info)
        assert bool(info[2]) == ((not M.is_nsplit(c, cdc, cffn)) and not cin and M.tail_supported(96, 240, c, cdc, cffn))
        assert bool(info[3]) == (M.is_nsplit(c, cdc, cffn) and not cin)          # feeds(a block of its own shape)
    finally:
        hd.close()


def test_fold_hand_example(env):
    """the three-channel example of test_module_cases_cpu.py through DcbW::load itself"""
    mt, _ = env
    sd = {k: torch.from_numpy(v) for k, v in M.hand_example().items()}
    case = dict(M.x_single("l_128", 1, 1), mods={"B": ("block", "l_128")})
    hd = Handle(mt, case, elems=1024, sd=sd)
    try:
        got = _read(mt, hd, hd.ids["B"], 0, 1, 3)
        assert got.tolist() == M.HAND_FOLDED, got.tolist()
        taps = _read(mt, hd, hd.ids["B"], 0, 0, 27)
        assert _same_bits(taps, M.prep_taps(sd["B.dc.2.weight"]))
    finally:
        hd.close()


@pytest.mark.parametrize("kind", ["stride2", "subpel", "subpel-k1-bias", "subpel-k3-bias", "upsample"])
def test_prepared_layouts(env, kind):
    mt, _ = env
    mod = {"stride2": ("stride2", 24, "l_128", True), "subpel": ("subpel", 24, 128, 1, False),
           "subpel-k1-bias": ("subpel", 24, 16, 1, True), "subpel-k3-bias": ("subpel", 24, 16, 3, True),
           "upsample": ("upsample", 24, "l_128", True, 1, False)}[kind]
    case = dict(M.x_single("l_128", 1, 1), mods={"S": mod})
    hd = Handle(mt, case, elems=1024)
    try:
        if kind == "stride2":
            w = hd.sd["S.down.weight"]
            got, want = _read(mt, hd, hd.ids["S"], 0, 2, w.numel()), M.prep_stride2(w)
        else:
            w = hd.sd["S.up.conv.0.weight" if kind == "upsample" else "S.conv.0.weight"]
            got = _read(mt, hd, hd.ids["S"], 0, 3, w.numel())
            want = M.prep_convk(w) if mod[-1] else M.prep_subpel(w)
        assert _same_bits(got, want), kind
        if kind != "subpel-k1-bias":        # (kernel 1 with a bias: [4 cout][1][1][cin] IS the checkpoint layout)
            assert not _same_bits(got, M.f16(w)), "the re-layout cannot be told from the checkpoint layout"
    finally:
        hd.close()


# ---------------------------------------------------------------------------------------------- bit-exact: the launch sequence
@pytest.mark.parametrize("case", M.CASES, ids=ids(M.CASES))
def test_case_equals_launch_sequence(env, case):
    mt, ops = env
    hd = Handle(mt, case)
    try:
        qs = {k: v.cuda() for k, v in M.case_qs(case).items()}
        start = make_bufs(case)
        got, want = clone(start), clone(start)
        rec = []
        run_module(mt, hd, case, got, qs, record=rec)
        keep = M.run_reference(ops, U, case, hd.sd, want, qs)
        del keep
        outputs_finite(case, want)
        COVER[case["name"]] = [sorted(M.classify(v, call["op"] != "subpel", call.get("fin") is not None))
                               for v, call in zip(rec, case["calls"])]
        compare(case, got, want, start, case["name"])
        # ... and took the launches that modules.hip's rules, restated in module_cases.predict_call, pick for these views
        for i, call in enumerate(case["calls"]):
            assert set(COVER[case["name"]][i]) == M.predict_call(case, call), "%s call %d: launches %s, predicted %s" % (
                case["name"], i, COVER[case["name"]][i], sorted(M.predict_call(case, call)))
    finally:
        hd.close()


# ---------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize("case", M.F64_CASES, ids=ids(M.F64_CASES))
def test_float64(env, case):
    mt, _ = env
    hd = Handle(mt, case)
    try:
        qs = {k: v.cuda() for k, v in M.case_qs(case).items()}
        bufs = make_bufs(case)
        run_module(mt, hd, case, bufs, qs)
        call = case["calls"][0]
        sd = {k: v.cuda() for k, v in hd.sd.items()}
        Hi, Wi = M.call_in_grid(case, call)
        x = half_view(case, bufs, call["x"]).reshape(case["batch"], Hi, Wi, -1)
        ap = M.f64_call(R, case, sd, x, qs)
        got = half_view(case, bufs, call["y"])
        st = R.check(got, ap, case["name"], sharp_bias=True)
        # The interval is rigorous but wide behind several ambiguous fp16 intermediates (every radius enters the next
        # contraction with sum |w|). The norm is the sharp companion: at most five fp16 roundings per block (adaptor, dc.0,
        # depthwise, dc.3, chunk-add) and the output's own, 2^-11 relative each and passed on with gains of order one
        # (test_module_cases_cpu.py derives the same 2^-8 for one block); a chain of n blocks gets n times that.
        blocks = len(M.block_prefixes(case, call["mod"])) if call["op"] == "chain" else 1
        rel = float((got.double() - R.reference16(ap)).norm() / R.reference16(ap).norm())
        print("%-28s max %.2f ulp, exact %.4f, bias %+.3f, norm %.2e" % (case["name"], st["max_ulp"], st["exact"], st["bias"], rel))
        assert rel < blocks * 2.0 ** -8, "%s: relative distance to float64 %.3e" % (case["name"], rel)
    finally:
        hd.close()


# ---------------------------------------------------------------------------------------------- state
SMALL = [c for c in M.CASES if c["H"] * c["W"] <= 700]


@pytest.mark.parametrize("case", SMALL[::3], ids=ids(SMALL[::3]))
def test_same_call_twice(env, case):
    mt, _ = env
    hd = Handle(mt, case)
    try:
        qs = {k: v.cuda() for k, v in M.case_qs(case).items()}
        start = make_bufs(case)
        a, b = clone(start), clone(start)
        run_module(mt, hd, case, a, qs)
        run_module(mt, hd, case, b, qs)
        for name in case["bufs"]:
            if name not in case["temps"]:
                assert torch.equal(a[name], b[name]), "%s: buffer %s differs between two runs of the same handle" % (case["name"], name)
    finally:
        hd.close()


def _hand_left_set():
    """two (384, 192) blocks with a closing conv: ONE hand-over with the depthwise conv inside, so Scratch::hand stays 1"""
    c = M.ld_fusion(9, 17)
    c = dict(c, name="ld-fusion-two-blocks", calls=[dict(c["calls"][0], n=2)])
    return c


@pytest.mark.parametrize("second", ["ld_recon_head", "ld_adaptor_i_fe", "ld_hyper_enc"])
def test_chain_after_hand_flip(env, second):
    """a chain behind a DIFFERENT chain that left Scratch::hand set gives the bits of a fresh handle"""
    mt, ops = env
    first = _hand_left_set()
    case = {"ld_recon_head": M.ld_recon_head(9, 17), "ld_adaptor_i_fe": M.ld_adaptor_i_fe(9, 17),
            "ld_hyper_enc": M.ld_hyper_enc(18, 34)}[second]
    qs = {k: v.cuda() for k, v in M.case_qs(case).items()}
    start = make_bufs(case)
    fresh, used = clone(start), clone(start)
    hd = Handle(mt, case)
    try:
        run_module(mt, hd, case, fresh, qs)
    finally:
        hd.close()
    hd = Handle(mt, [first, case], elems=max(M.scratch_elems(first), M.scratch_elems(case)))
    try:
        fb = make_bufs(first)
        want = clone(fb)
        run_module(mt, hd, first, fb, {})
        assert hd.hand() == 1, "the first chain was meant to leave Scratch::hand set"
        M.run_reference(ops, U, first, hd.sd, want, {})
        compare(first, fb, want, want, first["name"])
        run_module(mt, hd, case, used, qs)
        for name in case["bufs"]:
            if name not in case["temps"]:
                assert torch.equal(fresh[name], used[name]), "%s behind a hand flip: buffer %s differs from a fresh handle" % (case["name"], name)
    finally:
        hd.close()


def _plane(ops, hd, which, rows, c):
    """rows x c halves of scratch plane t1 / t2 / t3, copied out by the library's strided copy"""
    from dcvc_amd import _lib
    p = (ctypes.c_void_p * 3)()
    _lib.check(hd.mt.scratch(hd.h, ctypes.byref(p, 0), ctypes.byref(p, 8), ctypes.byref(p, 16), None))
    out = torch.empty((rows, c), dtype=torch.int16, device="cuda")
    U.call(ops.replicate_pad, ctypes.c_void_p(p[which]), c, 1, rows, c, 0, 0, U.ptr(out), c, U.stream())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", ["dw_outside", "dw_inside"])
def test_handed_dc0_waits_in_the_plane_the_header_names(env, kind):
    """modules.h: with `next`, the following block's dc.0 output waits in s.t1 - or, behind a launch with its depthwise conv
    inside, in the plane Scratch::hand names (hand set: s.t2)"""
    mt, ops = env
    case = M.x_blk_encoder(9, 17) if kind == "dw_outside" else M.ld_fusion(9, 17)
    if kind == "dw_inside":
        case = dict(case, calls=[M.blk("F", M.V("PF", 384), M.V("PF", 384), i=0, nxt=("F", 1))])
    else:
        case = dict(case, calls=case["calls"][:1])
    nxt = case["calls"][0]["next"]
    hd = Handle(mt, case)
    try:
        qs = {k: v.cuda() for k, v in M.case_qs(case).items()}
        bufs = make_bufs(case)
        run_module(mt, hd, case, bufs, qs)
        assert hd.hand() == (1 if kind == "dw_inside" else 0)
        w = M.prep_block(hd.sd, M.block_prefixes(case, nxt[0])[nxt[1]])
        NP, y = 9 * 17, case["calls"][0]["y"]
        w1, b1 = torch.from_numpy(w["w1"].view(np.int16)).cuda(), torch.from_numpy(w["b1"].view(np.int16)).cuda()
        want = torch.empty((NP, w["cdc"]), dtype=torch.int16, device="cuda")
        U.call(ops.conv1x1, U.at(bufs[y[0]], y[1]), bufs[y[0]].shape[1], U.ptr(w1), U.ptr(b1), None, 0, None, 0, None, None,
               U.ptr(want), w["cdc"], NP, w["c"], w["cdc"], 1, U.stream())
        torch.cuda.synchronize()
        assert torch.equal(_plane(ops, hd, hd.hand(), NP, w["cdc"]), want), "the handed-over dc.0 is not where modules.h says"
    finally:
        hd.close()


GRAPH_CASES = [M.ld_fusion(9, 17), M.dmci_encoder(9, 17), M.ld_hyper_enc(18, 34), M.ht_decoder(5, 3, 3), M.ld_adaptor_i_fe(5, 3),
               M.dmci_decoder(5, 3, 2)]


@pytest.mark.parametrize("case", GRAPH_CASES, ids=ids(GRAPH_CASES))
def test_graph_replay_equals_eager(env, case):
    mt, _ = env
    hd = Handle(mt, case)
    try:
        qs = {k: v.cuda() for k, v in M.case_qs(case).items()}
        start = make_bufs(case)
        eager, replayed = clone(start), clone(start)
        run_module(mt, hd, case, eager, qs)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run_module(mt, hd, case, replayed, qs, sync=False)
        torch.cuda.synchronize()
        for name in case["bufs"]:
            assert torch.equal(replayed[name], start[name]), "capture ran the launches"
        g.replay()
        torch.cuda.synchronize()
        for name in case["bufs"]:
            if name not in case["temps"]:
                assert torch.equal(eager[name], replayed[name]), "%s: buffer %s differs between eager and replay" % (case["name"], name)
    finally:
        hd.close()


# ---------------------------------------------------------------------------------------------- refusals
def _refusal_case(batch=1):
    return M.case("refusals", "none", 4, 4,
                  {"A": ("block", "l_fai0"), "B": ("blocks", ["l_256", "l_256"]), "C": ("block", "i_512"), "F": ("fin", "l_dec2"),
                   "U": ("upsample", 128, "h_256", True, 1, True)},
                  {"X": (256, "g"), "X2": (192, "g"), "Y": (512, "g"), "T": (256, "g"), "O": (256, "g"), "UPT": (1024, "g"),
                   "D": (256, "d"), "D2": (256, "d")}, [M.V("X", 256), M.V("X2", 192)], [], batch=batch)


X, X2, Y, T, O = M.V("X", 256), M.V("X2", 192), M.V("Y", 256), M.V("T", 256), M.V("O", 256)
REFUSALS = [
    ("fin+next", M.blk("B", X, Y, i=0, nxt=("B", 1), fin=M.fin("F", O)), "a closing conv sits behind the LAST block"),
    ("fin-width", M.blk("C", M.V("Y", 512), M.V("Y", 512), fin=M.fin("F", O)), "a closing conv sits behind the LAST block"),
    ("next-unfed", M.blk("B", X, Y, i=0, nxt=("C", 0)), "dc.0 hand-over between blocks that do not support it"),
    ("done-adaptor", M.blk("A", X2, Y, done=True), "dc.0 hand-over between blocks that do not support it"),
    ("adaptor+shortcut", M.blk("A", X2, Y, sc=True), "DepthConvBlock with adaptor and shortcut"),
    ("shortcut-in-place", M.blk("B", X, X, i=0, sc=True), "DepthConvBlock with shortcut cannot run in place"),
    ("chain-after+fin", M.chn("B", X, T, Y, fin=M.fin("F", O), after=("B", 0)), "run_dcb_chain: the chain behind this one"),
    ("chain-after-unfed", M.chn("B", X, T, Y, after=("C", 0)), "run_dcb_chain: the chain behind this one"),
]


@pytest.mark.parametrize("what", [r[0] for r in REFUSALS] + ["scratch", "biased-batch", "biased-no-tmp"])
def test_refusals(env, what):
    from dcvc_amd import _lib
    mt, _ = env
    case = _refusal_case(2 if what == "biased-batch" else 1)
    if what == "scratch":
        call, msg, elems = M.blk("B", X, Y, i=0), "DepthConvBlock: scratch planes too small", 16 * 128 - 1
    elif what == "biased-batch":
        call, msg, elems = M.ups("U", M.V("X", 128), M.V("D2", 256), M.V("D", 256), up_tmp="UPT"), "takes one picture per launch", None
    elif what == "biased-no-tmp":
        call, msg, elems = M.ups("U", M.V("X", 128), M.V("D2", 256), M.V("D", 256)), "biased SubpelConv2x needs a temporary", None
    else:
        call, msg = [(r[1], r[2]) for r in REFUSALS if r[0] == what][0]
        elems = None
    hd = Handle(mt, case, elems=elems if elems is not None else 64 * 1024)
    try:
        start = make_bufs(case)
        bufs = clone(start)
        with pytest.raises(_lib.DcvcError) as e:
            run_module(mt, hd, case, bufs, {}, calls=[call])
        assert msg in str(e.value), str(e.value)
        torch.cuda.synchronize()
        for name in bufs:
            assert torch.equal(bufs[name], start[name]), "a refused call wrote %s" % name
    finally:
        hd.close()


# ---------------------------------------------------------------------------------------------- coverage of the dispatch
def test_zz_coverage_report():
    """the launch records of the cases above reached every branch of DcbW::forward that default mode can reach"""
    if not COVER:
        pytest.skip("no case of test_case_equals_launch_sequence ran in this session")
    reached = {}
    for name, calls in COVER.items():
        for i, br in enumerate(calls):
            for b in br:
                reached.setdefault(b, []).append("%s#%d" % (name, i))
    print("\nbranches of DcbW::forward reached by tests/module_cases.py (case#call):")
    for b in M.BRANCHES:
        hits = reached.get(b, [])
        print("  %-11s %3d calls, e.g. %s" % (b, len(hits), ", ".join(hits[:4])))
    for b, why in M.UNREACHABLE.items():
        print("  %-11s unreachable in default mode: %s" % (b, why))
    if len(COVER) == len(M.CASES):
        missing = [b for b in M.BRANCHES if b not in reached and b not in M.UNREACHABLE]
        assert not missing, "branches no case reached: %s" % missing
        # the flips: the same call site on both sides of each threshold took different branches
        def branches(name):
            return {b for call in COVER[name] for b in call}
        assert "nsplit32" in branches("dmci-encoder-99x128") and "nsplit64" in branches("dmci-encoder-100x128")
        assert "dw_inside" in branches("ld-fusion-99x128") and "dw_outside" in branches("ld-fusion-100x128")
        assert "plain" in branches("x-tail256-96x240") and {"tail", "tail+dc0"} <= branches("x-tail256-96x256")
        assert {"tail", "tail+dc0"} <= branches("x-tail256-89x241")
        assert "plain" in branches("x-ffn-96x240") and "ffn_fused" in branches("x-ffn-96x256")
        assert "plain" in branches("x-ffn-89x241")
