"""What the fused DepthConvBlock kernels are compiled for, the dispatch rules that pick an instantiation, and the case tables of
tests/test_block_f64_gpu.py. TEST INFRASTRUCTURE ONLY (a helper module, not a conftest): test_block_f64_cpu.py checks on the
CPU that the case tables reach every instantiation parsed from the sources; the GPU tests confirm it from the launch records.

An instantiation key is
  ("nsplit8", C, CI, PXT, NEXT, DW)    dcb_nsplit8_kernel.h launch8<C, CI, PXT, NEXT, DW>  (PXT = 2: 64-pixel workgroups)
  ("pair8", CIN, C, CI, PXT)           dcb_pair8_kernel.h launch_pair<CIN, C, CI, PXT>
  ("tail", C, DW, QUANT, DC0)          dcb_tail.hip launch<C / 128, DW, QUANT, DC0>
  ("ffn", C, RES2, QUANT)              ffn_fused.hip launch<C / 128, RES2, QUANT>"""
import glob
import os
import re

KDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dcvc_amd", "csrc", "kernels")
TABLE_BYTES = 256 * 16                  # WSILU_SEGMENTS float4 rows
LDS = 160 * 1024
WIDE_PIXELS = 64 * 200                  # nsplit_wide / dcb_pair: 64-pixel workgroups from here on


def _read(name):
    with open(os.path.join(KDIR, name)) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def _ints(s):
    return [int(v) for v in s.replace(" ", "").split(",") if v]


# ---------------------------------------------------------------------------------------------- instantiations in the sources
def nsplit8_instantiations():
    keys = set()
    for path in sorted(glob.glob(os.path.join(KDIR, "dcb_nsplit8_*.hip"))):
        src = _read(os.path.basename(path))
        for m in re.finditer(r"(extern\s+)?template\s+void\s+launch8<([\d,\s]+)>", src):
            if m.group(1):
                continue                                    # a declaration: instantiated in its _fin unit
            a = _ints(m.group(2))
            keys.add(("nsplit8", a[0], a[1], a[2], a[3], a[4] if len(a) > 4 else 0))
    return keys


def pair8_instantiations():
    keys = set()
    for path in sorted(glob.glob(os.path.join(KDIR, "dcb_pair8_*.hip"))):
        for m in re.finditer(r"run_pair<([\d,\s]+)>", _read(os.path.basename(path))):
            cin, c, ci = _ints(m.group(1))
            keys.add(("pair8", cin, c, ci, 1))
            if pair_lay_fits(cin, c, ci, 2):
                keys.add(("pair8", cin, c, ci, 2))
    return keys


def _variant_branches(src, fn):
    body = src[src.index("void launch_variant"):]
    body = body[:body.index("\n}\n")]
    return [[v == "true" for v in m.split(",")[1:]] for m in re.findall(r"launch<(NT2[^>]*)>", body.replace(" ", ""))]


def tail_instantiations():
    src = _read("dcb_tail.hip")
    nts = {int(v) for v in re.findall(r"launch_variant<(\d)>", src)}
    return {("tail", 128 * nt, dw, quant, dc0) for nt in nts for dw, quant, dc0 in _variant_branches(src, "launch_variant")}


def ffn_instantiations():
    src = _read("ffn_fused.hip")
    nts = {int(v) for v in re.findall(r"launch_variant<(\d)>", src)}
    return {("ffn", 128 * nt, res2, quant) for nt in nts for res2, quant in _variant_branches(src, "launch_variant")}


def all_instantiations():
    return nsplit8_instantiations() | pair8_instantiations() | tail_instantiations() | ffn_instantiations()


# Share of a chained output's elements that must equal reference16 of the chained midpoints. Derived on the CPU from the
# oracle chain (test_block_f64_cpu.py::test_oracle_chain_inside_bound prints it for every shape, NEXT kind and option at
# 96 pixels): the lowest shares were 0.835 (normal, the 768-wide blocks' next dc.0 - behind four chained fp16 roundings),
# 0.974 (wide) and 0.835 (near_overflow); the floors leave 0.06 to 0.09 for smaller and larger grids. The kernels are
# bit-identical to that chain, so a kernel below the floor computes something else.
EXACT_FLOOR = {"normal": 0.75, "wide": 0.90, "near_overflow": 0.75}


# ---------------------------------------------------------------------------------------------- LDS layouts, restated
def align16k(b):
    return (b + 16383) & ~16383


def nsplit8_rt(C, CI, PXT, NEXT=1):
    """Lay<C, CI, PXT, NEXT>::RT of dcb_nsplit8_kernel.h (NS8_TRIPLE = 1): interleaved copies of the WSiLU table"""
    CIP, CP = (CI + 127) // 128 * 128, (C + 127) // 128 * 128
    A, B = 32 * PXT * CIP * 2, 32 * PXT * CP * 2
    NB = NEXT if NEXT > 1 else CI
    consts = (2 * C + 4 * CI + NB) * 4 + 2 * C * 2
    fit4 = 2 * A + B + 4 * TABLE_BYTES + consts <= LDS and (2 * A + B) % 16384 == 0
    fit1 = 2 * A + B + TABLE_BYTES + consts <= LDS and (2 * A + B) % 4096 == 0
    return 4 if fit4 else 1 if fit1 else 4


def pair_lay_fits(CIN, C, CI, PXT):
    """Lay<CIN, C, CI, PXT>::FITS of dcb_pair8_kernel.h"""
    CINP, CP = (CIN + 127) // 128 * 128, (C + 127) // 128 * 128
    A, B = 32 * PXT * CINP * 2, 32 * PXT * CP * 2
    return align16k(A + B) + 4 * TABLE_BYTES + (CP + CI) * 4 <= LDS


# ---------------------------------------------------------------------------------------------- dispatch rules, restated
NSPLIT_SHAPES = [(192, 192), (256, 128), (256, 256), (384, 192), (384, 384), (512, 256), (512, 512), (768, 768)]
FINS = {(256, 128): (128, 192, 256), (256, 256): (192,), (512, 512): (256, 512), (768, 768): (768,), (384, 192): (384,)}
PAIR_SHAPES = [(448, 256, 128), (512, 256, 128), (192, 256, 128), (128, 256, 256), (512, 256, 256), (192, 384, 384),
               (384, 192, 192), (256, 512, 512), (512, 512, 512), (192, 512, 512), (192, 512, 256)]


def nsplit_wide(P, C):
    return P >= WIDE_PIXELS and C < 768


def dw_supported(C, CI, P):
    return (C, CI) == (256, 128) or ((C, CI) == (384, 192) and not nsplit_wide(P, C))


def fin_supported(C, CI, NN):
    return NN in FINS.get((C, CI), ())


def pair_supported(CIN, C, CI):
    return (CIN, C, CI) in PAIR_SHAPES


def predict(case):
    k = case["kind"]
    if k == "nsplit8":
        P = case["H"] * case["W"]
        pxt = 2 if nsplit_wide(P, case["C"]) else 1
        return ("nsplit8", case["C"], case["CI"], pxt, case["next"], 1 if case["dw"] else 0)
    if k == "pair8":
        P = case["P"]
        pxt = 2 if P >= WIDE_PIXELS and pair_lay_fits(case["CIN"], case["C"], case["CI"], 2) else 1
        return ("pair8", case["CIN"], case["C"], case["CI"], pxt)
    if k == "tail":
        return ("tail", case["C"], case["dw"] or case["dc0"], case["q"], case["dc0"])
    return ("ffn", case["C"], case["r2"], case["q"])


def variant_bits(key):
    """the launch record's variant word (ops.h) of an instantiation key"""
    if key[0] == "nsplit8":
        _, C, CI, pxt, nx, dw = key
        return 0x50000000 | CI | (nx << 12) | (dw << 24) | ((pxt == 2) << 25)
    if key[0] == "pair8":
        _, cin, C, CI, pxt = key
        return 0x60000000 | CI | (cin << 12) | ((pxt == 2) << 25)
    if key[0] == "tail":
        _, C, dw, quant, dc0 = key
        return 0x20000000 | C | (int(dw) << 24) | (int(quant) << 26) | (int(dc0) << 27)
    _, C, res2, quant = key
    return 0x30000000 | C | (int(quant) << 26) | (int(res2) << 27)


# ---------------------------------------------------------------------------------------------- case tables
def NS(C, CI, H, W, nxt=0, sc=False, q=False, q2=False, inplace=False, dw=False):
    return dict(kind="nsplit8", C=C, CI=CI, H=H, W=W, next=nxt, sc=sc, q=q, q2=q2, inplace=inplace, dw=dw)


def _nsplit_cases():
    cases = []
    for C, CI in NSPLIT_SHAPES:
        nexts = [0, 1] + list(FINS.get((C, CI), ()))
        i = 0
        for pxt in ((1, 2) if C < 768 else (1,)):
            for nx in nexts:
                opt = i % 4          # none, shortcut + q2, q, shortcut
                big = nx == 1        # one picture of 1080p size per shape and workgroup size: the NEXT = dc.0 case
                if pxt == 2:
                    H, W = (136, 240) if big else (1, 12801)
                else:
                    H, W = (68, 120) if big else (1, 45 + 2 * i) if i % 2 else (1, 100)
                cases.append(NS(C, CI, H, W, nx, sc=opt in (1, 3), q=opt == 2, q2=opt == 1, inplace=(i % 3 == 0 and opt not in (1, 3))))
                i += 1
    # depthwise inside: the DW_CASES geometries of test_kernels_gpu.py (one row, one column, tiles spanning rows, W < tile)
    geo = {(256, 128, 2): [(135, 240), (300, 50), (201, 65), (1000, 13), (135, 241)],
           (256, 128, 1): [(1, 40), (40, 1), (9, 7), (67, 121), (3, 3)],
           (384, 192, 1): [(68, 120), (400, 31), (1, 33)]}
    for (C, CI, pxt), hw in geo.items():
        for i, (nx, (H, W)) in enumerate(zip([0, 1] + list(FINS[(C, CI)]), hw)):
            opt = i % 4
            cases.append(NS(C, CI, H, W, nx, sc=opt in (1, 3), q=opt == 2, q2=opt == 1, dw=True))
    return cases


NSPLIT_CASES = _nsplit_cases()


def PR(CIN, C, CI, P):
    return dict(kind="pair8", CIN=CIN, C=C, CI=CI, P=P)


PAIR_CASES = [PR(cin, c, ci, 77 if i % 2 else 8160) for i, (cin, c, ci) in enumerate(PAIR_SHAPES)] + \
             [PR(cin, c, ci, 32640 if i == 0 else 12801) for i, (cin, c, ci) in enumerate(PAIR_SHAPES)
              if pair_lay_fits(cin, c, ci, 2)]


def TL(C, CD, CF, H, W, dw=True, q=False, dc0=False, sc=False, q2=False, n=1):
    return dict(kind="tail", C=C, CD=CD, CF=CF, H=H, W=W, dw=dw, q=q, dc0=dc0, sc=sc, q2=q2, n=n)


TAIL_CASES = [
    # C = 256 (half-width blocks: cdc = cffn = 128), the six launch_variant branches
    TL(256, 128, 128, 16, 32, dw=False),                   # 8 x 16 patches exactly
    TL(256, 128, 128, 13, 37, dw=False, q=True, q2=True),  # ragged patches
    TL(256, 128, 128, 24, 48, sc=True),
    TL(256, 128, 128, 1, 1, q=True),                       # one pixel: every tap outside the picture
    TL(256, 128, 128, 4, 4, dc0=True, sc=True, q2=True),
    TL(256, 128, 128, 13, 37, dc0=True, q=True),
    # C = 128 (full-width hyper-network blocks and the narrow half-width ones)
    TL(128, 64, 64, 4, 4, dw=False, sc=True),
    TL(128, 128, 128, 16, 32, dw=False, q=True),
    TL(128, 64, 64, 13, 37, q2=True),
    TL(128, 128, 128, 17, 30, q=True, q2=True),
    TL(128, 128, 128, 1, 1, dc0=True),
    TL(128, 64, 64, 24, 40, dc0=True, q=True, q2=True),
    # batched: n pictures with odd H, checked per picture against the single-picture reference
    TL(256, 128, 128, 9, 20, dc0=True, n=3),
    TL(128, 128, 128, 7, 17, n=2, sc=True),
    TL(256, 128, 128, 5, 16, q=True, n=2),
]


def FF(C, CF, P, r2=False, q=False, q2=False, inplace=False):
    return dict(kind="ffn", C=C, CF=CF, P=P, r2=r2, q=q, q2=q2, inplace=inplace)


FFN_CASES = [FF(C, CF, P, r2, q, q2=(i % 2 == 1), inplace=(i % 3 == 0))
             for C, CF, P in ((128, 64, 130), (256, 128, 1000), (384, 384, 300))
             for i, (r2, q) in enumerate(((False, False), (True, False), (False, True), (True, True)))]

ALL_CASES = NSPLIT_CASES + PAIR_CASES + TAIL_CASES + FFN_CASES


def name(c):
    k = c["kind"]
    opts = "".join(s for s, f in (("-sc", "sc"), ("-q", "q"), ("-q2", "q2"), ("-r2", "r2"), ("-inpl", "inplace"),
                                  ("-dc0", "dc0")) if c.get(f))
    if k == "nsplit8":
        nx = {0: "none", 1: "dc0"}.get(c["next"], "fin%d" % c["next"])
        return "nsplit8-%d-%d-%dx%d-%s%s%s" % (c["C"], c["CI"], c["H"], c["W"], nx, "-dw" if c["dw"] else "", opts)
    if k == "pair8":
        return "pair8-%d-%d-%d-P%d" % (c["CIN"], c["C"], c["CI"], c["P"])
    if k == "tail":
        return "tail-%d-%d-%d-n%dx%dx%d%s%s" % (c["C"], c["CD"], c["CF"], c["n"], c["H"], c["W"], "-dw" if c["dw"] else "", opts)
    return "ffn-%d-%d-P%d%s" % (c["C"], c["CF"], c["P"], opts)


def key_name(key):
    return "%s<%s>" % (key[0], ", ".join(str(int(v)) for v in key[1:]))


# ---------------------------------------------------------------------------------------------- operands
def _fit(R, ap, w, b, target):
    return R.fit_overflow(w, b, ap.t.abs().amax(0), target)


def block_operands(dist, seed, P, C, CI, CF=None, entry="t2", geom=None, nxt=0, sc=False, q=False, q2=False, qf=False,
                   dev="cpu"):
    """operands of one DepthConvBlock behind dc.0 (f64_ref.DISTS). entry: "t2" (the depthwise output is given), "t1" (the
    depthwise conv runs inside: taps, geom = (n, H, W)) or "x" (dc.0 inside as well: w1, b1). nxt: 0, 1 (w1n, b1n) or the
    width of a closing conv (wf, bf [, qf]). near_overflow: every stage's weights and bias are fitted against the float64 value
    of that stage, the earlier stages already fitted (chunk-add stages to 6e3: four of them sum to ~2.4e4; dc.3 and ffn.2 to
    1.5e4 each, so that y1 + ffn.2 + x stays below 3.1e4 and its q, q2 in [0.5, 1.2] below fp16's range)."""
    import torch
    import f64_ref as R
    CF = CF or CI
    big = dist == "near_overflow"
    g = torch.Generator().manual_seed(seed)

    def I(k, xshape, N):
        return R.inputs(dist, xshape, N, seed * 16 + k, dev)

    def qs(n):
        return (torch.randn((n,), generator=g) * 0.25 + 1).clamp(0.5, 1.2 if big else 1.5).half().to(dev)
    x = I(0, (P, C), 1)[0]
    ent, w3, b3 = I(1, (P, CI), C)
    _, w0, b0 = I(2, (P, C), 4 * CF)
    _, w2, b2 = I(3, (P, CF), C)
    op = dict(x=x, w3=w3, b3=b3, w0=w0, b0=b0, w2=w2, b2=b2, sc=sc, q=qs(C) if q else None, q2=qs(C) if q2 else None)
    if entry == "x":
        _, op["w1"], op["b1"] = I(4, (P, C), CI)
    else:
        op[entry] = ent
    if entry != "t2":
        op["taps"] = (torch.randn((9, CI), generator=g) * 0.3).half().to(dev)
        op["geom"] = geom
    if nxt == 1:
        _, op["w1n"], op["b1n"] = I(5, (P, C), CI)
    elif nxt:
        _, op["wfin"], op["bfin"] = I(5, (P, C), nxt)
        op["qfin"] = qs(nxt) if qf else None
    if big:
        if entry == "x":
            op["w1"], op["b1"] = _fit(R, R.conv1x1(x, op["w1"], op["b1"]), op["w1"], op["b1"], 4e3)
            t1 = R.Mid.of(R.conv1x1(x, op["w1"], op["b1"], wsilu=True))
        elif entry == "t1":
            t1 = R.Mid.exact(op["t1"])
        t2 = R.Mid.of(R.dwconv3x3(t1, op["taps"], *geom)) if entry != "t2" else R.Mid.exact(op["t2"])
        op["w3"], op["b3"] = _fit(R, R.conv1x1(t2, w3, b3), w3, b3, 1.5e4)
        y1 = R.Mid.of(R.conv1x1(t2, op["w3"], op["b3"], r1=x))
        op["w0"], op["b0"] = _fit(R, R.conv1x1(y1, w0, b0), w0, b0, 6e3)
        t = R.Mid.of(R.conv1x1(y1, op["w0"], op["b0"], wsilu=True, chunk_add=True))
        op["w2"], op["b2"] = _fit(R, R.conv1x1(t, w2, b2), w2, b2, 1.5e4)
        if nxt:
            y = R.Mid.of(R.conv1x1(t, op["w2"], op["b2"], r1=y1, r2=x if sc else None, q=op["q"], q2=op["q2"]))
            wk, bk = ("w1n", "b1n") if nxt == 1 else ("wfin", "bfin")
            op[wk], op[bk] = _fit(R, R.conv1x1(y, op[wk], op[bk]), op[wk], op[bk], 2e4)
    return op


def block_ref(R, op, band=1 << 15):
    return R.dcb(op["x"], op["w3"], op["b3"], op["w0"], op["b0"], op["w2"], op["b2"], t2=op.get("t2"), t1=op.get("t1"),
                 taps=op.get("taps"), geom=op.get("geom"), w1=op.get("w1"), b1=op.get("b1"), shortcut=op["sc"], q=op["q"],
                 q2=op["q2"], w1n=op.get("w1n"), b1n=op.get("b1n"), wfin=op.get("wfin"), bfin=op.get("bfin"),
                 qfin=op.get("qfin"), band=band)


def pair_operands(dist, seed, P, CIN, C, CI, dev="cpu"):
    import f64_ref as R
    x, wa, ba = R.inputs(dist, (P, CIN), C, seed * 16, dev)
    _, w1, b1 = R.inputs(dist, (P, C), CI, seed * 16 + 1, dev)
    if dist == "near_overflow":
        wa, ba = _fit(R, R.conv1x1(x, wa, ba), wa, ba, 2e4)
        w1, b1 = _fit(R, R.conv1x1(R.Mid.of(R.conv1x1(x, wa, ba)), w1, b1), w1, b1, 2e4)
    return dict(x=x, wa=wa, ba=ba, w1=w1, b1=b1)


def ffn_operands(dist, seed, P, C, CF, r2=False, q=False, q2=False, dev="cpu"):
    import torch
    import f64_ref as R
    big = dist == "near_overflow"
    g = torch.Generator().manual_seed(seed)
    x, w0, b0 = R.inputs(dist, (P, C), 4 * CF, seed * 16, dev)
    _, w2, b2 = R.inputs(dist, (P, CF), C, seed * 16 + 1, dev)
    if big:
        w0, b0 = _fit(R, R.conv1x1(x, w0, b0), w0, b0, 6e3)
        w2, b2 = _fit(R, R.conv1x1(R.Mid.of(R.conv1x1(x, w0, b0, wsilu=True, chunk_add=True)), w2, b2), w2, b2, 2e4)

    def qs(n):
        return (torch.randn((n,), generator=g) * 0.25 + 1).clamp(0.5, 1.2 if big else 1.5).half().to(dev)
    rr = (torch.randn((P, C), generator=g) * (100.0 if big else 1.0)).half().to(dev) if r2 else None
    return dict(x=x, w0=w0, b0=b0, w2=w2, b2=b2, r2=rr, q=qs(C) if q else None, q2=qs(C) if q2 else None)
