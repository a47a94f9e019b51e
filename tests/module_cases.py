"""Case table and references of tests/test_modules_gpu.py: the module layer (dcvc_amd/csrc/codec/modules.{h,hip}) against plain
launch sequences. TEST INFRASTRUCTURE ONLY (a helper module, not a conftest); test_module_cases_cpu.py checks the table itself.

A case is a small program over named buffers: the modules it loads (synthetic checkpoint-layout weights of the block shapes the
three codecs load), the buffers with their row widths, the views that hold input data, and the calls - each one a call of
DcbW::forward, run_dcb_chain / DcbChain::forward, Stride2W::forward, UpsampleW::forward or SubpelW::forward with every argument
spelled out as (buffer, channel offset, channels) views. Three interpreters run it:

  * the module layer itself, through include/dcvc_amd_modtest.h (test_modules_gpu.py);
  * `run_reference`: the PLAIN launch sequence - adaptor, dc.0 + WSiLU, depthwise, dc.3 + residual, ffn.0 + WSiLU + chunk-add,
    ffn.2 + residuals [* q], closing conv; conv_kxk / tconv2x2 / conv + shuffle2 in front - through the per-kernel C ABI
    (gpu_util.Ops) on weights prepared HERE in numpy, every intermediate in a private dense buffer. Every fused kernel claims
    the bits of that sequence (test_block_f64_gpu.py holds the kernels to it), so the module layer must give them too,
    whichever kernels and planes it picks: a wrong plane or a wrong prepared weight shows as different bits;
  * `f64_call`: the float64 value of a single call from the checkpoint-layout tensors (f64_ref, chained through `Mid`).

The folded bias in float64. DcbW::load replaces dc.3's bias by b' = fp16(fp16(a32) + b3) with a32 the fp32 fmaf chain of
a = sum_c W3[n][c] b2[c] (the depthwise bias pushed through dc.3). The float64 reference uses s = a + b3 exactly and allows
for the difference, rounding by rounding:
    fp32 chain     |a32 - a| <= K 2^-24 A with A = sum_c |W3[n][c] b2[c]|  (every product of two fp16 values is exact in
                   fp32; each of the K additions rounds a partial sum of magnitude <= A (1 + K 2^-24), the 2^-48 terms are
                   covered by taking K + 1 for K)
    first fp16     |fp16(a32) - a32| <= ulp16(|a| + K 2^-24 A) / 2
    fp32 sum       t + b3 of two fp16 values: one fp32 rounding, <= 2^-24 |t + b3|
    second fp16    <= ulp16(|t + b3| (1 + 2^-24)) / 2
so |b' - s| <= e_fold = (K + 1) 2^-24 A + u1 / 2 + 2^-24 S + u2 / 2, with u1 = ulp16(|a| + (K + 1) 2^-24 A),
S = |s| + (K + 1) 2^-24 A + u1 / 2 and u2 = ulp16(S (1 + 2^-24)). e_fold is added to the contraction bound of dc.3 before its
residual; nothing in it is fitted to what the GPU returns.
"""
import numpy as np

import block_cases as B

# ---------------------------------------------------------------------------------------------- dispatch rules, restated
PATCH_H, PATCH_W = 8, 16            # dcb_tail.hip PH x PW
TAIL_PATCHES = 192                  # dcb_tail_supported: 256-wide blocks from here on (128-wide ones always)
FFN_PIXELS = 128 * 192              # ffn_fused_supported
WIDE_PIXELS = B.WIDE_PIXELS         # nsplit_wide


def patches(H, W):
    return ((H + PATCH_H - 1) // PATCH_H) * ((W + PATCH_W - 1) // PATCH_W)


def is_nsplit(c, cdc, cffn):
    """dcb_nsplit_supported in default mode (DCVC_NSPLIT unset = 2)"""
    return cdc == cffn and (c, cdc) in B.NSPLIT_SHAPES


def tail_supported(H, W, c, cdc, cffn):
    ok = c in (128, 256) and cdc % 64 == 0 and 64 <= cdc <= 128 and cffn % 64 == 0 and cffn >= 64
    return ok and (patches(H, W) >= TAIL_PATCHES or c <= 128)


def ffn_fused_supported(P, c, cffn):
    return c in (128, 256, 384) and cffn % 64 == 0 and cffn >= 64 and P >= FFN_PIXELS and c <= 256


def dw_inside(c, cdc, P, batch):
    return batch == 1 and B.dw_supported(c, cdc, P)


# ---------------------------------------------------------------------------------------------- block shapes
# name -> (c, cdc, cffn, adaptor cin or 0). From the kCh* constants of dmci.h / dmc_ld.h / dmc_ht.h and the load() calls of the
# three codecs (dcvc_amd/arch.py lists the same checkpoints): LD's blocks and HT-S's picture-resolution blocks are half width.
SHAPES = {
    # dmci.hip (kChSrc 192, kChEncDec 384, kChY 256, kChZ 128)
    "i_enc1": (384, 384, 384, 192),         # enc.enc_1
    "i_384": (384, 384, 384, 0),            # enc.enc_2.*, dec.dec_1.*
    "i_henc0": (128, 128, 128, 256),        # hyper_enc.conv.0
    "i_128": (128, 128, 128, 0),            # hyper_enc.conv.1/2.conv, hyper_dec.conv.0/1.conv
    "i_hdec2": (256, 256, 256, 128),        # hyper_dec.conv.2
    "i_fus0": (512, 512, 512, 256),         # y_prior_fusion.conv.0
    "i_512": (512, 512, 512, 0),            # y_prior_fusion.conv.1/2, y_spatial_prior.conv.*, HT: the same and recon_head.conv1.*
    "i_spad": (512, 512, 512, 512),         # y_spatial_prior_adaptor_* (DMCI and HT)
    "i_dec2": (192, 192, 192, 384),         # dec.dec_2
    # dmc_ld.hip (kChSrc 192, kChY 128, kChZ 128, kChD 256, kChM 256)
    "l_fai0": (256, 128, 128, 192),         # feature_adaptor_i.conv.0
    "l_fam0": (256, 128, 128, 512),         # feature_adaptor_m.conv.0, y_spatial_prior.conv.0, decoder.conv1.0
    "l_enc0": (256, 128, 128, 448),         # encoder.conv1.0
    "l_256": (256, 128, 128, 0),            # every other block at picture resolution, temporal_prior_encoder.conv.conv
    "l_128": (128, 64, 64, 0),              # the hyper networks
    "l_fus": (384, 192, 192, 0),            # y_prior_fusion.conv.*
    # dmc_ht.hip (kChSrcI 192, kChY 256, kChZ 128, kChD 512, kChM 512, kChRecon 256)
    "h_fai0": (512, 256, 256, 192),         # HT-S feature_adaptor_i.conv.0
    "h_fam0": (512, 256, 256, 1024),        # HT-S feature_adaptor_m.conv.0, decoder.conv1.0
    "h_512h": (512, 256, 256, 0),           # HT-S half-width blocks
    "h_enc0": (512, 256, 256, 2048),        # HT-S encoder.conv1.0
    "h_256": (256, 256, 256, 0),            # hyper networks, recon heads
    "h_rh0": (256, 256, 256, 512),          # recon_head.conv2.*.0 / recon_head.conv.*.0
    "h_768": (768, 768, 768, 0),            # y_prior_fusion.conv.*
    "hl_fai0": (512, 512, 512, 192),        # HT-L feature_adaptor_i.conv.0
    # no model loads these: the branches of DcbW::forward that the model shapes do not reach in default mode
    "x_tail256": (256, 128, 64, 0),         # cdc != cffn: not an N-split block, so dcb_tail decides by the 192-patch rule
    "x_ffn": (256, 256, 128, 0),            # neither N-split nor dcb_tail: dc.0, depthwise, dc.3, then ffn_fused from 128*192 pixels
    "x_ffn_ad": (256, 256, 128, 192),
}
# closing convs (cin, cout): y_prior_fusion.conv.3, y_spatial_prior.conv.2/3, decoder.conv2, recon_head.head / .3 / .5
FINS = {"i_fus3": (512, 512), "l_fus3": (384, 384), "l_sp2": (256, 128), "l_dec2": (256, 256), "l_head": (256, 192),
        "h_fus3": (768, 768), "h_sp3s": (512, 256), "h_head": (256, 192), "x_fin": (256, 64)}


# ---------------------------------------------------------------------------------------------- synthetic weights
def _seed(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7FFFFFF


def _conv(sd, name, cin, cout, gain=1.0, bias=True):
    """f64_ref.inputs' scaling: w ~ N(0, 1 / cin), bias ~ N(0, 0.25); gain is a power of two (exact in fp16)"""
    import f64_ref as R
    _, w, b = R.inputs("normal", (1, cin), cout, _seed(name))
    sd[name + ".weight"] = (w * gain).reshape(cout, cin, 1, 1).contiguous()
    if bias:
        sd[name + ".bias"] = b * gain


def block_weights(sd, prefix, shape):
    """checkpoint-layout tensors of one DepthConvBlock (layers.py DepthConvBlock: adaptor, dc.0, dc.2, dc.3, ffn.0, ffn.2). The
    residual branches are halved so that a chain of five blocks stays far inside fp16; the depthwise bias is of order one so
    that the fold through dc.3 matters in every output channel."""
    import torch
    c, cdc, cffn, cin = shape
    if cin:
        _conv(sd, prefix + "adaptor", cin, c)
    _conv(sd, prefix + "dc.0", c, cdc)
    g = torch.Generator().manual_seed(_seed(prefix + "dc.2"))
    sd[prefix + "dc.2.weight"] = (torch.randn((cdc, 1, 3, 3), generator=g) * 0.3).half()
    sd[prefix + "dc.2.bias"] = (torch.randn((cdc,), generator=g) * 0.5).half()
    _conv(sd, prefix + "dc.3", cdc, c, 0.5)
    _conv(sd, prefix + "ffn.0", c, 4 * cffn)
    _conv(sd, prefix + "ffn.2", cffn, c, 0.5)


def module_weights(sd, prefix, mod):
    """mod: ("block", shape) | ("blocks" | "chain", [shapes]) | ("stride2", cin, shape, shortcut) |
    ("upsample", cin, shape, shortcut, k, bias) | ("subpel", cin, cout, k, bias) | ("fin", fin)"""
    import torch
    kind = mod[0]
    if kind == "block":
        block_weights(sd, prefix, SHAPES[mod[1]])
    elif kind in ("blocks", "chain"):
        for i, s in enumerate(mod[1]):
            block_weights(sd, prefix + "%d." % i, SHAPES[s])
    elif kind == "stride2":
        c = SHAPES[mod[2]][0]
        _conv(sd, prefix + "down", 4 * mod[1], c)
        block_weights(sd, prefix + "conv.", SHAPES[mod[2]])
    elif kind in ("upsample", "subpel"):
        cin, cout = (mod[1], SHAPES[mod[2]][0]) if kind == "upsample" else (mod[1], mod[2])
        k, bias = mod[-2], mod[-1]
        p = prefix + ("up." if kind == "upsample" else "")
        g = torch.Generator().manual_seed(_seed(p + "conv.0"))
        sd[p + "conv.0.weight"] = (torch.randn((4 * cout, cin, k, k), generator=g) / float(np.sqrt(cin * k * k))).half()
        if bias:
            sd[p + "conv.0.bias"] = (torch.randn((4 * cout,), generator=g) * 0.5).half()
        if kind == "upsample":
            block_weights(sd, prefix + "conv.", SHAPES[mod[2]])
    elif kind == "fin":
        cin, cout = FINS[mod[1]]
        _conv(sd, prefix[:-1], cin, cout)
    else:
        raise ValueError(kind)


def case_weights(case):
    sd = {}
    for name, mod in case["mods"].items():
        module_weights(sd, name + ".", mod)
    return sd


def case_qs(case):
    import torch
    out = {}
    for name, n in case["qs"].items():
        g = torch.Generator().manual_seed(_seed(case["name"] + name))
        out[name] = (torch.randn((n,), generator=g) * 0.25 + 1).clamp(0.5, 1.5).half()
    return out


# ---------------------------------------------------------------------------------------------- weight preparation in numpy
def f16(t):
    return np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float16)


def prep_taps(dc2_weight):
    """[cdc][1][3][3] -> tap major [9][cdc]"""
    w = f16(dc2_weight)
    return np.ascontiguousarray(w.reshape(w.shape[0], 9).T)


def fold_bias(w3, b2, b3):
    """fp16( fp16( sum_c W3[n][c] b2[c] ) + b3[n] ), the sum as an fp32 fmaf chain over c. A product of two fp16 values is
    exact in fp32, so fmaf(w, b, acc) = fp32(w b + acc) = one fp32 addition of the exact product."""
    w = f16(w3).reshape(f16(w3).shape[0], -1).astype(np.float32)
    b = f16(b2).astype(np.float32)
    acc = np.zeros(w.shape[0], dtype=np.float32)
    for ch in range(w.shape[1]):
        acc = (acc + w[:, ch] * b[ch]).astype(np.float32)
    t = acc.astype(np.float16)
    return (t.astype(np.float32) + f16(b3).astype(np.float32)).astype(np.float16)


def hand_example():
    """a three-channel block (numpy fp16, checkpoint layout, prefix "B.") whose fold can be done by hand, b2 = (1, 1/2, 2):
      row 0: W3 = (1, 2^-10, 0), b3 = 2^-11: a = 1 + 2^-11 -> fp16 (tie, to even) 1; 1 + 2^-11 -> fp16 1. One rounding of the
             exact sum 1 + 2^-10 would have kept it: the two roundings show
      row 1: W3 = (1, 2^-10, 2^-12), b3 = 0: a = 1 + 2^-11 + 2^-11 = 1 + 2^-10, representable
      row 2: W3 = (3, -6, 1/4), b3 = 1/4: a = 3 - 3 + 1/2, + 1/4 = 3/4"""
    h = np.float16
    sd = {"B.dc.0.weight": np.eye(3, dtype=h).reshape(3, 3, 1, 1), "B.dc.0.bias": np.zeros(3, h),
          "B.dc.2.weight": (np.arange(27, dtype=np.float32) / 16).astype(h).reshape(3, 1, 3, 3), "B.dc.2.bias": np.array([1, 0.5, 2], h),
          "B.dc.3.weight": np.array([[1, 2.0 ** -10, 0], [1, 2.0 ** -10, 2.0 ** -12], [3, -6, 0.25]], h).reshape(3, 3, 1, 1),
          "B.dc.3.bias": np.array([2.0 ** -11, 0, 0.25], h),
          "B.ffn.0.weight": np.ones((12, 3, 1, 1), h), "B.ffn.0.bias": np.zeros(12, h),
          "B.ffn.2.weight": np.eye(3, dtype=h).reshape(3, 3, 1, 1), "B.ffn.2.bias": np.zeros(3, h)}
    return sd


HAND_FOLDED = [1.0, 1.0009765625, 0.75]


def prep_stride2(w):
    """down.weight [cout][4 cin][1][1], input channel = c * 4 + dy * 2 + dx -> [cout][2][2][cin]"""
    w = f16(w)
    cout, cin = w.shape[0], w.shape[1] // 4
    return np.ascontiguousarray(w.reshape(cout, cin, 4).transpose(0, 2, 1))


def prep_subpel(w):
    """up.conv.0.weight without a bias [4 cout][cin][1][1], row = co * 4 + dy * 2 + dx -> [4][cout][cin]"""
    w = f16(w)
    cout, cin = w.shape[0] // 4, w.shape[1]
    return np.ascontiguousarray(w.reshape(cout, 4, cin).transpose(1, 0, 2))


def prep_convk(w):
    """[cout][cin][k][k] -> tap major [cout][k][k][cin]"""
    return np.ascontiguousarray(f16(w).transpose(0, 2, 3, 1))


def prep_block(sd, p):
    """the operands of one block's launch sequence"""
    two = lambda t: f16(t).reshape(t.shape[0], -1)
    out = dict(w1=two(sd[p + "dc.0.weight"]), b1=f16(sd[p + "dc.0.bias"]), taps=prep_taps(sd[p + "dc.2.weight"]),
               w3=two(sd[p + "dc.3.weight"]), b3=fold_bias(sd[p + "dc.3.weight"], sd[p + "dc.2.bias"], sd[p + "dc.3.bias"]),
               w0=two(sd[p + "ffn.0.weight"]), b0=f16(sd[p + "ffn.0.bias"]),
               w2=two(sd[p + "ffn.2.weight"]), b2=f16(sd[p + "ffn.2.bias"]))
    if p + "adaptor.weight" in sd:
        out["wa"], out["ba"] = two(sd[p + "adaptor.weight"]), f16(sd[p + "adaptor.bias"])
    out["c"], out["cdc"] = out["w1"].shape[1], out["w1"].shape[0]
    out["cffn"] = out["w0"].shape[0] // 4
    return out


def block_prefixes(case, mod):
    """checkpoint prefixes of the blocks of module `mod`, in block_forward's index order"""
    m = case["mods"][mod]
    if m[0] == "block":
        return [mod + "."]
    if m[0] in ("blocks", "chain"):
        return [mod + ".%d." % i for i in range(len(m[1]))]
    if m[0] in ("stride2", "upsample"):
        return [mod + ".conv."]
    return []


def block_shapes(case, mod):
    m = case["mods"][mod]
    if m[0] == "block":
        return [SHAPES[m[1]]]
    if m[0] in ("blocks", "chain"):
        return [SHAPES[s] for s in m[1]]
    if m[0] in ("stride2", "upsample"):
        return [SHAPES[m[2]]]
    return []


# ---------------------------------------------------------------------------------------------- the case table
def V(buf, c, off=0):
    return (buf, off, c)


def blk(mod, x, y, i=0, sc=False, qf=None, qa=None, alt=None, nxt=None, done=False, fin=None):
    return dict(op="block", mod=mod, i=i, x=x, y=y, sc=sc, qf=qf, qa=qa, alt=alt, next=nxt, done=done, fin=fin)


def chn(mod, x, tmp, y, first=0, n=0, qf=None, qa=None, tmp2=None, fin=None, after=None, done=False):
    """qf / qa: ChainCall::q_fused_last / q_after_last, the scales of the LAST block"""
    return dict(op="chain", mod=mod, first=first, n=n, x=x, tmp=tmp, y=y, qf=qf, qa=qa, tmp2=tmp2, fin=fin, after=after, done=done)


def s2(mod, x, tmp, y):
    return dict(op="stride2", mod=mod, x=x, tmp=tmp, y=y)


def ups(mod, x, tmp, y, up_tmp=None, nxt=None):
    return dict(op="upsample", mod=mod, x=x, tmp=tmp, y=y, up_tmp=up_tmp, next=nxt)


def sub(mod, x, y, up_tmp=None):
    return dict(op="subpel", mod=mod, x=x, y=y, up_tmp=up_tmp)


def fin(mod, y, q=None, keep=False):
    """FinCall: the closing conv `mod` writes the view y (its buffer's row width is ldy)"""
    return dict(mod=mod, y=y, q=q, keep=keep)


def case(name, site, H, W, mods, bufs, init, calls, temps=(), qs=None, batch=1, f64=False):
    """bufs: name -> (row width, grid) with grid "g" = H x W, "h" = H/2 x W/2, "d" = 2H x 2W (all times batch);
    init: the views that hold input data; temps: buffers whose contents the module layer does not define (a temporary the
    call may or may not use, a block output that is not stored) - everything else must equal the launch sequence, whole."""
    return dict(name="%s-%dx%d%s" % (name, H, W, "-n%d" % batch if batch > 1 else ""), site=site, H=H, W=W, batch=batch,
                mods=mods, bufs=bufs, init=list(init), calls=list(calls), temps=tuple(temps), qs=qs or {}, f64=f64)


def grid_of(case, g):
    H, W = case["H"], case["W"]
    return {"g": (H, W), "h": (H // 2, W // 2), "d": (2 * H, 2 * W)}[g]


def pixels_of(case, buf):
    h, w = grid_of(case, case["bufs"][buf][1])
    return case["batch"] * h * w


def scratch_elems(case):
    """what a codec would allocate: the widest inner tensor of any block on its grid (one plane also takes the adaptor /
    conv output of the one-launch blocks: c halves per pixel)"""
    need = 1
    for call in case["calls"]:
        if call["op"] == "subpel":
            continue
        h, w = call_grid(case, call)
        for c, cdc, cffn, _ in block_shapes(case, call["mod"]):
            need = max(need, case["batch"] * h * w * max(c, cdc, cffn))
    return need


# ---- dmci.hip ----------------------------------------------------------------------------------------------------------
def dmci_encoder(H, W, batch=1):
    # dmci.hip run_encoder: enc_1 as a one-block chain (adaptor block, q_after_last, after) into the in-place chain of enc_2
    # with first_dc0_done
    return case("dmci-encoder", "dmci.hip run_encoder", H, W,
                {"E1": ("block", "i_enc1"), "E2": ("blocks", ["i_384", "i_384"])},
                {"U": (192, "g"), "F": (384, "g")}, [V("U", 192)],
                [chn("E1", V("U", 192), V("F", 384), V("F", 384), qa="q", after=("E2", 0)),
                 chn("E2", V("F", 384), V("F", 384), V("F", 384), done=True)], qs={"q": 384}, batch=batch)


def dmci_hyper_enc(H, W, batch=1, f64=False):
    # dmci.hip run_hyper_and_priors_enc: hyper_enc.conv.0 (adaptor, distinct output), then Stride2W with a distinct tmp and
    # the block shortcut
    return case("dmci-hyper-enc", "dmci.hip run_hyper_and_priors_enc", H, W,
                {"H0": ("block", "i_henc0"), "S1": ("stride2", 128, "i_128", True)},
                {"Y": (256, "g"), "Z1": (128, "g"), "Z2a": (128, "h"), "Z2": (128, "h")}, [V("Y", 256)],
                [blk("H0", V("Y", 256), V("Z1", 128)), s2("S1", V("Z1", 128), V("Z2a", 128), V("Z2", 128))],
                temps=("Z2a",), batch=batch)


def dmci_hyper_dec(H, W, batch=1):
    # dmci.hip run_priors_from_zhat: UpsampleW with a distinct tmp and the shortcut, then hyper_dec.conv.2 (adaptor block)
    return case("dmci-hyper-dec", "dmci.hip run_priors_from_zhat (hyper_dec)", H, W,
                {"U0": ("upsample", 128, "i_128", True, 1, False), "H2": ("block", "i_hdec2")},
                {"ZH": (128, "g"), "H1a": (128, "d"), "H1": (128, "d"), "HP": (256, "d")}, [V("ZH", 128)],
                [ups("U0", V("ZH", 128), V("H1a", 128), V("H1", 128)), dict(blk("H2", V("H1", 128), V("HP", 256)), grid="d")],
                temps=("H1a",), batch=batch)


def dmci_fusion(H, W, batch=1, keep=False):
    # dmci.hip run_priors_from_zhat: y_prior_fusion as ONE chain - adaptor block into a distinct buffer, two blocks in place,
    # the closing conv behind the last one (the block's own output is not stored unless keep_block_output)
    return case("dmci-fusion" + ("-keep" if keep else ""), "dmci.hip run_priors_from_zhat (y_prior_fusion)", H, W,
                {"F": ("blocks", ["i_fus0", "i_512", "i_512"]), "F3": ("fin", "i_fus3")},
                {"HP": (256, "g"), "PF": (512, "g"), "PAR": (512, "g")}, [V("HP", 256)],
                [chn("F", V("HP", 256), V("PF", 512), V("PF", 512), fin=fin("F3", V("PAR", 512), keep=keep))],
                temps=() if keep else ("PF",), batch=batch)


def dmci_spatial_prior(H, W, batch=1):
    # dmci.hip run_spatial_prior: y_spatial_prior_adaptor_k as a one-block chain (adaptor of its own width, after) and the
    # in-place chain with first_dc0_done that ends in y_spatial_prior.conv.3
    return case("dmci-spatial-prior", "dmci.hip run_spatial_prior", H, W,
                {"A": ("block", "i_spad"), "S": ("blocks", ["i_512", "i_512"]), "S3": ("fin", "i_fus3")},
                {"CAT": (512, "g"), "AD": (512, "g"), "SP": (512, "g")}, [V("CAT", 512)],
                [chn("A", V("CAT", 512), V("AD", 512), V("AD", 512), after=("S", 0)),
                 chn("S", V("AD", 512), V("AD", 512), V("AD", 512), done=True, fin=fin("S3", V("SP", 512)))],
                temps=("AD",), batch=batch)


def dmci_decoder(H, W, batch=1):
    # dmci.hip run_decoder: UpsampleW with next, the in-place chain with first_dc0_done and q_after_last, dec_2 (192-wide
    # adaptor block)
    return case("dmci-decoder", "dmci.hip run_decoder", H, W,
                {"U": ("upsample", 256, "i_384", True, 1, False), "D": ("blocks", ["i_384", "i_384"]), "D2": ("block", "i_dec2")},
                {"YH": (256, "g"), "D0": (384, "d"), "D1": (384, "d"), "R": (192, "d")}, [V("YH", 256)],
                [ups("U", V("YH", 256), V("D0", 384), V("D1", 384), nxt=("D", 0)),
                 dict(chn("D", V("D1", 384), V("D1", 384), V("D1", 384), qa="q", done=True), grid="d"),
                 dict(blk("D2", V("D1", 384), V("R", 192)), grid="d")],
                temps=("D0",), qs={"q": 384}, batch=batch)


# ---- dmc_ld.hip --------------------------------------------------------------------------------------------------------
def ld_adaptor_i_fe(H, W):
    # dmc_ld.hip run_fa_i + run_fe: a four-block chain with the tmp / tmp2 ping-pong into a slice of a wider row, `after` = the
    # extractor's first block; then the extractor with first_dc0_done, its output at a channel offset of another wide row
    return case("ld-fa_i-fe", "dmc_ld.hip run_fa_i, run_fe", H, W,
                {"A": ("blocks", ["l_fai0", "l_256", "l_256", "l_256"]), "E": ("blocks", ["l_256"] * 5)},
                {"FI": (192, "g"), "CATM": (512, "g"), "CATD": (512, "g"), "T": (256, "g"), "T2": (256, "g")}, [V("FI", 192)],
                [chn("A", V("FI", 192), V("T", 256), V("CATM", 256), tmp2=V("T2", 256), after=("E", 0)),
                 chn("E", V("CATM", 256), V("T", 256), V("CATD", 256, 256), tmp2=V("T2", 256), done=True)],
                temps=("T", "T2"))


def ld_adaptor_m(H, W):
    # dmc_ld.hip run_fa_m: x.p == y.p with different widths (View(m_CATM, ld, 512) into View(m_CATM, ld, 256)), ping-pong,
    # `after`; the extractor's first block then runs on the handed-over dc.0
    return case("ld-fa_m", "dmc_ld.hip run_fa_m", H, W,
                {"A": ("blocks", ["l_fam0", "l_256", "l_256", "l_256"]), "E": ("blocks", ["l_256"])},
                {"CATM": (512, "g"), "T": (256, "g"), "T2": (256, "g"), "O": (256, "g")}, [V("CATM", 512)],
                [chn("A", V("CATM", 512), V("T", 256), V("CATM", 256), tmp2=V("T2", 256), after=("E", 0)),
                 chn("E", V("CATM", 256), V("T", 256), V("O", 256), tmp2=V("T2", 256), done=True)],
                temps=("T", "T2"))


def ld_adaptor_in_place(H, W):
    # dmc_ld.hip run_fa_m's views with ONE block: the adaptor's output is the block output and starts where x starts, so the
    # adaptor + dc.0 pair launch must not be taken (its workgroups would write rows that others still read)
    return case("ld-fa_m-one-block", "dmc_ld.hip run_fa_m", H, W, {"A": ("blocks", ["l_fam0", "l_256"])},
                {"CATM": (512, "g"), "T": (256, "g")}, [V("CATM", 512)],
                [chn("A", V("CATM", 512), V("T", 256), V("CATM", 256), n=1)], temps=("T",))


def ld_tpe(H, W):
    # dmc_ld.hip run_tpe: Stride2W without the shortcut, tmp == y, from a slice of a wider row
    return case("ld-tpe", "dmc_ld.hip run_tpe", H, W, {"S": ("stride2", 256, "l_256", False)},
                {"CATM": (512, "g"), "TP": (256, "h")}, [V("CATM", 256)],
                [s2("S", V("CATM", 256), V("TP", 256), V("TP", 256))])


def ld_encoder(H, W):
    # dmc_ld.hip run_encoder: a chain whose x sits at a channel offset inside a concatenation (m_CATD + 64), tmp == y,
    # ping-pong, q_fused_last
    return case("ld-encoder", "dmc_ld.hip run_encoder", H, W, {"E": ("blocks", ["l_enc0", "l_256", "l_256"])},
                {"CATD": (512, "g"), "T": (256, "g"), "T2": (256, "g")}, [V("CATD", 448, 64)],
                [chn("E", V("CATD", 448, 64), V("T", 256), V("T", 256), qf="q", tmp2=V("T2", 256))],
                temps=("T2",), qs={"q": 256})


def ld_hyper_enc(H, W, f64=False):
    # dmc_ld.hip run_hyper_encoder: the 128-wide half-width block (one launch, input != output), then Stride2W without the
    # shortcut and tmp == y: the one-launch block cannot run in place, the conv's output is redirected to s.t3
    return case("ld-hyper-enc", "dmc_ld.hip run_hyper_encoder", H, W,
                {"H0": ("block", "l_128"), "S1": ("stride2", 128, "l_128", False)},
                {"Y": (128, "g"), "Z1": (128, "g"), "Z2": (128, "h")}, [V("Y", 128)],
                [blk("H0", V("Y", 128), V("Z1", 128)), s2("S1", V("Z1", 128), V("Z2", 128), V("Z2", 128))])


def ld_hyper_dec(H, W):
    # dmc_ld.hip run_priors: UpsampleW without the shortcut and tmp == y (redirected to s.t3), then hyper_decoder.conv.2
    return case("ld-hyper-dec", "dmc_ld.hip run_priors (hyper_decoder)", H, W,
                {"U0": ("upsample", 128, "l_128", False, 1, False), "H2": ("block", "l_128")},
                {"ZH": (128, "g"), "H1": (128, "d"), "HP": (128, "d")}, [V("ZH", 128)],
                [ups("U0", V("ZH", 128), V("H1", 128), V("H1", 128)), dict(blk("H2", V("H1", 128), V("HP", 128)), grid="d")])


def ld_fusion(H, W, keep=False):
    # dmc_ld.hip run_priors: x = tmp = y, the (384, 192) blocks hand dc.0 over with the depthwise conv inside (s.hand flips),
    # and the closing conv writes a 384-wide slice of a 512-wide row whose first 128 channels hold y_hat
    return case("ld-fusion" + ("-keep" if keep else ""), "dmc_ld.hip run_priors (y_prior_fusion)", H, W,
                {"F": ("blocks", ["l_fus"] * 3), "F3": ("fin", "l_fus3")},
                {"PF": (384, "g"), "CATSP": (512, "g")}, [V("PF", 384), V("CATSP", 128)],
                [chn("F", V("PF", 384), V("PF", 384), V("PF", 384), fin=fin("F3", V("CATSP", 384, 128), keep=keep))],
                temps=() if keep else ("PF",))


def ld_spatial_prior(H, W):
    # dmc_ld.hip run_spatial_prior: adaptor block on the whole 512-wide row, tmp == y, y_spatial_prior.conv.2 closes the chain
    return case("ld-spatial-prior", "dmc_ld.hip run_spatial_prior", H, W,
                {"S": ("blocks", ["l_fam0", "l_256"]), "S2": ("fin", "l_sp2")},
                {"CATSP": (512, "g"), "T": (256, "g"), "M": (128, "g")}, [V("CATSP", 512)],
                [chn("S", V("CATSP", 512), V("T", 256), V("T", 256), fin=fin("S2", V("M", 128)))], temps=("T",))


def ld_decoder(H, W):
    # dmc_ld.hip run_decoder: SubpelW (no bias) between slices of two wide rows, then the chain with ping-pong and
    # decoder.conv2 as closing conv WITH q into the second half of the adaptor_m input
    return case("ld-decoder", "dmc_ld.hip run_decoder", H, W,
                {"U": ("subpel", 128, 256, 1, False), "D": ("blocks", ["l_fam0", "l_256", "l_256"]), "D2": ("fin", "l_dec2")},
                {"CATSP": (512, "g"), "CATD": (512, "d"), "T": (256, "d"), "T2": (256, "d"), "CATM": (512, "d")},
                [V("CATSP", 128), V("CATD", 256, 256), V("CATM", 256)],
                [sub("U", V("CATSP", 128), V("CATD", 256)),
                 dict(chn("D", V("CATD", 512), V("T", 256), V("T", 256), tmp2=V("T2", 256),
                          fin=fin("D2", V("CATM", 256, 256), q="q")), grid="d")],
                temps=("T", "T2"), qs={"q": 256})


def ld_recon_head(H, W):
    # dmc_ld.hip run_recon_head: x at a channel offset (m_CATM + kChM), tmp == y, ping-pong, recon_head.head closes the chain
    return case("ld-recon-head", "dmc_ld.hip run_recon_head", H, W,
                {"R": ("blocks", ["l_256"] * 3), "RH": ("fin", "l_head")},
                {"CATM": (512, "g"), "T": (256, "g"), "T2": (256, "g"), "FI": (192, "g")}, [V("CATM", 256, 256)],
                [chn("R", V("CATM", 256, 256), V("T", 256), V("T", 256), tmp2=V("T2", 256), fin=fin("RH", V("FI", 192)))],
                temps=("T", "T2"))


# ---- dmc_ht.hip --------------------------------------------------------------------------------------------------------
def ht_adaptor_i(H, W, large=False):
    # dmc_ht.hip run_fa_i: DcbChain::forward without a second temporary (in place behind the first block), into a slice
    return case("ht%s-fa_i" % ("l" if large else "s"), "dmc_ht.hip run_fa_i", H, W,
                {"A": ("chain", ["hl_fai0", "i_512", "i_512"] if large else ["h_fai0", "h_512h", "h_512h", "h_512h"])},
                {"FI": (192, "g"), "T": (512, "g"), "CATM": (1024, "g")}, [V("FI", 192)],
                [chn("A", V("FI", 192), V("T", 512), V("CATM", 512))], temps=("T",))


def ht_adaptor_m_fe(H, W):
    # dmc_ht.hip run_fa_m + run_fe: x.p == y.p with different widths and no second temporary; then the extractor from that
    # slice to a channel offset of another wide row
    return case("hts-fa_m-fe", "dmc_ht.hip run_fa_m, run_fe", H, W,
                {"A": ("chain", ["h_fam0", "h_512h"]), "E": ("chain", ["h_512h", "h_512h"])},
                {"CATM": (1024, "g"), "T": (512, "g"), "CATE": (1024, "g")}, [V("CATM", 1024)],
                [chn("A", V("CATM", 1024), V("T", 512), V("CATM", 512)),
                 chn("E", V("CATM", 512), V("T", 512), V("CATE", 512, 512))], temps=("T",))


def ht_tpe(H, W, shortcut):
    # dmc_ht.hip run_tpe: Stride2W into a slice at a channel offset (m_CATPF + kChY): with the shortcut through a distinct tmp,
    # without it tmp == y
    tmp = V("AD", 512) if shortcut else V("CATPF", 512, 256)
    return case("ht-tpe-%s" % ("sc" if shortcut else "nosc"), "dmc_ht.hip run_tpe", H, W,
                {"S": ("stride2", 512, "i_512", shortcut)},
                {"TI": (512, "g"), "AD": (512, "h"), "CATPF": (768, "h")}, [V("TI", 512)],
                [s2("S", V("TI", 512), tmp, V("CATPF", 512, 256))], temps=("AD",))


def ht_encoder(H, W):
    # dmc_ht.hip run_encoder: DcbChain::forward(x, t, t, q_fused_last) on the 2048-wide concatenation, tmp == y, no tmp2
    return case("hts-encoder", "dmc_ht.hip run_encoder", H, W, {"E": ("chain", ["h_enc0", "h_512h", "h_512h"])},
                {"CATE": (2048, "g"), "T": (512, "g")}, [V("CATE", 2048)],
                [chn("E", V("CATE", 2048), V("T", 512), V("T", 512), qf="q")], qs={"q": 512})


def ht_hyper_enc(H, W):
    # dmc_ht.hip run_hyper_encoder: a full-width block without adaptor into a distinct output, Stride2W 256 -> 128 with a
    # distinct tmp (the two halves of one allocation in the codec)
    return case("ht-hyper-enc", "dmc_ht.hip run_hyper_encoder", H, W,
                {"H0": ("block", "h_256"), "S2": ("stride2", 256, "i_128", True)},
                {"Y": (256, "g"), "Z1": (256, "g"), "Z3a": (128, "h"), "Z3": (128, "h")}, [V("Y", 256)],
                [blk("H0", V("Y", 256), V("Z1", 256)), s2("S2", V("Z1", 256), V("Z3a", 128), V("Z3", 128))], temps=("Z3a",))


def ht_hyper_dec(H, W, shortcut=True):
    # dmc_ht.hip run_common (HT-L): the BIASED up-sampler with kernel 1 (conv1x1 + shuffle2 through up_tmp, zeros passed), then
    # hyper_decoder.conv.2
    tmp = V("H1a", 256) if shortcut else V("H1", 256)
    return case("htl-hyper-dec-%s" % ("sc" if shortcut else "nosc"), "dmc_ht.hip run_common (hyper_decoder)", H, W,
                {"U0": ("upsample", 128, "h_256", shortcut, 1, True), "H2": ("block", "h_256")},
                {"ZH": (128, "g"), "UPT": (1024, "g"), "H1a": (256, "d"), "H1": (256, "d"), "HP": (256, "d")}, [V("ZH", 128)],
                [ups("U0", V("ZH", 128), tmp, V("H1", 256), up_tmp="UPT"), dict(blk("H2", V("H1", 256), V("HP", 256)), grid="d")],
                temps=("UPT", "H1a"))


def ht_fusion(H, W):
    # dmc_ht.hip run_common: DcbChain::forward(pf, pf, pf, fin) on the 768-wide blocks
    return case("ht-fusion", "dmc_ht.hip run_common (y_prior_fusion)", H, W,
                {"F": ("chain", ["h_768"] * 3), "F3": ("fin", "h_fus3")},
                {"PF": (768, "g"), "COMMON": (768, "g")}, [V("PF", 768)],
                [chn("F", V("PF", 768), V("PF", 768), V("PF", 768), fin=fin("F3", V("COMMON", 768)))], temps=("PF",))


def ht_spatial_prior(H, W):
    # dmc_ht.hip run_spatial_prior: the adaptor block WITHOUT next, then DcbChain::forward(ad, ad, ad, fin) computing its own
    # dc.0; HT-S's y_spatial_prior.conv.3 is 512 -> 256
    return case("hts-spatial-prior", "dmc_ht.hip run_spatial_prior", H, W,
                {"A": ("block", "i_spad"), "S": ("chain", ["i_512"] * 3), "S3": ("fin", "h_sp3s")},
                {"CATSP": (512, "g"), "AD": (512, "g"), "SP": (256, "g")}, [V("CATSP", 512)],
                [blk("A", V("CATSP", 512), V("AD", 512)),
                 chn("S", V("AD", 512), V("AD", 512), V("AD", 512), fin=fin("S3", V("SP", 256)))], temps=("AD",))


def ht_decoder(H, W, k):
    # dmc_ht.hip run_decoder: SubpelW from a slice into [up out | ctx] of the 2048-wide row - HT-L: biased, kernel 3, through
    # up_tmp with zeros; HT-S: no bias - then decoder.conv1 from that 1024-wide view into a slice, q_fused_last, no tmp2
    return case("ht%s-decoder" % ("l" if k == 3 else "s"), "dmc_ht.hip run_decoder", H, W,
                {"U": ("subpel", 256, 512, k, k == 3), "D": ("chain", ["h_fam0", "h_512h"])},
                {"CATSP": (512, "g"), "UPT": (2048, "g"), "CATE": (2048, "d"), "T": (512, "d"), "CATM": (1024, "d")},
                [V("CATSP", 256), V("CATE", 512, 1536)],
                [sub("U", V("CATSP", 256), V("CATE", 512, 1024), up_tmp="UPT" if k == 3 else None),
                 dict(chn("D", V("CATE", 1024, 1024), V("T", 512), V("CATM", 512, 512), qf="q"), grid="d")],
                temps=("UPT", "T"), qs={"q": 512})


def ht_recon_head(H, W):
    # dmc_ht.hip run_head (one picture of run_recon_head; the reset path): recon_head.conv1.j (full-width block from a slice into a dense buffer), then
    # the head chain (adaptor 512 -> 256) with tmp == y and the 192-wide closing conv
    return case("hts-recon-head", "dmc_ht.hip run_head", H, W,
                {"C": ("block", "i_512"), "R": ("chain", ["h_rh0", "h_256", "h_256"]), "RH": ("fin", "h_head")},
                {"CATM": (1024, "g"), "RC": (512, "g"), "RT": (256, "g"), "FI": (192, "g")}, [V("CATM", 512, 512)],
                [blk("C", V("CATM", 512, 512), V("RC", 512)),
                 chn("R", V("RC", 512), V("RT", 256), V("RT", 256), fin=fin("RH", V("FI", 192)))], temps=("RT",))


# ---- the branches no model shape reaches in default mode ----------------------------------------------------------------
def x_tail256(H, W):
    # no call site: a (256, 128, 64) block (not an N-split shape) - dcb_tail with dc.0 inside when input != output, without
    # when in place, from 192 patches on; below, the plain four launches. A closing conv behind it, q_fused and q_after
    return case("x-tail256", "none: DcbW::forward, 256-wide dcb_tail", H, W,
                {"B": ("blocks", ["x_tail256", "x_tail256"]), "FN": ("fin", "x_fin")},
                {"X": (256, "g"), "Y": (256, "g"), "O": (64, "g")}, [V("X", 256)],
                [chn("B", V("X", 256), V("Y", 256), V("Y", 256), qf="q", fin=fin("FN", V("O", 64), q="q2")),
                 blk("B", V("X", 256), V("Y", 256), i=1, sc=True, qa="q")], qs={"q": 256, "q2": 64})


def x_ffn(H, W):
    # no call site: a (256, 256, 128) block (neither N-split nor dcb_tail) - ffn_fused from 128 * 192 pixels on, the plain
    # four launches below; with an adaptor (alt given / not given), with the shortcut, in place
    return case("x-ffn", "none: DcbW::forward, ffn_fused and the plain launches", H, W,
                {"A": ("block", "x_ffn_ad"), "B": ("block", "x_ffn")},
                {"X": (192, "g"), "Y": (256, "g"), "ALT": (256, "g"), "Z": (256, "g"), "Y2": (256, "g")}, [V("X", 192)],
                [blk("A", V("X", 192), V("Y", 256), alt=V("ALT", 256)),
                 blk("B", V("Y", 256), V("Z", 256), sc=True, qa="q"),
                 blk("B", V("Z", 256), V("Z", 256), qf="q"),
                 blk("A", V("X", 192), V("Y2", 256))], temps=("ALT",), qs={"q": 256})


def x_blk_encoder(H, W, batch=1):
    # no call site: the encoder's sequence as DcbW::forward calls - an adaptor block with q_after and next, then blocks in
    # place that are handed their dc.0 (dc0_done) and hand the next one over
    return case("x-blk-encoder", "none: DcbW::forward, q_after with next and the block-level hand-over", H, W,
                {"E1": ("block", "i_enc1"), "E2": ("blocks", ["i_384", "i_384"])},
                {"U": (192, "g"), "F": (384, "g")}, [V("U", 192)],
                [blk("E1", V("U", 192), V("F", 384), qa="q", nxt=("E2", 0)),
                 blk("E2", V("F", 384), V("F", 384), i=0, nxt=("E2", 1), done=True),
                 blk("E2", V("F", 384), V("F", 384), i=1, done=True)], qs={"q": 384}, batch=batch)


def x_blk_fusion(H, W, batch=1, keep=False):
    # no call site: the fusion sequence as DcbW::forward calls - the last block with fin, with and without keep_block_output
    return case("x-blk-fusion" + ("-keep" if keep else ""), "none: DcbW::forward, fin with keep_block_output", H, W,
                {"F": ("blocks", ["i_fus0", "i_512", "i_512"]), "F3": ("fin", "i_fus3")},
                {"HP": (256, "g"), "PF": (512, "g"), "PAR": (512, "g")}, [V("HP", 256)],
                [blk("F", V("HP", 256), V("PF", 512), i=0, nxt=("F", 1)),
                 blk("F", V("PF", 512), V("PF", 512), i=1, nxt=("F", 2), done=True),
                 blk("F", V("PF", 512), V("PF", 512), i=2, done=True, fin=fin("F3", V("PAR", 512), keep=keep))],
                temps=() if keep else ("PF",), batch=batch)


def x_blk_spatial_prior(H, W, batch=1):
    # no call site: the spatial prior's sequence as DcbW::forward calls - an adaptor of the block's own width with next, blocks
    # in place, fin behind a block that was handed its dc.0
    return case("x-blk-spatial-prior", "none: DcbW::forward, hand-over into a block with fin", H, W,
                {"A": ("block", "i_spad"), "S": ("blocks", ["i_512", "i_512"]), "S3": ("fin", "i_fus3")},
                {"CAT": (512, "g"), "AD": (512, "g"), "SP": (512, "g")}, [V("CAT", 512)],
                [blk("A", V("CAT", 512), V("AD", 512), nxt=("S", 0)),
                 blk("S", V("AD", 512), V("AD", 512), i=0, nxt=("S", 1), done=True),
                 blk("S", V("AD", 512), V("AD", 512), i=1, done=True, fin=fin("S3", V("SP", 512)))],
                temps=("AD",), batch=batch)


def x_blk_decoder(H, W, batch=1):
    # no call site: the decoder's sequence as DcbW::forward calls - UpsampleW with next, blocks in place with the hand-over,
    # q_after on a block that was handed its dc.0
    return case("x-blk-decoder", "none: UpsampleW::forward with next, DcbW::forward with q_after and dc0_done", H, W,
                {"U": ("upsample", 256, "i_384", True, 1, False), "D": ("blocks", ["i_384", "i_384"]), "D2": ("block", "i_dec2")},
                {"YH": (256, "g"), "D0": (384, "d"), "D1": (384, "d"), "R": (192, "d")}, [V("YH", 256)],
                [ups("U", V("YH", 256), V("D0", 384), V("D1", 384), nxt=("D", 0)),
                 dict(blk("D", V("D1", 384), V("D1", 384), i=0, nxt=("D", 1), done=True), grid="d"),
                 dict(blk("D", V("D1", 384), V("D1", 384), i=1, qa="q", done=True), grid="d"),
                 dict(blk("D2", V("D1", 384), V("R", 192)), grid="d")],
                temps=("D0",), qs={"q": 384}, batch=batch)


def x_single(shape, H, W, sc=False, batch=1):
    # no single call site: one block of a model shape on its own, input != output - the float64 cases
    c, _, _, cin = SHAPES[shape]
    return case("single-%s%s" % (shape, "-sc" if sc else ""), "none: one DcbW::forward", H, W, {"B": ("block", shape)},
                {"X": (cin or c, "g"), "Y": (c, "g")}, [V("X", cin or c)],
                [blk("B", V("X", cin or c), V("Y", c), sc=sc, qf=None if sc else "q", qa="q2")], qs={"q": c, "q2": c}, batch=batch,
                f64=True)      # (the launch sequence has no fused scale behind two residuals: conv1x1 refuses it, no codec asks)


def x_chain(shapes, H, W, tag):
    # no single call site: a short chain on its own with a second temporary - the float64 cases
    c, cin = SHAPES[shapes[-1]][0], SHAPES[shapes[0]][3] or SHAPES[shapes[0]][0]
    return case("chain-%s" % tag, "none: one run_dcb_chain", H, W, {"C": ("blocks", list(shapes))},
                {"X": (cin, "g"), "T": (c, "g"), "T2": (c, "g"), "Y": (c, "g")}, [V("X", cin)],
                [chn("C", V("X", cin), V("T", c), V("Y", c), qf="q", tmp2=V("T2", c))], temps=("T", "T2"), qs={"q": c}, f64=True)


def x_stride2(shape, cin, H, W, shortcut):
    c = SHAPES[shape][0]
    tmp = V("T", c) if shortcut else V("Y", c)
    return case("stride2-%s-%s" % (shape, "sc" if shortcut else "nosc"), "none: one Stride2W::forward", H, W,
                {"S": ("stride2", cin, shape, shortcut)}, {"X": (cin, "g"), "T": (c, "h"), "Y": (c, "h")}, [V("X", cin)],
                [s2("S", V("X", cin), tmp, V("Y", c))], temps=("T",), f64=True)


def x_upsample(shape, cin, H, W, shortcut):
    c = SHAPES[shape][0]
    tmp = V("T", c) if shortcut else V("Y", c)
    return case("upsample-%s-%s" % (shape, "sc" if shortcut else "nosc"), "none: one UpsampleW::forward", H, W,
                {"U": ("upsample", cin, shape, shortcut, 1, False)}, {"X": (cin, "g"), "T": (c, "d"), "Y": (c, "d")},
                [V("X", cin)], [ups("U", V("X", cin), tmp, V("Y", c))], temps=("T",), f64=True)


# The grids: either side of nsplit_wide (99 x 128 / 100 x 128 = 12 672 / 12 800 pixels), either side of 192 patches and of
# 128 * 192 pixels (96 x 240 = 180 patches / 96 x 256 = 192 patches and 24 576 pixels), 192 ragged patches below 128 * 192 pixels
# (89 x 241), partial patches and tiles both ways (9 x 17, 5 x 3), one pixel. Stride-2 inputs are even-sided; a grid named for
# a module that up-samples is the INPUT grid, chosen so that the block's grid is the one meant.
def _cases():
    cs = []
    # --- N-split blocks either side of the 64-pixel workgroups
    for hw in ((99, 128), (100, 128)):
        cs += [dmci_encoder(*hw), dmci_fusion(*hw), ld_fusion(*hw), ld_adaptor_i_fe(*hw), ht_fusion(*hw), ld_recon_head(*hw)]
    cs += [dmci_decoder(50, 64), dmci_decoder(33, 96)]            # block grids 100 x 128 and 66 x 192 = 12 672 pixels
    # --- dcb_tail / ffn_fused either side of their flips, and the ragged grid
    for hw in ((96, 240), (96, 256), (89, 241), (9, 17), (1, 1)):
        cs += [x_tail256(*hw), x_ffn(*hw)]
    # --- every call site at the ragged small grids; batches for the intra patterns
    for hw in ((9, 17), (5, 3)):
        cs += [dmci_encoder(*hw), dmci_hyper_dec(*hw), dmci_fusion(*hw), dmci_fusion(*hw, keep=True), dmci_spatial_prior(*hw),
               dmci_decoder(*hw), ld_adaptor_i_fe(*hw), ld_adaptor_m(*hw), ld_encoder(*hw), ld_hyper_dec(*hw), ld_fusion(*hw),
               ld_fusion(*hw, keep=True), ld_spatial_prior(*hw), ld_decoder(*hw), ld_recon_head(*hw), ht_adaptor_i(*hw),
               ht_adaptor_i(*hw, large=True), ht_adaptor_m_fe(*hw), ht_encoder(*hw), ht_hyper_dec(*hw, True),
               ht_hyper_dec(*hw, False), ht_fusion(*hw), ht_spatial_prior(*hw), ht_decoder(*hw, 1), ht_decoder(*hw, 3),
               ht_recon_head(*hw)]
    for hw in ((18, 34), (10, 6)):                                # stride-2 inputs: block grids 9 x 17 and 5 x 3
        cs += [dmci_hyper_enc(*hw), ld_tpe(*hw), ld_hyper_enc(*hw), ht_tpe(*hw, True), ht_tpe(*hw, False), ht_hyper_enc(*hw)]
    cs += [dmci_encoder(1, 1), dmci_fusion(1, 1), ld_fusion(1, 1), ld_hyper_enc(2, 2), dmci_hyper_dec(1, 1), ld_adaptor_m(1, 1)]
    for n in (2, 3):
        cs += [dmci_encoder(9, 17, n), dmci_hyper_enc(10, 6, n), dmci_hyper_dec(5, 3, n), dmci_fusion(5, 3, n),
               dmci_spatial_prior(5, 3, n), dmci_decoder(5, 3, n)]
    cs += [ld_adaptor_m(100, 128), ld_encoder(99, 128), ld_decoder(50, 64), ld_spatial_prior(100, 128),
           ld_adaptor_in_place(9, 17), ld_adaptor_in_place(100, 128)]
    # --- float64: single modules and chains of two and three blocks (small grids: the arithmetic does not depend on the grid)
    for hw in ((9, 17), (5, 3)):
        cs += [x_single("i_enc1", *hw), x_single("i_128", *hw, sc=True), x_single("l_128", *hw), x_single("l_256", *hw, sc=True),
               x_single("l_fus", *hw), x_single("i_dec2", *hw), x_single("h_768", *hw), x_single("x_tail256", *hw),
               x_single("x_ffn", *hw, sc=True)]
    cs += [x_single("i_128", 5, 3, batch=2), x_single("l_256", 1, 1),
           x_chain(["l_fai0", "l_256"], 9, 17, "ld2"), x_chain(["l_256"] * 3, 5, 3, "ld3"), x_chain(["l_fus"] * 3, 9, 17, "fus3"),
           x_chain(["i_fus0", "i_512"], 5, 3, "intra2"), x_chain(["l_128"] * 3, 9, 17, "hyper3"),
           x_stride2("i_128", 128, 10, 6, True), x_stride2("l_128", 128, 18, 34, False), x_stride2("l_256", 256, 10, 6, False),
           x_stride2("i_512", 512, 10, 6, True),
           x_upsample("i_128", 128, 5, 3, True), x_upsample("l_128", 128, 9, 17, False), x_upsample("i_384", 256, 5, 3, True)]
    # --- the block form of the intra sequences (DMCI itself runs them as chains): DcbW::forward's next / dc0_done / q_after / fin
    for hw in ((9, 17), (5, 3)):
        cs += [x_blk_encoder(*hw), x_blk_fusion(*hw), x_blk_fusion(*hw, keep=True), x_blk_spatial_prior(*hw), x_blk_decoder(*hw)]
    cs += [x_blk_encoder(5, 3, 2), x_blk_fusion(5, 3, 2), x_blk_spatial_prior(5, 3, 2), x_blk_decoder(5, 3, 2)]
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cs


CASES = _cases()
F64_CASES = [c for c in CASES if c["f64"]]

# every way the three codecs call the layer: the call sites the table must name (test_module_cases_cpu.py)
CALL_SITES = [
    "dmci.hip run_encoder", "dmci.hip run_hyper_and_priors_enc", "dmci.hip run_priors_from_zhat (hyper_dec)",
    "dmci.hip run_priors_from_zhat (y_prior_fusion)", "dmci.hip run_spatial_prior", "dmci.hip run_decoder",
    "dmc_ld.hip run_fa_i, run_fe", "dmc_ld.hip run_fa_m", "dmc_ld.hip run_tpe", "dmc_ld.hip run_encoder",
    "dmc_ld.hip run_hyper_encoder", "dmc_ld.hip run_priors (hyper_decoder)", "dmc_ld.hip run_priors (y_prior_fusion)",
    "dmc_ld.hip run_spatial_prior", "dmc_ld.hip run_decoder", "dmc_ld.hip run_recon_head",
    "dmc_ht.hip run_fa_i", "dmc_ht.hip run_fa_m, run_fe", "dmc_ht.hip run_tpe", "dmc_ht.hip run_encoder",
    "dmc_ht.hip run_hyper_encoder", "dmc_ht.hip run_common (hyper_decoder)", "dmc_ht.hip run_common (y_prior_fusion)",
    "dmc_ht.hip run_spatial_prior", "dmc_ht.hip run_decoder", "dmc_ht.hip run_head",
]


def call_grid(case, call):
    """the grid a call's BLOCKS run on (and, for block / chain calls, the grid of its operands)"""
    g = call.get("grid") or {"stride2": "h", "upsample": "d"}.get(call["op"], "g")
    return grid_of(case, g)


def call_in_grid(case, call):
    """the grid of a call's input"""
    return grid_of(case, call.get("grid", "g"))


# ---------------------------------------------------------------------------------------------- expected branches
BRANCHES = ("tail+dc0", "tail", "pair", "nsplit32", "nsplit64", "dw_inside", "dw_outside", "fin_inside", "fin_behind",
            "ffn_fused", "plain")
# default mode reaches every one of them from the table's shapes; a branch that no shape can reach would be listed here with
# its reason, and test_zz_coverage_report prints it
UNREACHABLE = {}


def predict_block(shape, H, W, batch, xp, yp, altp=None, with_fin=None, fin_packed=True):
    """the branches one DcbW::forward takes in default mode, restated from modules.hip. xp / yp / altp: (buffer, channel
    offset) of the views' first elements (what the pointer comparisons of forward() see), "t3" for the third scratch plane"""
    c, cdc, cffn, cin = shape
    P = H * W
    out = set()
    ns = is_nsplit(c, cdc, cffn)
    tail = (not ns) and tail_supported(H, W, c, cdc, cffn)
    inp = xp
    if cin:
        if altp is None and tail:
            altp = "t3"                      # the adaptor's landing place when the one-launch block cannot run in place
        a = altp if altp is not None and altp != yp else yp
        if ns and B.pair_supported(cin, c, cdc) and a != xp:
            out.add("pair")
        inp = a
    if tail:
        out.add("tail+dc0" if inp != yp else "tail")
        if with_fin:
            out.add("fin_behind")
        return out
    if ns:
        out.add("nsplit64" if B.nsplit_wide(P, c) else "nsplit32")
        out.add("dw_inside" if dw_inside(c, cdc, P, batch) else "dw_outside")
        if with_fin:
            out.add("fin_inside" if fin_packed and with_fin >= 128 and B.fin_supported(c, cdc, with_fin) else "fin_behind")
        return out
    out.add("ffn_fused" if ffn_fused_supported(P, c, cffn) else "plain")
    if with_fin:
        out.add("fin_behind")
    return out


def predict_call(case, call):
    """the branches of one call of the table: run_dcb_chain's choice of outputs and spare buffers, Stride2W's and UpsampleW's
    redirect of tmp == y to the third scratch plane, then predict_block per block (a chain's qf / qa go to its last block;
    no launch choice depends on a scale)"""
    op = call["op"]
    if op == "subpel":
        return set()
    H, W = call_grid(case, call)
    n = case["batch"]
    p = lambda v: None if v is None else (v[0], v[1])
    fw = FINS[case["mods"][call["fin"]["mod"]][1]][1] if call.get("fin") else None
    shapes = block_shapes(case, call["mod"])
    if op == "block":
        return predict_block(shapes[call["i"]], H, W, n, p(call["x"]), p(call["y"]), p(call["alt"]), fw)
    if op in ("stride2", "upsample"):
        c, cdc, cffn, cin = shapes[0]
        tmp, y = p(call["tmp"]), p(call["y"])
        one_launch = not is_nsplit(c, cdc, cffn) and not cin and tail_supported(H, W, c, cdc, cffn)
        if tmp == y and one_launch:
            tmp = "t3"
        return predict_block(shapes[0], H, W, n, tmp, y)
    shapes = shapes[call["first"]:call["first"] + call["n"]] if call["n"] else shapes[call["first"]:]
    out = set()
    x, a, b, y = p(call["x"]), p(call["tmp"]), p(call["tmp2"]), p(call["y"])
    cur = x
    for i, s in enumerate(shapes):
        last = i == len(shapes) - 1
        if b is None:
            dst, alt = (y if last else a), None
        else:
            dst = y
            if not last:
                back = len(shapes) - 1 - i
                dst = ((b if y == a else a) if back % 2 == 1 else (a if y == a else b))
            spare = b if dst == a else a
            alt = None if cur == spare else spare
        out |= predict_block(s, H, W, n, cur, dst, alt, fw if last else None)
        cur = dst
    return out


def classify(variants, has_block, has_fin):
    """launch records (ops.h variant words) of one call -> the branches it took"""
    out = set()
    fams = [v >> 28 for v in variants]
    for v in variants:
        f = v >> 28
        if f == 2:
            out.add("tail+dc0" if v >> 27 & 1 else "tail")
        elif f == 3:
            out.add("ffn_fused")
        elif f == 5:
            out.add("nsplit64" if v >> 25 & 1 else "nsplit32")
            out.add("dw_inside" if v >> 24 & 1 else "dw_outside")
            if (v >> 12 & 0xFFF) > 1:
                out.add("fin_inside")
        elif f == 6:
            out.add("pair")
    if has_block and not any(f in (2, 3, 5) for f in fams):
        out.add("plain")
    if has_fin and "fin_inside" not in out:
        out.add("fin_behind")
    return out


# ---------------------------------------------------------------------------------------------- the launch-sequence reference
class Dev:
    """device copies of prepared operands, made once per case"""

    def __init__(self, torch):
        self.torch = torch
        self.keep = []

    def up(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()
        self.keep.append(t)
        return t

    def empty(self, rows, c):
        t = self.torch.empty((max(rows, 1), c), dtype=self.torch.int16, device="cuda")
        self.keep.append(t)
        return t


def run_reference(ops, U, case, sd, bufs, qs):
    """the plain launch sequence of every call of `case` on the buffers `bufs` (name -> int16 [rows][ld] device tensor).
    U = gpu_util; every intermediate lives in a private dense buffer, so which plane the module layer used cannot matter."""
    import torch
    dev = Dev(torch)
    st = U.stream()
    prep = {}

    def P(prefix):
        if prefix not in prep:
            prep[prefix] = {k: (dev.up(v) if isinstance(v, np.ndarray) else v) for k, v in prep_block(sd, prefix).items()}
        return prep[prefix]

    def vw(view):
        buf, off, c = view
        return U.at(bufs[buf], off), bufs[buf].shape[1], c

    def c1(x, ldx, w, b, y, ldy, pixels, cin, cout, r1=None, ldr1=0, r2=None, ldr2=0, q=None, q2=None, flags=0):
        U.call(ops.conv1x1, x, ldx, U.ptr(w), U.ptr(b), r1, ldr1, r2, ldr2, U.ptr(q), U.ptr(q2), y, ldy, pixels, cin, cout,
               flags, st)

    def block(prefix, x, ldx, y, ldy, H, W, sc=False, qf=None, qa=None, fn=None):
        w = P(prefix)
        NP = case["batch"] * H * W
        c, cdc, cffn = w["c"], w["cdc"], w["cffn"]
        if "wa" in w:
            a = dev.empty(NP, c)
            c1(x, ldx, w["wa"], w["ba"], U.ptr(a), c, NP, w["wa"].shape[1], c)
            x, ldx = U.ptr(a), c
        t1, t2, y1, t3 = dev.empty(NP, cdc), dev.empty(NP, cdc), dev.empty(NP, c), dev.empty(NP, cffn)
        c1(x, ldx, w["w1"], w["b1"], U.ptr(t1), cdc, NP, c, cdc, flags=1)
        U.call(ops.dwconv3x3_b, U.ptr(t1), cdc, U.ptr(w["taps"]), U.ptr(t2), cdc, H, W, cdc, case["batch"], st)
        c1(U.ptr(t2), cdc, w["w3"], w["b3"], U.ptr(y1), c, NP, cdc, c, r1=x, ldr1=ldx)
        c1(U.ptr(y1), c, w["w0"], w["b0"], U.ptr(t3), cffn, NP, c, 4 * cffn, flags=3)
        c1(U.ptr(t3), cffn, w["w2"], w["b2"], y, ldy, NP, cffn, c, r1=U.ptr(y1), ldr1=c, r2=x if sc else None,
           ldr2=ldx if sc else 0, q=qs.get(qf), q2=qs.get(qa))
        if fn is not None:
            fw = f16(sd[fn["mod"] + ".weight"])
            fw, fb = dev.up(fw.reshape(fw.shape[0], -1)), dev.up(f16(sd[fn["mod"] + ".bias"]))
            fy, fld, fc = vw(fn["y"])
            c1(y, ldy, fw, fb, fy, fld, NP, c, fc, q=qs.get(fn["q"]))

    for call in case["calls"]:
        op = call["op"]
        H, W = call_grid(case, call)
        if op == "block":
            x, ldx, _ = vw(call["x"])
            y, ldy, _ = vw(call["y"])
            block(block_prefixes(case, call["mod"])[call["i"]], x, ldx, y, ldy, H, W, call["sc"], call["qf"], call["qa"], call["fin"])
        elif op == "chain":
            pre = block_prefixes(case, call["mod"])
            pre = pre[call["first"]:call["first"] + call["n"]] if call["n"] else pre[call["first"]:]
            x, ldx, _ = vw(call["x"])
            for i, p in enumerate(pre):
                last = i == len(pre) - 1
                if last:
                    y, ldy, _ = vw(call["y"])
                else:
                    c = P(p)["c"]
                    y, ldy = U.ptr(dev.empty(case["batch"] * H * W, c)), c
                block(p, x, ldx, y, ldy, H, W, False, call["qf"] if last else None, call["qa"] if last else None,
                      call["fin"] if last else None)
                x, ldx = y, ldy
        elif op == "stride2":
            m = case["mods"][call["mod"]]
            p = call["mod"] + "."
            Hi, Wi = call_in_grid(case, call)
            cin, c = m[1], SHAPES[m[2]][0]
            x, ldx, _ = vw(call["x"])
            y, ldy, _ = vw(call["y"])
            t = dev.empty(case["batch"] * H * W, c)
            U.call(ops.conv_kxk_b, x, ldx, U.ptr(dev.up(prep_stride2(sd[p + "down.weight"]))), U.ptr(dev.up(f16(sd[p + "down.bias"]))),
                   U.ptr(t), c, Hi, Wi, cin, c, 2, 2, 0, case["batch"], st)
            block(p + "conv.", U.ptr(t), c, y, ldy, H, W, sc=m[3])
        else:
            m = case["mods"][call["mod"]]
            up = op == "upsample"
            p = call["mod"] + (".up." if up else ".")
            Hi, Wi = call_in_grid(case, call)
            cin, cout, k, bias = (m[1], SHAPES[m[2]][0], m[4], m[5]) if up else m[1:]
            x, ldx, _ = vw(call["x"])
            y, ldy, _ = vw(call["y"])
            if up:
                o = dev.empty(4 * case["batch"] * Hi * Wi, cout)
                dst, ldd = U.ptr(o), cout
            else:
                dst, ldd = y, ldy
            w = sd[p + "conv.0.weight"]
            if not bias:
                U.call(ops.tconv2x2_b, x, ldx, U.ptr(dev.up(prep_subpel(w))), dst, ldd, Hi, Wi, cin, cout, case["batch"], st)
            else:
                assert case["batch"] == 1
                t = dev.empty(Hi * Wi, 4 * cout)
                bb = dev.up(f16(sd[p + "conv.0.bias"]))
                if k == 1:
                    c1(x, ldx, dev.up(f16(w).reshape(4 * cout, cin)), bb, U.ptr(t), 4 * cout, Hi * Wi, cin, 4 * cout)
                else:
                    U.call(ops.conv_kxk, x, ldx, U.ptr(dev.up(prep_convk(w))), U.ptr(bb), U.ptr(t), 4 * cout, Hi, Wi, cin,
                           4 * cout, k, 1, k // 2, st)
                U.call(ops.shuffle2, U.ptr(t), 4 * cout, Hi, Wi, cout, dst, ldd, st)
            if up:
                block(call["mod"] + ".conv.", U.ptr(o), cout, y, ldy, H, W, sc=m[3])
    torch.cuda.synchronize()
    return dev


# ---------------------------------------------------------------------------------------------- the float64 reference
def fold_bias64(R, w3, b2, b3):
    """(s, e_fold): the float64 bias W3 b2 + b3 of dc.3 and the allowance for DcbW::load's fp32 chain and two fp16 roundings
    (derived in this module's docstring)"""
    import torch
    w, b2, b3 = w3.double().reshape(w3.shape[0], -1), b2.double(), b3.double()
    K = w.shape[1]
    a = w @ b2
    A = w.abs() @ b2.abs()
    ch = (K + 1) * R.U32 * A
    u1 = R.ulp16(a.abs() + ch)
    s = a + b3
    S = s.abs() + ch + u1 / 2
    u2 = R.ulp16(S * (1 + R.U32))
    return s, ch + u1 / 2 + R.U32 * S + u2 / 2


def f64_block(R, sd, p, x, geom, sc=False, q=None, q2=None):
    """one DepthConvBlock in float64 from the checkpoint-layout tensors at prefix p. x: fp16 tensor or Mid, [n H W, cin];
    geom = (n, H, W). Returns the Approx of the block output."""
    two = lambda t: t.reshape(t.shape[0], -1)
    x = R._mid(x)
    if p + "adaptor.weight" in sd:
        x = R.Mid.of(R.conv1x1(x, two(sd[p + "adaptor.weight"]), sd[p + "adaptor.bias"]))
    t1 = R.Mid.of(R.conv1x1(x, two(sd[p + "dc.0.weight"]), sd[p + "dc.0.bias"], wsilu=True))
    taps = two(sd[p + "dc.2.weight"]).t().contiguous()           # [9][cdc] (exact: a re-layout)
    t2 = R.Mid.of(R.dwconv3x3(t1, taps, *geom))
    s, e_fold = fold_bias64(R, sd[p + "dc.3.weight"], sd[p + "dc.2.bias"], sd[p + "dc.3.bias"])
    acc, e = R._contract(t2.mid, two(sd[p + "dc.3.weight"]), s, t2.rad)
    y1 = R.epilogue(acc, e + e_fold, r1=x.mid, r1_rad=x.rad)
    f = R.ffn(R.Mid.of(y1), two(sd[p + "ffn.0.weight"]), sd[p + "ffn.0.bias"], two(sd[p + "ffn.2.weight"]), sd[p + "ffn.2.bias"],
              r2=x if sc else None, q=q, q2=q2)
    return f["y"]


def f64_call(R, case, sd, x, qs):
    """the float64 Approx of the output view of a single-call case; x: the input view's fp16 tensor [n, H, W, cin]"""
    call = case["calls"][0]
    n = case["batch"]
    H, W = call_grid(case, call)
    geom = (n, H, W)
    x2 = x.reshape(-1, x.shape[-1])
    op = call["op"]
    if op == "block":
        return f64_block(R, sd, call["mod"] + ".", x2, geom, call["sc"], qs.get(call["qf"]), qs.get(call["qa"]))
    if op == "chain":
        pre = block_prefixes(case, call["mod"])
        cur = x2
        for i, p in enumerate(pre):
            last = i == len(pre) - 1
            ap = f64_block(R, sd, p, cur, geom, q=qs.get(call["qf"]) if last else None, q2=qs.get(call["qa"]) if last else None)
            cur = R.Mid.of(ap)
        return ap
    m = case["mods"][call["mod"]]
    p = call["mod"] + "."
    if op == "stride2":
        # pixel_unshuffle(2) + 1x1 conv: input channel c * 4 + dy * 2 + dx of down.weight is tap (dy, dx) of channel c
        w = sd[p + "down.weight"]
        w4 = w.reshape(w.shape[0], m[1], 2, 2)
        t = R.Mid.of(R.conv_kxk(x, w4, sd[p + "down.bias"], 2, 2, 0))
        return f64_block(R, sd, p + "conv.", t, geom, sc=m[3])
    if op == "upsample":
        # 1x1 conv to 4 cout channels + pixel_shuffle(2): row co * 4 + dy * 2 + dx lands at (2h + dy, 2w + dx, co)
        w = sd[p + "up.conv.0.weight"]
        cout = w.shape[0] // 4
        w4 = w.reshape(cout, 4, w.shape[1]).permute(1, 0, 2).contiguous()
        ap = R.tconv2x2(x, w4)
        t = R.Mid.of(R.Approx(ap.t.reshape(-1, cout), ap.e.reshape(-1, cout)))
        return f64_block(R, sd, p + "conv.", t, geom, sc=m[3])
    raise ValueError(op)


def nn_block64(sd, p, x, sc=False, q=None, q2=None):
    """the same block as a plain torch float64 nn-style forward (DepthConvBlock: adaptor; out = dc(x) + x with dc = conv1x1,
    WSiLU, depthwise 3x3 WITH its bias, conv1x1; out = ffn(out) + out with ffn = conv1x1, WSiLU, chunk(4)-sum, conv1x1;
    + x with the block shortcut), no rounding anywhere. x [n, C, H, W] float64."""
    import torch
    import torch.nn.functional as F
    d = lambda k: sd[p + k].double()
    wsilu = lambda v: v * torch.sigmoid(4.0 * v)
    if p + "adaptor.weight" in sd:
        x = F.conv2d(x, d("adaptor.weight"), d("adaptor.bias"))
    t = wsilu(F.conv2d(x, d("dc.0.weight"), d("dc.0.bias")))
    t = F.conv2d(t, d("dc.2.weight"), d("dc.2.bias"), padding=1, groups=t.shape[1])
    y1 = F.conv2d(t, d("dc.3.weight"), d("dc.3.bias")) + x
    u = wsilu(F.conv2d(y1, d("ffn.0.weight"), d("ffn.0.bias")))
    n, c4, H, W = u.shape
    u = u.reshape(n, c4 // 4, 4, H, W).sum(2)                    # output channel j sums ffn.0's channels 4j .. 4j + 3
    y = F.conv2d(u, d("ffn.2.weight"), d("ffn.2.bias")) + y1
    if sc:
        y = y + x
    if q is not None:
        y = y * q.double().view(1, -1, 1, 1)
    if q2 is not None:
        y = y * q2.double().view(1, -1, 1, 1)
    return y
