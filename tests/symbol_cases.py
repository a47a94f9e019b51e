"""Inputs of tests/test_symbols_edges_gpu.py and the oracle chains they are compared with. TEST INFRASTRUCTURE ONLY (a helper
module, not a conftest): tests/test_symbol_cases_cpu.py proves on the CPU, from oracle/symbols_np.py alone, that every case
reaches what it claims - the int8 clamp on both sides, both infinities, exact ties, an fp16 overflow of y - mean, every entry of
the scale-to-index table and both sides of the skip threshold - so a case that misses its edge fails before it reaches a GPU.

All tensors are numpy float16 [H, W, C] (NHWC), built from bit patterns or from a seeded numpy generator.

NOT covered, on purpose: NaN in y, in the means or in q_dec. The reference clamps with max(at::Half, ...) / min(...), and what
those do with a NaN operand is not pinned by anything the reference documents; the oracle (numpy maximum / minimum propagate the
NaN) and the kernels (fmaxf / fminf drop it) differ there. NaN *scales* are covered: both sides send them to the table's first
entry with the keep flag off. The sign of a zero in y_hat is not pinned either (the reference accumulates y_hat_so_far with
adds, the kernels store the active group): y_hat is compared as fp16 values, symbols, indexes, flags and counts as integers."""
import numpy as np

from oracle import symbols_np as orc

F16 = np.float16
SENT = 0x7E5A                       # NaN payload around every output, as in the GEMM tests
BLOCK = 2048                        # symbols per workgroup of the symbol kernels (symbols.hip kBlockElems)
THRESHOLDS = (0.0, 0.15)


def from_bits(b):
    return np.asarray(b, dtype=np.uint16).view(F16)


def bits(x):
    return np.ascontiguousarray(x, dtype=F16).view(np.uint16)


def bit(x):
    """the bit pattern of one fp16 value"""
    return int(np.asarray(x, dtype=F16).reshape(1).view(np.uint16)[0])


def symbol_blocks(count):
    return (count + BLOCK - 1) // BLOCK


def _groups4(v, H, W, C):
    """[H*W*C/4] values -> [H, W, C] with the same C/4 values in each of the four channel groups of a pixel: whichever group a
    step activates at a pixel, every step sees every value once (and each of the 2 / 4 full-tensor steps too: the four groups
    of a pixel belong to four different steps, its two channel halves to two)."""
    return np.ascontiguousarray(np.tile(v.reshape(H, W, C // 4), (1, 1, 4)))


def _rng(seed):
    return np.random.default_rng(seed)


def mild(shape, scale, seed):
    return (_rng(seed).standard_normal(shape) * scale).astype(F16)


def mild_scales(shape, seed):
    return (np.exp(_rng(seed).standard_normal(shape)) * 0.3).astype(F16)


# ------------------------------------------------------------------------------------------------------------ scale_sweep
SCALE_SWEEP_SHAPE = (32, 64, 128)        # 2048 pixels x 32 symbols = every one of the 65536 fp16 bit patterns


def scale_sweep():
    H, W, C = SCALE_SWEEP_SHAPE
    patterns = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    return {"H": H, "W": W, "C": C, "patterns": patterns.view(F16),
            "scales": _groups4(patterns.view(F16), H, W, C),
            "y": mild((H, W, C), 6.0, 101), "means": [mild((H, W, C), 2.0, 102 + k) for k in range(4)],
            "q_dec": (mild((H, W, C), 0.6, 107).astype(np.float32) + 0.9).astype(F16)}


# ------------------------------------------------------------------------------------------------------------ quant_sweep
QUANT_MEANS = (0.0, 0.5, -3.25, 100.0, 6e-8, -65504.0)
QUANT_SHAPE = (125, 96, 128)             # 12000 pixels x 32 symbols >= 6 x 63490 (y, mean) pairs; an odd height


def non_nan_patterns():
    b = np.arange(65536, dtype=np.uint32)
    return b[(b & 0x7fff) <= 0x7c00].astype(np.uint16)


def index_scales():
    """128 scales, entry i inside the table's bucket i (found from the oracle over all positive patterns)"""
    s = from_bits(np.arange(0x0001, 0x7c00, dtype=np.uint16))
    idx = orc.scale_to_index(s)
    first = np.array([np.flatnonzero(idx == i)[0] for i in range(128)])
    last = np.array([np.flatnonzero(idx == i)[-1] for i in range(128)])
    return s[(first + last) // 2]


def quant_sweep():
    H, W, C = QUANT_SHAPE
    n = H * W * (C // 4)
    pat = non_nan_patterns().view(F16)
    y = np.zeros(n, F16)
    m = np.zeros(n, F16)
    y[:6 * pat.size] = np.tile(pat, 6)
    m[:6 * pat.size] = np.repeat(np.array(QUANT_MEANS, dtype=F16), pat.size)
    # scales: all 128 table entries in turn (the entries at and below the skip threshold included)
    sc = index_scales()[np.arange(n) % 128]
    # q_dec of the full-tensor steps: 1 for most (y unchanged: the clamps stay reached), some below 0.5, one 65504
    q = np.ones(n, F16)
    q[3::7] = np.array([0.25, 0.4375, 2.0, 0.5, 3.0], F16)[np.arange(q[3::7].size) % 5]
    q[0] = F16(65504)
    return {"H": H, "W": W, "C": C, "y": _groups4(y, H, W, C), "means": _groups4(m, H, W, C),
            "scales": _groups4(sc, H, W, C), "q_dec": _groups4(q, H, W, C)}


def quant_picture(H, W, C):
    """an H x W x C picture cut from the sweep's value list: the first half runs upwards from 120 and the second downwards
    from -120 (through the clamp on either side and, when the picture is large enough, on to the infinity), against the first
    four means in turn and every table entry"""
    n = H * W * (C // 4)
    pat = non_nan_patterns().view(F16)
    up, down = int(np.flatnonzero(pat == F16(120.0))[0]), int(np.flatnonzero(pat == F16(-120.0))[0])
    y = np.concatenate([pat[up:up + n // 2], pat[down:down + n - n // 2]])
    assert y.size == n
    m = np.array(QUANT_MEANS[:4], dtype=F16)[np.arange(n) % 4]
    sc = index_scales()[(np.arange(n) * 5 + 3) % 128]
    return {"y": _groups4(y, H, W, C), "means": _groups4(m, H, W, C), "scales": _groups4(sc, H, W, C)}


# ------------------------------------------------------------------------------------------------------------ geometries
# (H, W, C, what): symbols per picture = H * W * C / 4
GEOMETRIES = [
    (16, 16, 32, "exactly one block"),
    (8, 8, 128, "exactly one block, 32 symbols per pixel"),
    (15, 17, 32, "one block less 8"),
    (1, 257, 32, "one block plus 8"),
    (273, 241, 32, "257 blocks plus 8: the sum over earlier blocks takes a second pass"),
    (5, 3, 256, "one ragged block"),
    (5, 3, 32, "one ragged block, one vector per pixel"),
    (17, 30, 128, "eight blocks, the last ragged"),
    (96, 96, 256, "288 full blocks"),
]


def geometry_count(H, W, C):
    return H * W * (C // 4)


# ------------------------------------------------------------------------------------------------------------ oracle chains
@np.errstate(all="ignore")       # an fp16 overflow to Inf is one of the cases, not an accident
def y_steps(y, scales, means, thres):
    """The four autoregressive steps of the intra y coding, op by op as the reference runs them. scales / means: one tensor
    per step. -> per step: sym (int16, uncompacted), keep (bool), idx (uint8), acc (y_hat_so_far after the step)."""
    H, W, C = y.shape
    masks = orc.get_mask_4x(H, W, C)
    acc = np.zeros((H, W, C), F16)
    out = []
    for k in range(4):
        y_q, y_hat, s_hat = orc.process_with_mask(y, scales[k], means[k], masks[k], thres)
        comb, keep = orc.build_index_enc(orc.fold4(y_q), orc.fold4(s_hat), thres)
        s_r = orc.fold4(np.where(masks[k], scales[k], F16(0)))
        idx, keep_d = orc.build_index_dec(s_r, thres)
        assert np.array_equal(keep, keep_d) and np.array_equal(idx, (comb & 0xff).astype(np.uint8))
        acc = (acc + y_hat).astype(F16)
        out.append({"sym": comb, "keep": keep, "idx": idx, "acc": acc.copy()})
    return out


@np.errstate(all="ignore")
def mask_steps(y, q_dec, scales, means, nsteps, thres):
    """The inter models' full-tensor steps (means: one tensor per step) -> y / max(q, 0.5), sym, keep, idx, final y_hat"""
    H, W, C = y.shape
    masks = orc.get_mask_2x(H, W, C) if nsteps == 2 else orc.get_mask_4x(H, W, C)
    y_div = orc.divide_with_clamp(y, q_dec)
    y_q_all = np.zeros((H, W, C), F16)
    y_hat = np.zeros((H, W, C), F16)
    for k in range(nsteps):
        yq, yh = orc.process_with_mask_2x(y_div, scales, means[k], masks[k], thres)
        y_q_all = (y_q_all + yq).astype(F16)
        y_hat = (y_hat + yh).astype(F16)
    y_hat = (y_hat * orc.clamp_min_half(q_dec)).astype(F16)
    comb, keep = orc.build_index_enc(y_q_all, scales, thres)
    idx, _ = orc.build_index_dec(scales, thres)
    return {"y_div": y_div, "sym": comb, "keep": keep, "idx": idx, "y_hat": y_hat}
