"""numpy restatement of the code-length tables (dcvc_amd/csrc/rans/code_length.cpp) and of the sums the device kernels
take over them (csrc/kernels/code_length.hip), plus the inputs the prediction tests share.

An entry is the cost of one symbol under one CDF in units of 2^-16 bit: rint(65536 * (16 - log2(freq))) in float64 for
the value the coder codes, plus 2 bits for every bypass group of an escaped value. The symbol -> value mapping, the escape
and the group count follow enc_symbol of csrc/rans/rans_coder.cpp."""
import numpy as np

UNIT = 1 << 16
UNCODABLE = 0xFFFFFFFF


def cost(freq, groups=0):
    """uint64 array: cost of values of frequency `freq` (1 .. 65536) followed by `groups` bypass groups"""
    freq = np.asarray(freq, dtype=np.float64)
    base = np.rint(UNIT * (16.0 - np.log2(freq))).astype(np.uint64)
    return base + np.asarray(groups, dtype=np.uint64) * np.uint64(2 * UNIT)


def value_and_groups(sym, max_value):
    """(coded value, bypass groups) of symbol `sym` under a CDF whose escape value is max_value"""
    value = abs(sym) * 2 - (1 if sym > 0 else 0)
    if value < max_value:
        return value, 0
    raw = value - max_value
    n_groups = 0
    while (raw >> (2 * n_groups)) != 0:
        n_groups += 1
    return max_value, n_groups + 1 + n_groups // 3


def table(cdfs, cdf_sizes, cols):
    """[num_cdf][cols] uint32: cols = 256 -> column uint8(symbol) (y), cols = 128 -> column symbol + 64 (z)"""
    cdfs = np.asarray(cdfs, dtype=np.int64)
    out = np.zeros((cdfs.shape[0], cols), dtype=np.uint32)
    for i in range(cdfs.shape[0]):
        max_value = int(cdf_sizes[i]) - 2
        for col in range(cols):
            sym = (col - 256 if col >= 128 else col) if cols == 256 else col - 64
            v, groups = value_and_groups(sym, max_value)
            freq = int(cdfs[i, v + 1] - cdfs[i, v]) & 0xFFFF
            out[i, col] = UNCODABLE if freq == 0 else int(cost(freq, groups))
    return out


def sum_y(table_y, comb, keep=None):
    """(units, symbols counted) of int16 symbols (q << 8) + index; keep: bool per symbol or None = all"""
    comb = np.asarray(comb, dtype=np.int16).astype(np.int64) & 0xFFFF
    idx, col = comb & 0xFF, comb >> 8
    on = idx < table_y.shape[0]
    if keep is not None:
        on &= np.asarray(keep, dtype=bool)
    return int(table_y[idx[on], col[on]].astype(np.uint64).sum()), int(on.sum())


def sum_z(table_z_rows, z, ch):
    """units of int8 z symbols, symbol i under row i % ch of table_z_rows"""
    z = np.asarray(z, dtype=np.int8).astype(np.int64)
    return int(table_z_rows[np.arange(z.size) % ch, (z + 64) & 127].astype(np.uint64).sum())


def unpack_keep(cond, count):
    """keep flags of the device layout: bit e % 8 of byte e // 8"""
    return np.unpackbits(np.asarray(cond, dtype=np.uint8), bitorder="little")[:count].astype(bool)


def draw_from_tables(cdfs, cdf_sizes, seed, count):
    """`count` y symbols, each under a random CDF and drawn from that CDF's own distribution (the escape value itself
    stands for its whole tail), as int16 (q << 8) + index"""
    rng = np.random.default_rng(seed)
    cdfs = np.asarray(cdfs, dtype=np.int64)
    idx = rng.integers(0, cdfs.shape[0], count)
    u = rng.integers(0, 1 << 16, count)
    value = np.zeros(count, dtype=np.int64)
    for i in range(cdfs.shape[0]):
        m = idx == i
        row = cdfs[i, 1:int(cdf_sizes[i])]
        value[m] = np.searchsorted(row, u[m], side="right")
    sym = np.where(value % 2 == 0, -(value // 2), (value + 1) // 2)
    return ((sym << 8) + idx).astype(np.int16)
