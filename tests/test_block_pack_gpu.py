"""The block kernels' packed weight streams, byte for byte (-m gpu).

dcb_nsplit_pack_main / _dc0 / _fin and dcb_pair_pack_adaptor (dcvc_amd/csrc/kernels/dcb_nsplit.hip, dcb_pair.hip) write the
per-wave streams the kernels consume; a fragment out of place is a wrong weight in a wave's registers. The layout is restated
here in numpy from the comment at the top of dcb_nsplit.hip, with no arithmetic shared with the library:

* a stream is [8 waves][fragments][64 lanes][8 halves]; a fragment is one (32-channel tile, 16-deep k-slice) of a layer [N][K]:
  lane l holds row 32 tile + (l & 31), k = 16 slice + 8 (l >> 5) .. + 7;
* a wave's fragments of a layer: k-slice major, the wave's tiles inside;
* tiles BY SIMD PAIR (N a multiple of 128: N / 128 tiles per pair, wave w < 4 the first half rounded up, wave w + 4 the rest)
  or BY WAVE (waves 0 .. 3 ceil(tiles / 8) each, then as many of the waves 4 .. 7 as the rest fills, the others a tile of zeros);
* main = per wave dc.3 | ffn.0 | ffn.2; ffn.0's 4 CI channels in pairs of tiles, passes of two tiles, k-slice major inside a pass.

No pixels, no launches of the block kernels: every shape of tests/block_cases.py in a few milliseconds."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_cases as B  # noqa: E402

pytestmark = pytest.mark.gpu

MAIN, DC0, FIN, ADAPTOR = 0, 1, 2, 3
TAIL = 1024                         # halves behind the stream that must stay untouched
vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


# ---------------------------------------------------------------------------------------------- the layout, restated
def by_pair(n):
    """tiles of the waves 0 .. 7 of an n-wide layer, n a multiple of 128"""
    assert n % 128 == 0
    q = n // 128
    hi = (q + 1) // 2
    return [[(w & 3) * q + (0 if w < 4 else hi) + j for j in range(hi if w < 4 else q - hi)] for w in range(8)]


def by_wave(n):
    """... by wave; None = a tile of zeros (a wave without a share still walks one)"""
    tn = n // 32
    hi = -(-tn // 8)
    rem = tn - 4 * hi
    lo = -(-rem // 4) if rem > 0 else 0
    act = rem // lo if lo else 0
    assert 4 * hi + act * lo == tn
    return [[w * hi + j for j in range(hi)] for w in range(4)] + \
           [[4 * hi + w * lo + j if w < act else None for j in range(lo)] for w in range(4)]


def block_layer(n):
    return by_pair(n) if n % 128 == 0 else by_wave(n)


def fragment(w, tile, ks):
    """[64][8] uint16"""
    if tile is None:
        return np.zeros((64, 8), np.uint16)
    lane = np.arange(64)
    rows = 32 * tile + (lane & 31)
    k = 16 * ks + 8 * (lane >> 5)
    return w[rows[:, None], k[:, None] + np.arange(8)[None, :]]


def layer_segment(w, tiles):
    """one wave's fragments of the layer w [N][K]"""
    return [fragment(w, t, ks) for ks in range(w.shape[1] // 16) for t in tiles]


def cat(frags):
    return np.concatenate([f.reshape(-1) for f in frags]) if frags else np.zeros((0,), np.uint16)


def layer_stream(w, shares):
    return cat([f for wave in range(8) for f in layer_segment(w, shares[wave])])


def main_stream(w3, w0, w2, C, CI):
    shares = block_layer(C)
    pairs = CI // 16                                   # ffn.0: 4 CI / 32 tiles, two to a pair
    p_hi = -(-pairs // 8)
    p_lo = (pairs - 4 * p_hi) // 4
    assert 4 * (p_hi + p_lo) == pairs and p_lo >= 1
    frags = []
    for wave in range(8):
        frags += layer_segment(w3, shares[wave])
        first = wave * 2 * p_hi if wave < 4 else 4 * 2 * p_hi + (wave - 4) * 2 * p_lo         # the wave's first ffn.0 tile
        for p in range(p_hi if wave < 4 else p_lo):
            frags += [fragment(w0, first + 2 * p + t, ks) for ks in range(C // 16) for t in range(2)]
        frags += layer_segment(w2, shares[wave])
    return cat(frags)


# ---------------------------------------------------------------------------------------------- the library's streams
@pytest.fixture(scope="module")
def pack():
    assert torch.cuda.is_available(), "needs the MI355X"
    from dcvc_amd import _lib
    from dcvc_amd.plugin import MLCodec_extensions_cpp  # noqa: F401  (loads the library)
    fn = _lib.fn("dcvc_modtest_pack_stream", cll, [ci, vp, vp, vp, ci, ci, vp, cll, vp])

    def run(kind, ws, a, b, expect):
        dev = [torch.from_numpy(w.view(np.int16)).cuda() for w in ws] + [None] * (3 - len(ws))
        out = torch.full((expect.size + TAIL,), -1, dtype=torch.int16, device="cuda")          # 0xFFFF everywhere
        n = fn(kind, *[None if t is None else vp(t.data_ptr()) for t in dev], a, b, vp(out.data_ptr()), out.numel(),
               vp(torch.cuda.current_stream().cuda_stream))
        if n < 0:
            raise _lib.DcvcError(_lib.lib().dcvc_last_error().decode())
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint16)
        assert n == expect.size, "size in halves: %d, the layout has %d" % (n, expect.size)
        assert np.array_equal(got[:n], expect), "first difference at half %d" % int(np.argmax(got[:n] != expect))
        assert bool((got[n:] == 0xFFFF).all()), "written behind the stream"
    return run


def weights(seed, n, k):
    """random fp16 BIT PATTERNS (NaNs and infinities included: the pack copies bits)"""
    return np.random.default_rng(seed).integers(0, 1 << 16, size=(n, k), dtype=np.uint16)


FIN_CASES = [(c, ci_, nn) for (c, ci_), fins in sorted(B.FINS.items()) for nn in fins]
ADAPTOR_CASES = sorted({(cin, c) for cin, c, _ in B.PAIR_SHAPES})


@pytest.mark.parametrize("C,CI", B.NSPLIT_SHAPES)
def test_main_stream(pack, C, CI):
    w3, w0, w2 = weights(1, C, CI), weights(2, 4 * CI, C), weights(3, C, CI)
    pack(MAIN, [w3, w0, w2], C, CI, main_stream(w3, w0, w2, C, CI))


@pytest.mark.parametrize("C,CI", B.NSPLIT_SHAPES)
def test_dc0_stream(pack, C, CI):
    w1 = weights(4, CI, C)
    pack(DC0, [w1], C, CI, layer_stream(w1, block_layer(CI)))


@pytest.mark.parametrize("C,CI,NN", FIN_CASES)
def test_closing_conv_stream(pack, C, CI, NN):
    w = weights(5, NN, C)
    pack(FIN, [w], C, NN, layer_stream(w, by_wave(NN)))


@pytest.mark.parametrize("CIN,C", ADAPTOR_CASES)
def test_adaptor_stream(pack, CIN, C):
    w = weights(6, C, CIN)
    pack(ADAPTOR, [w], CIN, C, layer_stream(w, block_layer(C)))

