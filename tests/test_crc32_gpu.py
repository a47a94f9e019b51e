"""dcvc_crc32_segments on a real MI355X (-m gpu), DESIGN.md 19: every value is zlib.crc32 of the segment's bytes, at the
lengths and start addresses where the kernel changes path (crc32.hip: 16-byte words, 64-byte thread chunks, 16 KiB workgroups),
for every single set bit around those boundaries, for 16 segments in one call and beyond 2^31 bytes."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import crc32_np
from dcvc_amd import _lib, picture_hash as ph

pytestmark = pytest.mark.gpu

CHUNK = 64                   # bytes of one thread
GROUP = 256 * CHUNK          # bytes of one workgroup
LENGTHS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, CHUNK * 3 - 1, CHUNK * 3, CHUNK * 3 + 1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP,
           300001]


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _want(buf, offsets, lengths):
    raw = buf.tobytes()
    return [zlib.crc32(raw[o:o + n]) for o, n in zip(offsets, lengths)]


def _check(buf, offsets, lengths):
    """buf: numpy uint8; the segments in calls of up to 16"""
    t = _dev(buf)
    for at in range(0, len(offsets), 16):
        o, n = offsets[at:at + 16], lengths[at:at + 16]
        got, want = ph.crc32_segments(t, o, n), _want(buf, o, n)
        assert got == want, [(oo, nn, hex(g), hex(w)) for oo, nn, g, w in zip(o, n, got, want) if g != w]


@pytest.fixture(scope="module")
def random_bytes():
    return np.random.default_rng(32).integers(0, 256, 2 * GROUP + 300001 + 64, dtype=np.uint8)


def test_lengths(random_bytes):
    _check(random_bytes, [0] * len(LENGTHS), LENGTHS)


def test_every_start_offset_of_a_16_byte_word(random_bytes):
    lengths = [1, 5, 15, 16, 17, 31, 48, 49, 64, 65, 100, GROUP - 16, GROUP, GROUP + 7, 20000]
    offsets, lens = zip(*[(o, n) for n in lengths for o in range(16)])
    _check(random_bytes, list(offsets), list(lens))


@pytest.mark.parametrize("fill", [0x00, 0xFF], ids=["zeros", "ones"])
def test_constant_contents(fill):
    buf = np.full(2 * GROUP + 100, fill, dtype=np.uint8)
    lengths = [n for n in LENGTHS if n <= buf.size]
    _check(buf, [0] * len(lengths) + [3] * len(lengths), lengths + [max(0, n - 3) for n in lengths])
    # the init term: runs of zero bytes of different lengths hash differently (the raw CRC of each is 0)
    got = ph.crc32_segments(_dev(buf), [0, 0, 0, 0, 0], [1, 2, CHUNK, GROUP, GROUP + 1])
    assert len(set(got)) == 5 and 0 not in got


def _basis_positions(length):
    """bit positions: every bit of the first and the last 64 bytes, and the bits either side of every chunk and workgroup
    boundary"""
    bits = set(range(8 * 64)) | set(range(8 * (length - 64), 8 * length))
    for edge in range(CHUNK, length, CHUNK):
        bits |= {8 * edge - 1, 8 * edge}
    for edge in range(16, 4 * CHUNK, 16):                  # and of the 16-byte words of the first chunks
        bits |= {8 * edge - 1, 8 * edge}
    bits |= {8 * GROUP - 8, 8 * GROUP + 7}
    return sorted(bits)


@pytest.mark.parametrize("start", [0, 5], ids=["aligned", "start_5"])
def test_bit_basis(start):
    """a buffer a little over one workgroup's bytes with exactly one bit set: any error in a positional multiplier shows.
    16 copies of the buffer per call, each with its own bit; the copies start `start` bytes behind a 16-byte boundary."""
    length = GROUP + 200
    stride = (length + start + 15) // 16 * 16
    bits = _basis_positions(length)
    assert len(bits) > 1500
    zeros = zlib.crc32(bytes(length))
    seen = set()
    for at in range(0, len(bits), 16):
        group = bits[at:at + 16]
        buf = np.zeros(stride * 16, dtype=np.uint8)
        offsets = [k * stride + start for k in range(len(group))]
        for o, bit in zip(offsets, group):
            buf[o + bit // 8] = 1 << (bit % 8)
        got = ph.crc32_segments(_dev(buf), offsets, [length] * len(group))
        want = _want(buf, offsets, [length] * len(group))
        assert got == want, [(b, hex(g), hex(w)) for b, g, w in zip(group, got, want) if g != w]
        seen |= set(got)
    assert len(seen) == len(bits) and zeros not in seen          # every bit position has a CRC of its own


def _raw_call(t, offsets, lengths, out):
    n = len(offsets)
    f = _lib.fn("dcvc_crc32_segments", ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong),
                                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p])
    _lib.check(f(ctypes.c_void_p(t.data_ptr()), (ctypes.c_longlong * n)(*offsets), (ctypes.c_longlong * n)(*lengths), n,
                 ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def test_16_segments_in_one_call(random_bytes):
    lengths = [GROUP + 5, 0, 1, 77, 2 * GROUP, 0, 15, 16, 4097, 64, 0, 33333, 3, GROUP - 1, 640, 0]
    gaps = [3, 0, 7, 1, 16, 5, 0, 9, 2, 64, 11, 13, 1, 0, 6, 4]
    offsets, at = [], 1
    for n, g in zip(lengths, gaps):
        offsets.append(at)
        at += n + g
    buf = random_bytes[:at + 8].copy()
    want = _want(buf, offsets, lengths)
    assert [w for w, n in zip(want, lengths) if n == 0] == [0, 0, 0, 0]
    sentinel = 0x5A5A5A5A
    out = torch.full((24,), sentinel, dtype=torch.int32, device="cuda")
    t = _dev(buf)
    _raw_call(t, offsets, lengths, out)
    got = [int(v) & 0xFFFFFFFF for v in out.tolist()]
    assert got[:16] == want and got[16:] == [sentinel] * 8, "crc_out[n..] must keep what it held"
    # fewer segments: the words behind them stay too
    out.fill_(sentinel)
    _raw_call(t, offsets[:3], lengths[:3], out)
    got = [int(v) & 0xFFFFFFFF for v in out.tolist()]
    assert got[:3] == want[:3] and got[3:] == [sentinel] * 21
    # the bytes between the segments are not part of any result
    inside = np.zeros(buf.size, dtype=bool)
    for o, n in zip(offsets, lengths):
        inside[o:o + n] = True
    assert (~inside).sum() >= sum(gaps)
    other = buf.copy()
    other[~inside] ^= 0xFF
    assert ph.crc32_segments(_dev(other), offsets, lengths) == want
    # ... and in any order, overlapping
    order = [5, 0, 11, 4, 4, 13]
    assert ph.crc32_segments(t, [offsets[k] for k in order], [lengths[k] for k in order]) == [want[k] for k in order]


def test_repeats_and_split_views(random_bytes):
    t = _dev(random_bytes)
    n = random_bytes.size
    whole = ph.crc32_segments(t, [7], [n - 7])
    assert whole == ph.crc32_segments(t, [7], [n - 7]) == [zlib.crc32(random_bytes[7:].tobytes())]
    cuts = [7, 7 + 12345, 7 + 12345 + GROUP + 1, n]
    parts = ph.crc32_segments(t, cuts[:3], [cuts[k + 1] - cuts[k] for k in range(3)])
    crc = 0
    for k in range(3):
        crc = ph.crc32_combine(crc, parts[k], cuts[k + 1] - cuts[k])
    assert crc == whole[0]


@pytest.mark.parametrize("H,W", [(18, 18), (48, 64)], ids=["18x18", "64x48"])
@pytest.mark.parametrize("es", [1, 2], ids=["8bit", "16bit"])
def test_the_planes_of_a_yuv420_picture(H, W, es):
    rng = np.random.default_rng(H * es)
    hw = H * W
    buf = rng.integers(0, 256, hw * 3 // 2 * es, dtype=np.uint8)
    offsets = [0, hw * es, (hw + hw // 4) * es]
    lengths = [hw * es, hw // 4 * es, hw // 4 * es]
    if (H, W, es) == (18, 18, 1):
        assert offsets[1] == 324
    assert lengths == ph.plane_bytes("yuv420", 8 * es, W, H)
    got = ph.crc32_segments(_dev(buf), offsets, lengths)
    assert got == _want(buf, offsets, lengths)
    assert ph.picture_crc(got, lengths) == zlib.crc32(buf.tobytes())


def test_beyond_2_pow_31_bytes():
    """offsets and lengths are 64-bit: a segment that starts behind 2^31 bytes, and one that is longer than that. The buffer is
    zeros but for its ends, so the expected values come from zlib over the ends and the GF(2) restatement over the zeros."""
    head, tail = 1000, 5000
    n = 2 ** 31 + 4096 + 13
    rng = np.random.default_rng(31)
    a, b = rng.integers(0, 256, head, dtype=np.uint8), rng.integers(0, 256, tail, dtype=np.uint8)
    t = torch.zeros(n, dtype=torch.uint8, device="cuda")
    t[:head] = torch.from_numpy(a).cuda()
    t[n - tail:] = torch.from_numpy(b).cuda()
    zeros = n - head - tail
    zero_crc = crc32_np.mulmod(0xFFFFFFFF, crc32_np.xpow(8 * zeros)) ^ 0xFFFFFFFF
    whole = crc32_np.combine(crc32_np.combine(zlib.crc32(a.tobytes()), zero_crc, zeros), zlib.crc32(b.tobytes()), tail)
    behind = n - tail + 3
    got = ph.crc32_segments(t, [0, behind, 1], [n, tail - 3, n - 1])
    want = [whole, zlib.crc32(b[3:].tobytes()),
            crc32_np.combine(crc32_np.combine(zlib.crc32(a[1:].tobytes()), zero_crc, zeros), zlib.crc32(b.tobytes()), tail)]
    assert got == want, [hex(v) for v in got + want]


def test_the_wrapper_refuses_what_is_no_byte_range(random_bytes):
    t = _dev(random_bytes[:100])
    for o, n in (([0], [101]), ([-1], [4]), ([100], [1]), ([0] * 17, [1] * 17), ([], [])):
        with pytest.raises(ValueError):
            ph.crc32_segments(t, o, n)
    with pytest.raises(ValueError):
        ph.crc32_segments(t.to(torch.int16), [0], [4])
    assert ph.crc32_segments(t, [100], [0]) == [0]
