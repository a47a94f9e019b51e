"""The host side of the picture hashes, no GPU: dcvc_crc32_combine against zlib.crc32 of concatenations and,
for the lengths zlib cannot be fed cheaply, against the plain-Python GF(2) restatement (tests/crc32_np.py); the manifest
writer and reader of dcvc_amd/picture_hash.py."""
import zlib

import numpy as np
import pytest

import crc32_np
from dcvc_amd import picture_hash as ph

LEN_B = [0, 1, 2, 3, 4, 255, 256, 65535, 65536, 1000000]


@pytest.fixture(scope="module")
def data():
    return np.random.default_rng(19).integers(0, 256, 2000000, dtype=np.uint8).tobytes()


def test_the_restatement_is_zlibs_crc32(data):
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 300):
        assert crc32_np.crc32(data[:n]) == zlib.crc32(data[:n]), n
    assert crc32_np.crc32(bytes(7)) != crc32_np.crc32(bytes(8))             # the init term makes the length count
    assert crc32_np.raw(bytes(7)) == crc32_np.raw(bytes(8)) == 0
    assert crc32_np.mulmod(crc32_np.xpow(5), crc32_np.xpow(2 ** 32 - 1 - 5)) == crc32_np.ONE


@pytest.mark.parametrize("len_b", LEN_B)
@pytest.mark.parametrize("len_a", [0, 1, 777, 1000000])
def test_combine_equals_zlib_on_the_concatenation(data, len_a, len_b):
    a, b = data[:len_a], data[1000000:1000000 + len_b]
    assert ph.crc32_combine(zlib.crc32(a), zlib.crc32(b), len_b) == zlib.crc32(a + b)
    assert ph.crc32_combine(zlib.crc32(a), zlib.crc32(b), len_b) == zlib.crc32(b, zlib.crc32(a))


def test_combine_with_an_empty_b_returns_crc_a():
    for a in (0, 1, 0xDEADBEEF, 0xFFFFFFFF):
        assert ph.crc32_combine(a, 0, 0) == a


def test_combine_is_associative_over_three_parts(data):
    a, b, c = data[:1234], data[5000:5017], data[70000:70000 + 65537]
    ca, cb, cc = (zlib.crc32(x) for x in (a, b, c))
    left = ph.crc32_combine(ph.crc32_combine(ca, cb, len(b)), cc, len(c))
    right = ph.crc32_combine(ca, ph.crc32_combine(cb, cc, len(c)), len(b) + len(c))
    assert left == right == zlib.crc32(a + b + c)


@pytest.mark.parametrize("len_b", [2 ** 31 - 1, 2 ** 32 + 5, 2 ** 40], ids=["2^31-1", "2^32+5", "2^40"])
def test_combine_equals_the_restatement_at_lengths_zlib_cannot_be_fed(len_b):
    for a, b in ((0x12345678, 0x9ABCDEF0), (0xFFFFFFFF, 0), (0, 0xFFFFFFFF), (zlib.crc32(b"dcvc"), zlib.crc32(b"amd"))):
        assert ph.crc32_combine(a, b, len_b) == crc32_np.combine(a, b, len_b), (hex(a), hex(b))


def test_zero_bytes_behind_a_picture_through_two_splits():
    # crc32 of 5 MiB of zeros, 1 MiB at a time, against zlib
    z1, part = zlib.crc32(bytes(2 ** 20)), 0
    for _ in range(5):
        part = ph.crc32_combine(part, z1, 2 ** 20)
    assert part == zlib.crc32(bytes(5 * 2 ** 20)) == _zero_crc(5 * 2 ** 20)
    # crc32(A || 2^32 + 5 zero bytes), appended at once and as two parts: the arithmetic agrees with itself beyond 32 bits
    n, a = 2 ** 32 + 5, zlib.crc32(b"picture")
    whole = ph.crc32_combine(a, _zero_crc(n), n)
    halves = ph.crc32_combine(ph.crc32_combine(a, _zero_crc(n - 7), n - 7), _zero_crc(7), 7)
    assert whole == halves and _zero_crc(7) == zlib.crc32(bytes(7))


def _zero_crc(n):
    """crc32 of n zero bytes from the restatement: the raw CRC is 0, the init term and the final XOR remain"""
    return crc32_np.mulmod(0xFFFFFFFF, crc32_np.xpow(8 * n)) ^ 0xFFFFFFFF


def test_combine_refuses_what_is_no_crc_or_length():
    for bad in ((-1, 0, 1), (0, 1 << 32, 1), (0, 0, -1), (0, 0, 1 << 63)):
        with pytest.raises(ValueError):
            ph.crc32_combine(*bad)
    # the C entry point itself: a negative length gives 0 and a message
    import ctypes
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_crc32_combine", ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_longlong])
    assert f(5, 6, -1) == 0 and "negative length" in _lib.lib().dcvc_last_error().decode()


# ------------------------------------------------------------------------------------------------ manifest
def _manifest(src_type, depth, W, H, n, seed=0):
    rng = np.random.default_rng(seed)
    lens = ph.plane_bytes(src_type, depth, W, H)
    pictures = []
    for _ in range(n):
        planes = [int(v) for v in rng.integers(0, 1 << 32, len(lens), dtype=np.uint64)]
        pictures.append((ph.picture_crc(planes, lens), planes))
    return ph.Manifest(src_type, depth, W, H, pictures)


@pytest.mark.parametrize("src_type,depth,planes", [("yuv420", 8, 3), ("yuv420", 10, 3), ("yuv422", 12, 3), ("yuv444", 8, 3),
                                                   ("nv12", 10, 2), ("rgb24", 8, 1), ("png", 8, 1)])
def test_manifest_round_trip(tmp_path, src_type, depth, planes):
    m = _manifest(src_type, depth, 64, 48, 3)
    text = ph.format_manifest(m)
    lines = text.split("\n")
    assert lines[0] == "# dcvc-hash 1 crc32 %s %d 64 48" % (src_type, depth) and lines[-1] == ""
    assert [len(ln.split(" ")) for ln in lines[1:4]] == [2 + planes] * 3 and lines[4].startswith("sequence ")
    assert ph.parse_manifest(text) == m
    ph.write_manifest(str(tmp_path / "m.txt"), m)
    assert (tmp_path / "m.txt").read_bytes() == text.encode() and ph.read_manifest(str(tmp_path / "m.txt")) == m
    assert m.total_bytes == 3 * sum(ph.plane_bytes(src_type, depth, 64, 48))
    assert ph.parse_manifest(ph.format_manifest(_manifest(src_type, depth, 64, 48, 0))).pictures == []


def test_the_manifest_of_real_bytes_carries_zlibs_values():
    W, H = 18, 18
    rng = np.random.default_rng(4)
    pics = [rng.integers(0, 256, W * H * 3 // 2, dtype=np.uint8).tobytes() for _ in range(3)]
    lens = ph.plane_bytes("yuv420", 8, W, H)
    assert lens == [324, 81, 81]
    cuts = [0, 324, 405, 486]
    pictures = [(zlib.crc32(p), [zlib.crc32(p[cuts[k]:cuts[k + 1]]) for k in range(3)]) for p in pics]
    m = ph.Manifest("yuv420", 8, W, H, pictures)
    assert m.sequence_crc == zlib.crc32(b"".join(pics)) and m.total_bytes == 3 * 486
    assert ph.parse_manifest(ph.format_manifest(m)) == m           # the reader re-derives every picture from its planes


def _edit(text, line, new):
    lines = text.split("\n")
    lines[line] = new(lines[line])
    return "\n".join(lines)


MALFORMED = [
    ("empty", lambda t: ""),
    ("no newline at the end", lambda t: t[:-1]),
    ("another magic", lambda t: _edit(t, 0, lambda s: s.replace("dcvc-hash", "dcvc-hush"))),
    ("version 2", lambda t: _edit(t, 0, lambda s: s.replace("dcvc-hash 1", "dcvc-hash 2"))),
    ("another algorithm", lambda t: _edit(t, 0, lambda s: s.replace("crc32", "md5"))),
    ("unknown source type", lambda t: _edit(t, 0, lambda s: s.replace("yuv420", "yuv411"))),
    ("bit depth 7", lambda t: _edit(t, 0, lambda s: s.replace(" 8 64", " 7 64"))),
    ("a header field missing", lambda t: _edit(t, 0, lambda s: s.rsplit(" ", 1)[0])),
    ("negative width", lambda t: _edit(t, 0, lambda s: s.replace(" 64 48", " -64 48"))),
    ("upper-case hex", lambda t: _edit(t, 1, lambda s: s.upper())),
    ("seven hex digits", lambda t: _edit(t, 1, lambda s: s[:-1])),
    ("a plane missing", lambda t: _edit(t, 2, lambda s: s.rsplit(" ", 1)[0])),
    ("a plane too many", lambda t: _edit(t, 2, lambda s: s + " 00000000")),
    ("two spaces", lambda t: _edit(t, 2, lambda s: s.replace(" ", "  ", 1))),
    ("pictures out of order", lambda t: "\n".join([t.split("\n")[i] for i in (0, 2, 1, 3, 4, 5)])),
    ("a picture line removed", lambda t: "\n".join([t.split("\n")[i] for i in (0, 1, 3, 4, 5)])),
    ("an index that is no number", lambda t: _edit(t, 1, lambda s: "x" + s[1:])),
    ("no sequence line", lambda t: "\n".join(t.split("\n")[:4]) + "\n"),
    ("sequence line in the middle", lambda t: "\n".join([t.split("\n")[i] for i in (0, 1, 4, 2, 3, 5)])),
    ("another byte count", lambda t: _edit(t, 4, lambda s: s + "0")),
    ("another sequence CRC", lambda t: _edit(t, 4, lambda s: s[:9] + ("0" if s[9] != "0" else "1") + s[10:])),
    ("a picture CRC that is not its planes'", lambda t: _edit(t, 2, lambda s: s[:2] + ("0" if s[2] != "0" else "1") + s[3:])),
    ("trailing text", lambda t: t + "more\n"),
]


@pytest.mark.parametrize("why,damage", MALFORMED, ids=[m[0].replace(" ", "_") for m in MALFORMED])
def test_malformed_manifests_are_refused(why, damage):
    good = ph.format_manifest(_manifest("yuv420", 8, 64, 48, 3, seed=1))
    assert ph.parse_manifest(good).pictures
    with pytest.raises(ValueError):
        ph.parse_manifest(damage(good))


def test_manifest_refuses_rgb_at_another_depth_and_unknown_types():
    with pytest.raises(ValueError):
        ph.plane_bytes("yuv411", 8, 64, 48)
    with pytest.raises(ValueError):
        ph.parse_manifest("# dcvc-hash 1 crc32 rgb24 10 64 48\nsequence 00000000 0\n")
    assert ph.parse_manifest("# dcvc-hash 1 crc32 rgb24 8 64 48\nsequence 00000000 0\n").total_bytes == 0
