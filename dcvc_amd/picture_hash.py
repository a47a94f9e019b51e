"""Picture hashes (no reference counterpart): CRC-32 of decoded pictures on the GPU and the manifest of
``dcvc --hash-log`` / ``--verify-hash``.

``crc32_segments`` and ``crc32_combine`` are thin wrappers over the C-ABI entry points ``dcvc_crc32_segments`` and
``dcvc_crc32_combine`` (include/dcvc_amd_ops.h); the kernel runs on ``torch.cuda.current_stream()``. The values are zlib's:
``crc32_segments(t, [0], [t.numel()]) == [zlib.crc32(t.cpu().numpy().tobytes())]``.

The manifest is text, one line per picture::

    # dcvc-hash 1 crc32 <src_type> <bit_depth> <width> <height>
    <idx> <crc8hex> <plane crc8hex> ...
    sequence <crc8hex> <total bytes>

A picture's CRC is over its bytes in raw file layout (what ``-o`` writes), the plane CRCs are over Y, U, V (planar types), Y
and the interleaved chroma (nv12) or the packed pixels (rgb24, png; rgb48 at 9..16 bits and png16 at 16: little-endian u16
samples, 6 H W bytes); ``sequence`` is the CRC of all pictures back to back.
"""
import ctypes
import re

from . import _lib

_vp, _ci, _ll, _u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint32
_fns = {}
_SIGS = {
    "dcvc_crc32_segments": (_ci, [_vp, ctypes.POINTER(_ll), ctypes.POINTER(_ll), _ci, _vp, _vp]),
    "dcvc_crc32_combine": (_u32, [_u32, _u32, _ll]),
}
MAX_SEGMENTS = 16
SRC_TYPES = ("yuv420", "yuv422", "yuv444", "nv12", "rgb24", "png", "rgb48", "png16")
_HEX = re.compile(r"^[0-9a-f]{8}$")
_DEC = re.compile(r"^(0|[1-9][0-9]*)$")


def _fn(name):
    if name not in _fns:
        _fns[name] = _lib.fn(name, *_SIGS[name])
    return _fns[name]


def crc32_segments(t, offsets, lengths):
    """t: a contiguous uint8 CUDA tensor. offsets, lengths: up to 16 byte ranges of it, anywhere, in any order. Returns
    [zlib.crc32 of each range]; reading them waits for the stream."""
    import torch
    if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
        raise ValueError("crc32_segments: a contiguous uint8 CUDA tensor expected, got %s %s" % (t.dtype, tuple(t.shape)))
    offsets, lengths = [int(o) for o in offsets], [int(n) for n in lengths]
    n = len(offsets)
    if len(lengths) != n or not 1 <= n <= MAX_SEGMENTS:
        raise ValueError("crc32_segments: 1..%d offsets and as many lengths expected" % MAX_SEGMENTS)
    for o, ln in zip(offsets, lengths):
        if o < 0 or ln < 0 or o + ln > t.numel():
            raise ValueError("crc32_segments: segment (%d, %d) lies outside the %d bytes of the tensor" % (o, ln, t.numel()))
    out = torch.empty(n, dtype=torch.int32, device=t.device)
    # an empty tensor has no storage: the call still needs a pointer, which no launch reads
    base = t.data_ptr() if t.numel() else out.data_ptr()
    _lib.check(_fn("dcvc_crc32_segments")(_vp(base), (_ll * n)(*offsets), (_ll * n)(*lengths), n, _vp(out.data_ptr()),
                                          _vp(torch.cuda.current_stream(t.device).cuda_stream)))
    return [int(v) & 0xFFFFFFFF for v in out.tolist()]


def crc32_combine(a, b, len_b):
    """crc32(A || B) from a = crc32(A), b = crc32(B) and len_b = len(B); host arithmetic, no GPU"""
    a, b, len_b = int(a), int(b), int(len_b)
    if not (0 <= a <= 0xFFFFFFFF and 0 <= b <= 0xFFFFFFFF):
        raise ValueError("crc32_combine: CRCs are 32-bit values")
    if len_b < 0 or len_b >= 1 << 63:
        raise ValueError("crc32_combine: len_b must be in 0..2^63 - 1")
    return int(_fn("dcvc_crc32_combine")(a, b, len_b))


def plane_bytes(src_type, bit_depth, width, height):
    """the bytes of each hashed plane of one picture, in file order"""
    if src_type not in SRC_TYPES:
        raise ValueError("unknown source type %r" % (src_type,))
    hw = width * height
    if src_type in ("rgb24", "png"):
        return [3 * hw]
    if src_type in ("rgb48", "png16"):
        return [6 * hw]
    es = 2 if bit_depth > 8 else 1
    if src_type == "nv12":
        return [hw * es, hw // 2 * es]
    c = {"yuv420": hw // 4, "yuv422": hw // 2, "yuv444": hw}[src_type]
    return [hw * es, c * es, c * es]


class Manifest:
    """src_type, bit_depth, width, height; pictures: [(crc, [plane crc, ...])] in decoding order; sequence_crc, total_bytes"""

    def __init__(self, src_type, bit_depth, width, height, pictures=(), sequence_crc=None, total_bytes=None):
        self.src_type, self.bit_depth, self.width, self.height = src_type, int(bit_depth), int(width), int(height)
        self.pictures = [(int(c), [int(p) for p in planes]) for c, planes in pictures]
        lens = plane_bytes(src_type, self.bit_depth, self.width, self.height)
        if sequence_crc is None:
            sequence_crc = 0
            for c, _ in self.pictures:
                sequence_crc = crc32_combine(sequence_crc, c, sum(lens))
        self.sequence_crc = int(sequence_crc)
        self.total_bytes = len(self.pictures) * sum(lens) if total_bytes is None else int(total_bytes)

    def __eq__(self, other):
        return isinstance(other, Manifest) and vars(self) == vars(other)

    def __repr__(self):
        return "Manifest(%s %d-bit %dx%d, %d pictures, sequence %08x)" % (
            self.src_type, self.bit_depth, self.width, self.height, len(self.pictures), self.sequence_crc)


def picture_crc(plane_crcs, lens):
    """a picture's CRC from its planes' CRCs and lengths"""
    crc = 0
    for c, n in zip(plane_crcs, lens):
        crc = crc32_combine(crc, c, n)
    return crc


def format_manifest(m):
    """the text dcvc --hash-log writes, byte for byte"""
    lines = ["# dcvc-hash 1 crc32 %s %d %d %d" % (m.src_type, m.bit_depth, m.width, m.height)]
    for i, (crc, planes) in enumerate(m.pictures):
        lines.append(" ".join(["%d" % i, "%08x" % crc] + ["%08x" % p for p in planes]))
    lines.append("sequence %08x %d" % (m.sequence_crc, m.total_bytes))
    return "\n".join(lines) + "\n"


def parse_manifest(text):
    """the Manifest of a --hash-log text. ValueError for anything the format does not allow: another header, version or
    algorithm, a picture line out of order or with the wrong number of planes, hex that is not 8 lowercase digits, a missing
    or misplaced sequence line, a byte count that does not fit the pictures, or CRCs that are not the combination of their
    parts."""
    if not text.endswith("\n"):
        raise ValueError("manifest: the last line is not terminated")
    lines = text[:-1].split("\n")
    head = lines[0].split(" ")
    if len(head) != 8 or head[:4] != ["#", "dcvc-hash", "1", "crc32"]:
        raise ValueError("manifest: no '# dcvc-hash 1 crc32 <src_type> <bit_depth> <width> <height>' header: %r" % lines[0])
    if head[4] not in SRC_TYPES or not all(_DEC.match(v) for v in head[5:]):
        raise ValueError("manifest: bad source type or numbers in the header: %r" % lines[0])
    depth, width, height = (int(v) for v in head[5:])
    if not 8 <= depth <= 16 or width < 1 or height < 1 or (head[4] in ("rgb24", "png") and depth != 8):
        raise ValueError("manifest: bad bit depth or size in the header: %r" % lines[0])
    if (head[4] == "rgb48" and depth < 9) or (head[4] == "png16" and depth != 16):
        raise ValueError("manifest: bad bit depth or size in the header: %r" % lines[0])
    lens = plane_bytes(head[4], depth, width, height)
    if len(lines) < 2 or not lines[-1].startswith("sequence "):
        raise ValueError("manifest: no sequence line at the end")
    pictures = []
    for i, line in enumerate(lines[1:-1]):
        tok = line.split(" ")
        if len(tok) != 2 + len(lens) or tok[0] != "%d" % i or not all(_HEX.match(v) for v in tok[1:]):
            raise ValueError("manifest: bad line for picture %d: %r" % (i, line))
        crc, planes = int(tok[1], 16), [int(v, 16) for v in tok[2:]]
        if picture_crc(planes, lens) != crc:
            raise ValueError("manifest: the CRC of picture %d is not the combination of its planes' CRCs" % i)
        pictures.append((crc, planes))
    tok = lines[-1].split(" ")
    if len(tok) != 3 or not _HEX.match(tok[1]) or not _DEC.match(tok[2]):
        raise ValueError("manifest: bad sequence line: %r" % lines[-1])
    m = Manifest(head[4], depth, width, height, pictures)
    if int(tok[2]) != m.total_bytes or int(tok[1], 16) != m.sequence_crc:
        raise ValueError("manifest: the sequence line does not fit the %d pictures" % len(pictures))
    return m


def write_manifest(path, m):
    with open(path, "w", newline="\n") as f:
        f.write(format_manifest(m))


def read_manifest(path):
    with open(path, "r", newline="") as f:
        return parse_manifest(f.read())


__all__ = ["crc32_segments", "crc32_combine", "plane_bytes", "picture_crc", "Manifest", "format_manifest", "parse_manifest",
           "write_manifest", "read_manifest", "MAX_SEGMENTS", "SRC_TYPES"]
