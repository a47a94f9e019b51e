"""The PNG reader and writer of the library (include/dcvc_amd_image.h, through dcvc_amd.rgb) without a GPU, on files this test
builds itself with struct + zlib: every row filter, several IDAT chunks, colour types 0 / 2 / 3 / 4 / 6 expanded as PIL's
convert('RGB') does (video_reader.py:10-45), the refusal of what the reader does not decode or what is damaged, and the
writer's pixels read back. PIL, where it imports, reads the same pixels."""
import os
import struct
import zlib

import numpy as np
import pytest

from dcvc_amd import _lib, rgb

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def _filter(row, prev, f, bpp):
    row, prev = row.astype(np.int64), prev.astype(np.int64)
    out = np.zeros_like(row)
    for i in range(len(row)):
        a = row[i - bpp] if i >= bpp else 0
        c = prev[i - bpp] if i >= bpp else 0
        pred = [0, a, prev[i], (a + prev[i]) // 2, _paeth(a, prev[i], c)][f]
        out[i] = (row[i] - pred) & 255
    return out.astype(np.uint8)


def make_png(samples, colour, filters=(0,), idats=1, plte=None, depth=8, interlace=0, extra=b""):
    """samples: [H, W * channels] u8 rows; filters cycle over the rows"""
    H, stride = samples.shape
    W = stride // CHANNELS[colour]
    raw = b""
    prev = np.zeros(stride, np.uint8)
    for y in range(H):
        f = filters[y % len(filters)]
        raw += bytes([f]) + _filter(samples[y], prev, f, CHANNELS[colour]).tobytes()
        prev = samples[y]
    z = zlib.compress(raw, 9)
    cuts = np.linspace(0, len(z), idats + 1).astype(int)
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, interlace))
    data += _chunk(b"tEXt", b"Comment\x00ancillary chunks are skipped") + extra
    if plte is not None:
        data += _chunk(b"PLTE", plte.tobytes())
    for i in range(idats):
        data += _chunk(b"IDAT", z[cuts[i]:cuts[i + 1]])
    return data + _chunk(b"IEND", b"")


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _rgb_of(samples, colour, plte=None):
    """convert('RGB') of the samples"""
    H = samples.shape[0]
    s = samples.reshape(H, -1, CHANNELS[colour])
    if colour in (0, 4):
        return np.repeat(s[..., :1], 3, axis=2)
    if colour == 3:
        return plte[s[..., 0]]
    return s[..., :3]


@pytest.mark.parametrize("colour", [0, 2, 3, 4, 6])
def test_colour_types_filters_and_idats(tmp_path, colour):
    rng = np.random.default_rng(colour)
    H, W = 13, 29
    plte = rng.integers(0, 256, (200, 3), dtype=np.uint8) if colour == 3 else None
    samples = rng.integers(0, 200 if colour == 3 else 256, (H, W * CHANNELS[colour]), dtype=np.uint8)
    samples[1] = samples[0]            # repeated rows and runs make Up / Average / Paeth predict something
    want = _rgb_of(samples, colour, plte)
    for filters, idats in [((0, 1, 2, 3, 4), 1), ((4, 3, 2, 1, 0), 3), ((2,), 5)]:
        path = _write(tmp_path, "c%d.png" % colour, make_png(samples, colour, filters, idats, plte))
        assert rgb.png_info(path) == (W, H)
        got = rgb.read_png(path)
        assert got.shape == (H, W, 3) and np.array_equal(got, want), (filters, idats)
        pil = _pil()
        if pil is not None:
            assert np.array_equal(np.asarray(pil.open(path).convert("RGB")), got)


def _pil():
    try:
        from PIL import Image
    except ImportError:
        return None
    return Image


def _refused(tmp_path, data, msg):
    path = _write(tmp_path, "bad.png", data)
    with pytest.raises(_lib.DcvcError, match=msg):
        rgb.read_png(path)


def test_refuses_what_it_does_not_decode(tmp_path):
    s = np.zeros((4, 8), np.uint8)
    _refused(tmp_path, make_png(np.zeros((4, 16), np.uint8), 0, depth=16), "bit depth 16")
    _refused(tmp_path, make_png(np.zeros((4, 4), np.uint8), 0, depth=4), "bit depth 4")
    _refused(tmp_path, make_png(s, 0, interlace=1), "interlaced")
    _refused(tmp_path, make_png(s, 0).replace(b"IHDR", b"IHDX", 1), "IHDR")
    _refused(tmp_path, b"GIF89a" + bytes(40), "not a PNG")
    _refused(tmp_path, make_png(np.zeros((4, 4), np.uint8), 3), "PLTE")            # palette picture without a palette
    _refused(tmp_path, make_png(np.full((4, 4), 9, np.uint8), 3, plte=np.zeros((4, 3), np.uint8)), "palette index")
    with pytest.raises(_lib.DcvcError, match="cannot open"):
        rgb.read_png(str(tmp_path / "missing.png"))


def test_refuses_damaged_files(tmp_path):
    rng = np.random.default_rng(9)
    data = make_png(rng.integers(0, 256, (16, 48), dtype=np.uint8), 2, (1, 4), idats=2)
    for cut in [7, 20, 40, len(data) // 2, len(data) - 13, len(data) - 1]:
        _refused(tmp_path, data[:cut], "truncated|not a PNG")
    at = data.index(b"IDAT") + 10
    _refused(tmp_path, data[:at] + bytes([data[at] ^ 1]) + data[at + 1:], "CRC mismatch in chunk IDAT")
    at = data.index(b"IHDR") + 6
    _refused(tmp_path, data[:at] + bytes([data[at] ^ 4]) + data[at + 1:], "CRC mismatch in IHDR")
    # a consistent file whose deflate stream is short or corrupt, or whose row names an unknown filter
    short = make_png(rng.integers(0, 256, (16, 48), dtype=np.uint8), 2)
    z_at = short.index(b"IDAT")
    n = struct.unpack(">I", short[z_at - 4:z_at])[0]
    body = short[z_at + 4:z_at + 4 + n]
    end = short[z_at + 8 + n:]
    _refused(tmp_path, short[:z_at - 4] + _chunk(b"IDAT", zlib.compress(zlib.decompress(body)[:-30])) + end, "truncated image data")
    _refused(tmp_path, short[:z_at - 4] + _chunk(b"IDAT", body[:2] + bytes(len(body) - 2)) + end, "corrupt image data|truncated")
    raw = bytearray(zlib.decompress(body))
    raw[49] = 7                                    # the filter byte of row 1
    _refused(tmp_path, short[:z_at - 4] + _chunk(b"IDAT", zlib.compress(bytes(raw))) + end, "unknown row filter 7")


def test_write_then_read_gives_equal_pixels(tmp_path):
    rng = np.random.default_rng(3)
    for H, W in [(1, 1), (2, 6), (37, 53), (96, 128)]:
        pix = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        path = str(tmp_path / "w.png")
        rgb.write_png(path, pix)
        assert np.array_equal(rgb.read_png(path), pix)
        pil = _pil()
        if pil is not None:
            assert np.array_equal(np.asarray(pil.open(path).convert("RGB")), pix)
            pil.fromarray(pix).save(str(tmp_path / "p.png"))                   # the reference's writer
            assert np.array_equal(rgb.read_png(str(tmp_path / "p.png")), pix)
    with pytest.raises(ValueError):
        rgb.write_png(str(tmp_path / "x.png"), np.zeros((4, 4), np.uint8))


def test_sequence_naming_rules(tmp_path):
    pix = [np.full((4, 6, 3), i, np.uint8) for i in range(3)]
    for pad, d in [(1, tmp_path / "one"), (5, tmp_path / "five")]:
        d.mkdir()
        for i, p in enumerate(pix):
            rgb.write_png(str(d / ("im%s.png" % str(i + 1).zfill(pad))), p)
        assert rgb.png_naming(str(d)) == pad
        got = list(rgb.png_sequence(str(d)))
        assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, pix))
    other = tmp_path / "other"
    other.mkdir()
    rgb.write_png(str(other / "frame_001.png"), pix[0])
    with pytest.raises(ValueError, match="naming"):
        list(rgb.png_sequence(str(other)))
