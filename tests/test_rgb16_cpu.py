"""9..16-bit RGB without a GPU: the numpy restatement (tests/rgb16_np.py) of dcvc_rgb16_to_x_cs / dcvc_x_to_rgb16_cs against the
matrix in closed form in float64, the argument checks of the two entry points (which refuse before touching the device), the
16-bit PNG reader and writer against files built by hand, the hash manifest's rgb48 / png16 types and the dcvc tool's
flag-only refusals."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import colour_np
import rgb16_np

vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
CASES = [("bt709", "full", 8), ("bt601", "limited", 8), ("bt2020", "limited", 10), ("bt601", "full", 8), ("bt709", "limited", 16)]


def _colours(depth, n=1 << 16, seed=3):
    """[3, 1, n + ramp] u16: random colours, the grey ramp of every code (up to 4096 of them), black and white"""
    rng = np.random.default_rng(seed + depth)
    m = rgb16_np.max_val(depth)
    ramp = np.unique(np.linspace(0, m, min(m + 1, 4096)).round().astype(np.uint16))
    c = np.concatenate([rng.integers(0, m + 1, size=(3, n), dtype=np.uint16), np.stack([ramp] * 3),
                        np.array([[0, m]] * 3, dtype=np.uint16)], axis=1)
    return c[:, None, :]


@pytest.mark.parametrize("depth", [10, 12, 16])
@pytest.mark.parametrize("matrix,range_,yuv_depth", CASES)
def test_to_x_sits_on_the_closed_form(depth, matrix, range_, yuv_depth):
    """|x + 0.5 - exact| <= 2^-12 + 2^-13 + 2^-20. The roundings between the sample and x: fp16(clamp(.)) of a value in [0, 1]
    is off by at most half an ulp of [0.5, 1), 2^-12; fp32(that) - 0.5 is exact in fp32 and its fp16 rounding is exact for a
    first value in [0.25, 1] and off by at most 2^-13 (half an ulp of [0.25, 0.5]) below that; in front of the two, at most
    12 fp32 roundings (the division, 3 products and 2 sums of y, the difference, the product with the reciprocal, the
    limited-range multiply and add, and the roundings of the constants themselves), each at most 2^-24 relative on values of
    magnitude <= 1 with gains <= 1: 12 * 2^-24 < 2^-20."""
    c = _colours(depth)
    x = rgb16_np.rgb16_to_x(c, depth, matrix, range_, yuv_depth)
    got = x.astype(np.float64) + 0.5
    err = max(float(np.abs(got[..., k] - e).max()) for k, e in enumerate(rgb16_np.exact_ycc(c, depth, matrix, range_, yuv_depth)))
    print("max |x - exact| = %.6g" % err)
    assert err <= 2.0 ** -12 + 2.0 ** -13 + 2.0 ** -20


@pytest.mark.parametrize("depth", [10, 12, 16])
@pytest.mark.parametrize("matrix,range_,yuv_depth", CASES)
def test_from_x_sits_on_the_closed_form(depth, matrix, range_, yuv_depth):
    """|dist32 / max_val - exact| <= (A + 1) 2^-12 + 2^-18 against the float64 inverse of the same fp16 x_hat. fp16(x_hat + 0.5)
    is off by at most 2^-12 (half an ulp of [0.5, 1)) in each of Y, Cb, Cr; the matrix carries that into r, g, b with the gain
    A = sy + sc max(2 - 2 Kr, 2 - 2 Kb, (Kr (2 - 2 Kr) + Kb (2 - 2 Kb)) / Kg), sy = iy and sc = ic in limited range, 1 in
    full range; fp16(clamp(., 0, 1)) adds at most 2^-12 (the clamp is 1-Lipschitz); the fp32 steps (11 operations up to g, 5 rounded
    constants and the product with max_val: 17 roundings at 2^-24 relative on values of magnitude <= 2.2 with a downstream
    gain <= 1 / Kg <= 1.71) stay below 17 * 2.2 * 1.71 * 2^-24 < 2^-18. The written
    sample is within 0.5 of its plane."""
    kr, kg, kb = colour_np.MATRICES[matrix]
    gain = max(2 - 2 * kr, 2 - 2 * kb, (kr * (2 - 2 * kr) + kb * (2 - 2 * kb)) / kg)
    if range_ == "limited":
        _, _, _, _, iy, ic = (float(v) for v in colour_np.levels(yuv_depth))
        A = iy + ic * gain
    else:
        A = 1 + gain
    m = rgb16_np.max_val(depth)
    rng = np.random.default_rng(7 + depth)
    x_own = rgb16_np.rgb16_to_x(_colours(depth), depth, matrix, range_, yuv_depth)[0]
    x_any = (rng.random((1 << 16, 3)) - 0.5).astype(np.float16)
    x_hat = np.concatenate([x_own, x_any])[None]
    dist, out = rgb16_np.x_to_rgb16(x_hat, 1, x_hat.shape[1], depth, matrix, range_, yuv_depth)
    err = max(float(np.abs(dist[k].astype(np.float64) - e).max()) for k, e in enumerate(rgb16_np.exact_rgb(x_hat, depth, matrix, range_, yuv_depth)))
    print("max |dist32 - exact| = %.6g codes (bound %.6g)" % (err, ((A + 1) * 2.0 ** -12 + 2.0 ** -18) * m))
    assert err <= ((A + 1) * 2.0 ** -12 + 2.0 ** -18) * m
    assert dist.dtype == np.float32 and out.dtype == np.uint16
    assert float(dist.min()) >= 0 and float(dist.max()) <= m
    assert float(np.abs(out.transpose(2, 0, 1).astype(np.float64) - dist).max()) <= 0.5


def test_special_values_and_the_ends_of_the_scale():
    for depth in (10, 16):
        m = rgb16_np.max_val(depth)
        # black and white reach the ends of x and come back exactly
        c = np.array([[[0, m]]] * 3, dtype=np.uint16)
        x = rgb16_np.rgb16_to_x(c, depth)
        assert x[0, 0].tolist() == [-0.5, 0.0, 0.0] and x[0, 1].tolist() == [0.5, 0.0, 0.0]
        _, back = rgb16_np.x_to_rgb16(x, 1, 2, depth)
        assert np.array_equal(back.transpose(2, 0, 1), c)
        # NaN passes through the clamps into the plane and is written as 0; an infinite luma clamps in r and b and is
        # inf - inf = NaN in g; a finite value outside the range clamps
        x_hat = np.zeros((1, 4, 3), np.float16)
        x_hat[0, 0, 0], x_hat[0, 1, 0], x_hat[0, 2, 0], x_hat[0, 3] = np.nan, np.inf, -np.inf, 3.0
        dist, out = rgb16_np.x_to_rgb16(x_hat, 1, 4, depth)
        assert np.isnan(dist[:, 0, 0]).all() and (out[0, 0] == 0).all()
        assert out[0, 1].tolist() == [m, 0, m] and np.isnan(dist[1, 0, 1]) and (out[0, 2] == 0).all() and (out[0, 3] == m).all()
    # samples above max_val are not masked: they clamp at the top of x like any value above 1
    x = rgb16_np.rgb16_to_x(np.full((3, 1, 1), 4095, np.uint16), 10)
    assert x[0, 0].tolist() == [0.5, 0.0, 0.0]


def test_the_unit_value_is_a_true_division():
    """fp32(v) / fp32(max_val) and v * fp32(1 / max_val) differ for some v: the restatement (and the kernel) take the first"""
    v = np.arange(1024, dtype=np.uint16)
    a = v.astype(np.float32) / np.float32(1023)
    b = v.astype(np.float32) * (np.float32(1) / np.float32(1023))
    assert (a != b).any()
    assert np.array_equal(a, (v.astype(np.float64) / 1023).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ ABI
def _err():
    from dcvc_amd import _lib
    return _lib.lib().dcvc_last_error().decode()


def test_abi_refuses_bad_arguments():
    from dcvc_amd import _lib
    to_x = _lib.fn("dcvc_rgb16_to_x_cs", ci, [vp, ll, ll, ll, ci, ci, ci, vp, ci, vp, ci, ci, ci, vp])
    to_rgb = _lib.fn("dcvc_x_to_rgb16_cs", ci, [vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, vp])
    p = vp(4096)     # never dereferenced: every call below is refused by the argument checks

    def x_args(src=p, rs=384, ps=3, cs=1, depth=10, H=64, W=128, x=p, ldx=3, planar=None, colour=(1, 0, 8)):
        return (src, rs, ps, cs, depth, H, W, x, ldx, planar) + tuple(colour) + (None,)

    def rgb_args(x=p, row=128, H=64, W=128, depth=10, dist=p, out=p, colour=(1, 0, 8)):
        return (x, row, H, W, depth, dist, out) + tuple(colour) + (None,)

    for depth in (8, 7, 0, -1, 17, 32):
        assert to_x(*x_args(depth=depth)) == -1 and "9..16" in _err() and "rgb16_to_x_cs" in _err(), (depth, _err())
        assert to_rgb(*rgb_args(depth=depth)) == -1 and "9..16" in _err() and "x_to_rgb16_cs" in _err(), (depth, _err())
    assert to_x(*x_args(x=None, planar=None)) == -1 and "neither" in _err() and "rgb16_to_x_cs" in _err(), _err()
    assert to_rgb(*rgb_args(dist=None, out=None)) == -1 and "neither" in _err() and "x_to_rgb16_cs" in _err(), _err()
    bad_colour = [((-1, 0, 8), "matrix"), ((3, 0, 8), "matrix"), ((1, -1, 8), "range"), ((1, 2, 8), "range"),
                  ((1, 1, 7), "8..16"), ((1, 1, 17), "8..16"), ((0, 0, 7), "8..16")]
    for colour, msg in bad_colour:
        assert to_x(*x_args(colour=colour)) == -1 and msg in _err() and "rgb16_to_x_cs" in _err(), (colour, _err())
        assert to_rgb(*rgb_args(colour=colour)) == -1 and msg in _err() and "x_to_rgb16_cs" in _err(), (colour, _err())
    bad_strides = [(dict(rs=383), "too small"), (dict(ps=2), "too small"), (dict(rs=128, ps=1, cs=128 * 63), "too small"),
                   (dict(cs=0), "positive"), (dict(rs=-384), "positive"), (dict(ps=0), "positive")]
    for kw, msg in bad_strides:
        assert to_x(*x_args(**kw)) == -1 and msg in _err() and "rgb16_to_x_cs" in _err(), (kw, _err())
    assert to_x(*x_args(ldx=2)) == -1 and ">= 3" in _err() and "rgb16_to_x_cs" in _err(), _err()
    assert to_rgb(*rgb_args(row=127)) == -1 and "shorter" in _err() and "x_to_rgb16_cs" in _err(), _err()
    for kw in (dict(H=63), dict(W=127), dict(H=0)):
        assert to_x(*x_args(**kw)) == -1 and "even" in _err() and "rgb16_to_x_cs" in _err(), (kw, _err())
        assert to_rgb(*rgb_args(**kw)) == -1 and "even" in _err() and "x_to_rgb16_cs" in _err(), (kw, _err())
    assert to_x(*x_args(src=None)) == -1 and "source" in _err(), _err()
    assert to_rgb(*rgb_args(x=None)) == -1 and "x_hat" in _err(), _err()


def test_python_wrappers_refuse_unknown_names():
    from dcvc_amd import rgb
    with pytest.raises(ValueError, match="unknown matrix"):
        rgb.rgb16_to_x(None, 10, matrix="bt470")
    with pytest.raises(ValueError, match="unknown range"):
        rgb.x_to_rgb16(None, 2, 2, 10, range="tv")


# ------------------------------------------------------------------------------------------------------------------ PNG
def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def _filter_row(f, cur, prev, bpp):
    out = bytearray(len(cur))
    for i in range(len(cur)):
        a = cur[i - bpp] if i >= bpp else 0
        b = prev[i]
        c = prev[i - bpp] if i >= bpp else 0
        pred = (0, a, b, (a + b) // 2, _paeth(a, b, c))[f]
        out[i] = (cur[i] - pred) & 255
    return bytes(out)


def _png(samples, colour, depth=16, filters=(0,), idats=1, interlace=0, extra=b""):
    """a PNG file of samples [H, W, channels] (u16 at depth 16, u8 at depth 8), row r filtered with filters[r % len]"""
    H, W, ch = samples.shape
    assert ch == {0: 1, 2: 3, 4: 2, 6: 4}[colour]
    rows = [samples[r].astype(">u2" if depth == 16 else np.uint8).tobytes() for r in range(H)]
    bpp = ch * depth // 8
    raw, prev = b"", bytes(len(rows[0]))
    for r, row in enumerate(rows):
        f = filters[r % len(filters)]
        raw += bytes([f]) + _filter_row(f, row, prev, bpp)
        prev = row
    z = zlib.compress(raw, 6)
    cut = [len(z) * k // idats for k in range(idats + 1)]
    body = b"".join(_chunk(b"IDAT", z[cut[k]:cut[k + 1]]) for k in range(idats))
    ihdr = struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, interlace)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + extra + body + _chunk(b"IEND", b"")


def _samples(H, W, ch, seed=1):
    s = np.random.default_rng(seed).integers(0, 65536, size=(H, W, ch), dtype=np.uint16)
    s[0, 0], s[-1, -1] = 0, 65535
    return s


def _as_rgb(s, colour):
    return np.repeat(s[..., :1], 3, axis=2) if colour in (0, 4) else np.ascontiguousarray(s[..., :3])


def test_png16_write_read_round_trip(tmp_path):
    from dcvc_amd import rgb
    for H, W in ((5, 7), (1, 1), (16, 33)):
        px = _samples(H, W, 3, seed=H)
        path = str(tmp_path / ("rt%dx%d.png" % (W, H)))
        rgb.write_png16(path, px)
        assert rgb.png_info2(path) == (W, H, 16)
        got = rgb.read_png16(path)
        assert got.dtype == np.uint16 and np.array_equal(got, px)
        # the file is what the format says: colour type 2, depth 16, big-endian samples behind filter 1
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
        assert struct.unpack(">IIBBBBB", data[16:29]) == (W, H, 16, 2, 0, 0, 0)
        n = struct.unpack(">I", data[33:37])[0]
        assert data[37:41] == b"IDAT"
        raw = zlib.decompress(data[41:41 + n])
        assert len(raw) == H * (1 + 6 * W) and all(raw[r * (1 + 6 * W)] == 1 for r in range(H))
        assert raw[1:7] == px[0, 0].astype(">u2").tobytes()


@pytest.mark.parametrize("colour", [0, 2, 4, 6])
@pytest.mark.parametrize("f", [0, 1, 2, 3, 4])
def test_png16_reads_every_filter_and_colour_type(tmp_path, colour, f):
    from dcvc_amd import rgb
    s = _samples(6, 9, {0: 1, 2: 3, 4: 2, 6: 4}[colour], seed=10 * colour + f)
    path = str(tmp_path / "f.png")
    with open(path, "wb") as fh:
        fh.write(_png(s, colour, filters=(f,)))
    assert rgb.png_info2(path) == (9, 6, 16)
    assert np.array_equal(rgb.read_png16(path), _as_rgb(s, colour))


def test_png16_mixed_filters_two_idats_and_ancillary_chunks(tmp_path):
    from dcvc_amd import rgb
    s = _samples(10, 12, 3, seed=77)
    path = str(tmp_path / "m.png")
    sbit = _chunk(b"sBIT", bytes([10, 10, 10]))            # ignored: a 16-bit PNG is always depth 16
    with open(path, "wb") as fh:
        fh.write(_png(s, 2, filters=(4, 3, 2, 1, 0), idats=2, extra=sbit))
    assert open(path, "rb").read().count(b"IDAT") == 2
    assert np.array_equal(rgb.read_png16(path), s)
    assert rgb.png_info2(path) == (12, 10, 16)


def test_png16_refuses_what_it_does_not_decode(tmp_path):
    from dcvc_amd import _lib, rgb
    s = _samples(4, 6, 3)
    good = _png(s, 2, filters=(1,))
    path = str(tmp_path / "x.png")

    def put(data):
        with open(path, "wb") as fh:
            fh.write(data)

    # a bad CRC in the image data
    at = good.index(b"IDAT") + 6
    put(good[:at] + bytes([good[at] ^ 1]) + good[at + 1:])
    with pytest.raises(_lib.DcvcError, match="CRC mismatch in chunk IDAT"):
        rgb.read_png16(path)
    # interlaced
    put(_png(s, 2, interlace=1))
    with pytest.raises(_lib.DcvcError, match="interlaced"):
        rgb.read_png16(path)
    # an 8-bit file: info2 reports it, the 16-bit reader refuses it
    put(_png((s >> 8).astype(np.uint8), 2, depth=8))
    assert rgb.png_info2(path) == (6, 4, 8)
    out = np.empty((4, 6, 3), np.uint16)
    w, h = ci(), ci()
    read16 = _lib.fn("dcvc_png_read_rgb16", ci, [ctypes.c_char_p, vp, ctypes.c_size_t, ctypes.POINTER(ci), ctypes.POINTER(ci)])
    assert read16(os.fsencode(path), vp(out.ctypes.data), out.nbytes, ctypes.byref(w), ctypes.byref(h)) == -1
    assert "bit depth 8" in _err() and "16-bit PNG only" in _err(), _err()
    assert np.array_equal(rgb.read_png(path), (s >> 8).astype(np.uint8))
    # an unknown row filter, truncated data, a buffer that is too small
    raw = b"".join(bytes([5]) + s[r].astype(">u2").tobytes() for r in range(4))
    ihdr = struct.pack(">IIBBBBB", 6, 4, 16, 2, 0, 0, 0)
    put(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw)) + _chunk(b"IEND", b""))
    with pytest.raises(_lib.DcvcError, match="unknown row filter 5"):
        rgb.read_png16(path)
    put(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw[:-7])) + _chunk(b"IEND", b""))
    with pytest.raises(_lib.DcvcError, match="truncated image data"):
        rgb.read_png16(path)
    put(good)
    assert read16(os.fsencode(path), vp(out.ctypes.data), out.nbytes - 1, ctypes.byref(w), ctypes.byref(h)) == -1
    assert "does not fit" in _err(), _err()
    # a 16-bit palette file does not exist in the format
    put(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", 6, 4, 16, 3, 0, 0, 0)) + _chunk(b"IEND", b""))
    with pytest.raises(_lib.DcvcError, match="palette"):
        rgb.png_info2(path)


def test_the_8_bit_reader_still_refuses_a_16_bit_file(tmp_path):
    from dcvc_amd import _lib, rgb
    path = str(tmp_path / "p16.png")
    rgb.write_png16(path, _samples(4, 4, 3))
    with pytest.raises(_lib.DcvcError, match="8-bit PNG only"):
        rgb.read_png(path)
    with pytest.raises(_lib.DcvcError, match="8-bit PNG only"):
        rgb.png_info(path)


# ------------------------------------------------------------------------------------------------------------- manifest
def test_manifest_formats_and_parses_rgb48_and_png16():
    from dcvc_amd import picture_hash as ph
    assert "rgb48" in ph.SRC_TYPES and "png16" in ph.SRC_TYPES
    assert ph.plane_bytes("rgb48", 10, 128, 96) == [6 * 128 * 96] and ph.plane_bytes("png16", 16, 128, 96) == [6 * 128 * 96]
    data = [np.random.default_rng(k).integers(0, 1024, size=(4, 6, 3), dtype=np.uint16).astype("<u2").tobytes() for k in range(3)]
    for src_type, depth in (("rgb48", 10), ("rgb48", 16), ("png16", 16)):
        m = ph.Manifest(src_type, depth, 6, 4, [(zlib.crc32(d), [zlib.crc32(d)]) for d in data])
        assert m.total_bytes == 3 * 6 * 4 * 6 and m.sequence_crc == zlib.crc32(b"".join(data))
        text = ph.format_manifest(m)
        assert text.startswith("# dcvc-hash 1 crc32 %s %d 6 4\n0 %08x %08x\n" % (src_type, depth, zlib.crc32(data[0]), zlib.crc32(data[0])))
        assert ph.parse_manifest(text) == m
    ok = ph.format_manifest(ph.Manifest("rgb48", 10, 6, 4, []))
    for bad in (ok.replace("rgb48 10", "rgb48 8"), ok.replace("rgb48 10", "png16 10"), ok.replace("rgb48 10", "png16 8"),
                ok.replace("rgb48 10", "rgb24 10"), ok.replace("rgb48 10", "png 16"), ok.replace("rgb48 10", "rgb48 17")):
        with pytest.raises(ValueError, match="bad bit depth"):
            ph.parse_manifest(bad)


# ----------------------------------------------------------------------------------------------------------------- tool
def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra, size=("128", "96")):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.rgb"), "-o", str(tmp_path / "o.bin"),
                 "-W", size[0], "-H", size[1]] + extra)


def _decode(tmp_path, extra, out="o.rgb"):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path / out)] + extra)


def _no_output(tmp_path):
    return not any((tmp_path / n).exists() for n in ("o.bin", "o.rgb", "x.y4m"))


def test_tool_refuses_by_the_flags_alone(tmp_path):
    """before a model is loaded (the weight files named here do not exist), with status 2 and no output file"""
    for bad in ("8", "7", "17", "ten", ""):
        for mode, r in (("encode", _encode(tmp_path, ["--src-type", "rgb48", "--bit-depth", bad])),
                        ("decode", _decode(tmp_path, ["--src-type", "rgb48", "--bit-depth", bad]))):
            assert r.returncode == 2 and "--src-type rgb48 takes --bit-depth 9..16" in r.stderr and "got " + bad in r.stderr, (mode, bad, r.stderr)
    for bad in ("10", "8", "12"):
        r = _decode(tmp_path, ["--src-type", "png16", "--bit-depth", bad])
        assert r.returncode == 2 and "--src-type png16 holds 16-bit samples" in r.stderr and "--bit-depth " + bad in r.stderr, (bad, r.stderr)
        r = _encode(tmp_path, ["--src-type", "png16", "--bit-depth", bad])
        assert r.returncode == 2 and "--src-type png16 holds 16-bit samples" in r.stderr, (bad, r.stderr)
    for t in ("rgb48", "png16"):
        r = _encode(tmp_path, ["--src-type", t, "--scale", "64x48"])
        assert r.returncode == 2 and "--scale is for --src-type yuv420: RGB sources are not resampled yet" in r.stderr, (t, r.stderr)
        r = _decode(tmp_path, ["--src-type", t, "--out-size", "64x48"])
        assert r.returncode == 2 and "--out-size is for --src-type yuv420: RGB sources are not resampled yet" in r.stderr, (t, r.stderr)
        r = _decode(tmp_path, ["--src-type", t], out="x.y4m")
        assert r.returncode == 2 and "a Y4M file holds YUV pictures, not --src-type " + t in r.stderr, (t, r.stderr)
        r = _decode(tmp_path, ["--src-type", t, "--ref", str(tmp_path / "ref.y4m")])
        assert r.returncode == 2 and "--ref" in r.stderr and "a Y4M file holds YUV pictures, not --src-type " + t in r.stderr, (t, r.stderr)
    r = _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "o.bin"),
              "--src-type", "rgb48", "-W", "128", "-H", "96"])
    assert r.returncode == 2 and "-i" in r.stderr and "a Y4M file holds YUV pictures, not --src-type rgb48" in r.stderr, r.stderr
    for size in (("127", "96"), ("128", "95"), ("0", "96")):
        r = _encode(tmp_path, ["--src-type", "rgb48"], size=size)
        assert r.returncode == 2 and "picture size must be positive and even" in r.stderr and "missing.dcvw" not in r.stderr, (size, r.stderr)
    r = _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.rgb"), "-o", str(tmp_path / "o.bin"),
              "--src-type", "rgb48"])
    assert r.returncode == 2 and "--src-type rgb48 needs -W and -H" in r.stderr, r.stderr
    assert _no_output(tmp_path)


def test_tool_png16_refuses_an_8_bit_file_with_its_name(tmp_path):
    from dcvc_amd import rgb
    d = tmp_path / "seq"
    d.mkdir()
    rgb.write_png(str(d / "im00001.png"), np.zeros((96, 128, 3), np.uint8))
    r = _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(d), "-o", str(tmp_path / "o.bin"), "--src-type", "png16"])
    assert r.returncode == 2 and "im00001.png is an 8-bit PNG" in r.stderr and "missing.dcvw" not in r.stderr, r.stderr
    assert _no_output(tmp_path)


@pytest.mark.parametrize("flags", [["--src-type", "rgb48"], ["--src-type", "rgb48", "--bit-depth", "10"], ["--src-type", "rgb48", "--bit-depth", "16"],
                                   ["--src-type", "rgb48", "--bit-depth", "12", "--matrix", "bt2020", "--range", "limited", "--yuv-depth", "10"]],
                         ids=lambda f: "_".join(f).replace("-", ""))
def test_tool_valid_flags_pass_the_flag_checks(tmp_path, flags):
    for mode, r in (("encode", _encode(tmp_path, flags)), ("decode", _decode(tmp_path, flags)),
                    ("decode png16", _decode(tmp_path, ["--src-type", "png16", "--bit-depth", "16"]))):
        assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, (mode, r.stderr)
    assert _no_output(tmp_path)
