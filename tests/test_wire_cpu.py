"""Wire formats without a GPU: the v210 known vector and both round-trip identities in the numpy restatement
(tests/wire_np.py), dcvc_wire_picture_bytes and dcvc_wire_carrier against it, every refusal of the four entry points with
never-dereferenced pointers (the pattern of test_pixfmt_refusals_cpu.py), and the dcvc tool's refusals that the flags alone
decide - before a model is loaded: the weight files named here do not exist. dcvc_pix_to_x still knows four formats."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import wire_np as wn

vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
P = vp(0x100000)          # never dereferenced; far enough apart for a 16 x 24 picture
P2 = vp(0x200000)
NULL = None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")

SIG = {
    "wire_carrier": (ci, [ci]),
    "wire_picture_bytes": (cll, [ci, ci, ci, ci]),
    "wire_unpack": (ci, [vp, ci, ci, ci, ci, vp, vp]),
    "wire_pack": (ci, [vp, ci, ci, ci, ci, vp, vp]),
}
CASES = [(w, b) for w in sorted(wn.DEPTHS) for b in wn.DEPTHS[w]]


def _fn(name):
    from dcvc_amd import _lib
    return _lib.fn("dcvc_" + name, *SIG[name])


def _err():
    from dcvc_amd import _lib
    return _lib.lib().dcvc_last_error().decode()


def test_v210_known_vector():
    words = [0x00300801, 0x00601404, 0x00902007, 0x00C02C0A]
    assert wn.v210_words(range(1, 13)) == words
    # the same group through pack / unpack: fields 1..12 in wire order are Cb0 Y0 Cr0 Y1 Cb1 Y2 Cr1 Y3 Cb2 Y4 Cr2 Y5
    y, cb, cr = [2, 4, 6, 8, 10, 12], [1, 5, 9], [3, 7, 11]
    c = np.array(y + y + cb + cb + cr + cr, dtype=np.uint16)             # 2 rows of 6 pixels
    p = wn.pack(c, wn.V210, 10, 2, 6)
    assert p.size == 256
    row = p.view("<u4").reshape(2, 32)
    assert row[0, :4].tolist() == words and row[1, :4].tolist() == words and not row[:, 4:].any()
    assert np.array_equal(wn.unpack(p, wn.V210, 10, 2, 6), c)


@pytest.mark.parametrize("H,W,v210_row", [(2, 2, 128), (4, 46, 128), (4, 48, 128), (6, 50, 256)])
def test_picture_bytes(H, W, v210_row):
    f = _fn("wire_picture_bytes")
    for wire, bits in CASES:
        assert f(wire, bits, H, W) == wn.picture_bytes(wire, bits, H, W), (wire, bits)
    assert f(wn.V210, 10, H, W) == H * v210_row
    assert f(wn.NV21, 8, H, W) == H * W * 3 // 2 and f(wn.UYVY, 8, H, W) == 2 * H * W
    assert f(wn.NV16, 10, H, W) == 4 * H * W and f(wn.YUY2, 16, H, W) == 4 * H * W


def test_carrier():
    f = _fn("wire_carrier")
    assert [f(w) for w in range(5)] == [3, 1, 1, 1, 1]                   # DCVC_PIX_NV12, then DCVC_PIX_YUV422P
    assert [f(w) for w in range(5)] == [wn.carrier(w) for w in range(5)]
    for bad in (-1, 5, 99):
        assert f(bad) < 0 and _err().startswith("wire_carrier:") and "unknown wire format" in _err()


@pytest.mark.parametrize("wire,bits", CASES, ids=["%d-%d" % c for c in CASES])
def test_round_trips_in_numpy(wire, bits):
    rng = np.random.default_rng(1000 * wire + bits)
    for H, W in [(2, 2), (2, 6), (4, 46), (6, 50), (16, 96)]:
        c = wn.random_carrier(rng, wire, bits, H, W)
        p = wn.pack(c, wire, bits, H, W)
        assert p.dtype == np.uint8 and p.size == wn.picture_bytes(wire, bits, H, W)
        assert np.array_equal(wn.unpack(p, wire, bits, H, W), c)                      # unpack(pack(c)) == c
        assert not (p & wn.ignored_mask(wire, bits, H, W)).any()                      # pack leaves the ignored bits zero
        q = rng.integers(0, 256, p.size, dtype=np.uint8) & ~wn.ignored_mask(wire, bits, H, W)
        assert np.array_equal(wn.pack(wn.unpack(q, wire, bits, H, W), wire, bits, H, W), q)      # pack(unpack(p)) == p
        g = q | (rng.integers(0, 256, p.size, dtype=np.uint8) & wn.ignored_mask(wire, bits, H, W))
        assert np.array_equal(wn.unpack(g, wire, bits, H, W), wn.unpack(q, wire, bits, H, W))    # ignored bits are ignored


def test_every_v210_code_and_every_u16_pattern():
    # all 1024 codes in Y, Cb and Cr: 2 x 1024 luma samples hold each twice, each chroma plane once
    H, W = 2, 1024
    codes = np.arange(1024, dtype=np.uint16)
    c = np.concatenate([codes, codes[::-1], codes, (codes + 7) % 1024]).astype(np.uint16)
    p = wn.pack(c, wn.V210, 10, H, W)
    assert np.array_equal(wn.unpack(p, wn.V210, 10, H, W), c)
    assert np.array_equal(wn.pack(wn.unpack(p, wn.V210, 10, H, W), wn.V210, 10, H, W), p)
    # all 65536 patterns of a u16 in a yuy2 picture at 16 bits: 2 H W = 65536 samples
    H, W = 128, 256
    p = np.arange(65536, dtype="<u2").view(np.uint8)
    c = wn.unpack(p, wn.YUY2, 16, H, W)
    assert np.array_equal(np.sort(c), np.arange(65536)) and np.array_equal(wn.pack(c, wn.YUY2, 16, H, W), p)


def _args(src=P, wire=wn.UYVY, bits=8, H=16, W=24, dst=P2):
    return (src, wire, bits, H, W, dst, NULL)


def _refusals(name):
    r = [
        (name, _args(src=NULL), "null source"),
        (name, _args(dst=NULL), "null destination"),
        (name, _args(wire=5), "unknown format"),
        (name, _args(wire=-1), "negative format"),
        (name, _args(wire=wn.NV21, bits=10), "nv21 at 10 bits"),
        (name, _args(wire=wn.UYVY, bits=10), "uyvy at 10 bits"),
        (name, _args(wire=wn.V210, bits=8), "v210 at 8 bits"),
        (name, _args(wire=wn.V210, bits=12), "v210 at 12 bits"),
        (name, _args(wire=wn.NV16, bits=7), "nv16 at 7 bits"),
        (name, _args(wire=wn.YUY2, bits=17), "yuy2 at 17 bits"),
        (name, _args(H=15), "odd height"),
        (name, _args(W=23), "odd width"),
        (name, _args(H=0), "no rows"),
        (name, _args(W=-2), "negative width"),
        (name, _args(H=1 << 18, W=1 << 17), "beyond the 32-bit thread index"),
        (name, _args(wire=wn.V210, bits=10, H=(1 << 30) + 2, W=2), "v210: two threads per row"),
        (name, _args(dst=P), "the same range"),
        (name, _args(dst=vp(0x100000 + 100)), "ranges that overlap"),
        (name, _args(src=vp(0x200000 + 767)), "the last byte overlaps"),
    ]
    return r


REFUSED = _refusals("wire_unpack") + _refusals("wire_pack") + [
    ("wire_picture_bytes", (5, 8, 16, 24), "unknown format"),
    ("wire_picture_bytes", (wn.NV21, 9, 16, 24), "nv21 at 9 bits"),
    ("wire_picture_bytes", (wn.UYVY, 16, 16, 24), "uyvy at 16 bits"),
    ("wire_picture_bytes", (wn.V210, 8, 16, 24), "v210 at 8 bits"),
    ("wire_picture_bytes", (wn.YUY2, 7, 16, 24), "yuy2 at 7 bits"),
    ("wire_picture_bytes", (wn.NV16, 17, 16, 24), "nv16 at 17 bits"),
    ("wire_picture_bytes", (wn.NV16, 8, 15, 24), "odd height"),
    ("wire_picture_bytes", (wn.NV16, 8, 16, 23), "odd width"),
    ("wire_picture_bytes", (wn.NV16, 8, 0, 24), "no rows"),
    ("wire_picture_bytes", (wn.NV16, 8, 1 << 18, 1 << 17), "beyond the 32-bit thread index"),
    ("wire_carrier", (5,), "unknown format"),
    ("wire_carrier", (-1,), "negative format"),
]


@pytest.mark.parametrize("name,args,why", REFUSED, ids=["%s-%s" % (r[0], r[2].replace(" ", "_")) for r in REFUSED])
def test_refused_before_any_launch(name, args, why):
    f = _fn(name)
    assert len(args) == len(SIG[name][1])
    assert f(*args) < 0, why
    assert _err().startswith(name + ":") and "wire" in _err(), _err()


def test_the_refusal_says_what_is_wrong():
    assert _fn("wire_unpack")(*_args(H=1 << 18, W=1 << 17)) < 0 and "picture too large" in _err()
    assert _fn("wire_pack")(*_args(wire=wn.V210, bits=10, H=(1 << 30) + 2, W=2)) < 0 and "picture too large" in _err()
    assert _fn("wire_pack")(*_args(dst=P)) < 0 and "overlap" in _err()
    assert _fn("wire_unpack")(*_args(wire=wn.V210, bits=8)) < 0 and "10 bits" in _err()
    assert _fn("wire_unpack")(*_args(src=NULL)) < 0 and "null" in _err()


def test_every_entry_point_of_the_group_is_tried():
    assert {r[0] for r in REFUSED} == set(SIG)


def test_pix_to_x_still_knows_four_formats():
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_pix_to_x", ci, [vp, ci, ci, ci, ci, vp, ci, vp, vp])
    assert f(P, 4, 8, 16, 24, P2, 3, NULL, NULL) < 0 and "unknown pixel format 4" in _err()
    assert _lib.fn("dcvc_pix_picture_samples", cll, [ci, ci, ci])(4, 16, 24) < 0


# ------------------------------------------------------------------------------------------------ the tool's flag refusals
WIRE_TYPES = ["nv21", "nv16", "p210", "uyvy", "yuy2", "y210", "v210"]


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra, out="o.bin", src="missing.yuv"):
    return _run(["encode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / src), "-o", str(tmp_path / out),
                 "-W", "352", "-H", "288"] + extra)


def _decode(tmp_path, extra, out="o.yuv"):
    return _run(["decode", "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing.bin"), "-o", str(tmp_path / out)]
                + extra)


BAD_DEPTHS = [("p210", "12"), ("y210", "8"), ("v210", "8"), ("v210", "12"), ("uyvy", "10"), ("nv21", "10"), ("nv16", "17"),
              ("yuy2", "7")]


@pytest.mark.parametrize("src_type,depth", BAD_DEPTHS, ids=["%s-%s" % d for d in BAD_DEPTHS])
def test_the_tool_refuses_a_bad_depth(tmp_path, src_type, depth):
    for r in (_encode(tmp_path, ["--src-type", src_type, "--bit-depth", depth]),
              _decode(tmp_path, ["--src-type", src_type, "--bit-depth", depth])):
        assert r.returncode == 2 and "--bit-depth" in r.stderr and "missing.dcvw" not in r.stderr, r.stderr
    assert not (tmp_path / "o.bin").exists() and not (tmp_path / "o.yuv").exists()


@pytest.mark.parametrize("src_type", WIRE_TYPES)
def test_the_tool_refuses_what_the_flags_decide(tmp_path, src_type):
    r = _encode(tmp_path, ["--scale", "176x144", "--src-type", src_type])
    assert r.returncode == 2 and src_type + " sources are not resampled yet" in r.stderr, r.stderr
    r = _decode(tmp_path, ["--out-size", "176x144", "--src-type", src_type])
    assert r.returncode == 2 and src_type + " sources are not resampled yet" in r.stderr, r.stderr
    r = _decode(tmp_path, ["--src-type", src_type], out="rec.y4m")
    assert r.returncode == 2 and "Y4M" in r.stderr and src_type in r.stderr and "missing.dcvw" not in r.stderr, r.stderr
    r = _decode(tmp_path, ["--src-type", src_type, "--ref", str(tmp_path / "ref.y4m")])
    assert r.returncode == 2 and "Y4M" in r.stderr and src_type in r.stderr and "missing.dcvw" not in r.stderr, r.stderr
    r = _encode(tmp_path, ["--src-type", src_type], src="in.y4m")
    assert r.returncode == 2 and "Y4M" in r.stderr and src_type in r.stderr and "missing.dcvw" not in r.stderr, r.stderr
    for flags in (["--matrix", "bt601"], ["--range", "limited"]):
        r = _encode(tmp_path, ["--src-type", src_type] + flags)
        assert r.returncode == 2 and src_type + " pictures are not converted" in r.stderr, r.stderr
        r = _decode(tmp_path, ["--src-type", src_type] + flags)
        assert r.returncode == 2 and src_type + " pictures are not converted" in r.stderr, r.stderr
    assert not any((tmp_path / n).exists() for n in ("o.bin", "o.yuv", "rec.y4m"))


@pytest.mark.parametrize("src_type", WIRE_TYPES)
def test_good_flags_pass_on_to_the_model(tmp_path, src_type):
    extra = {"nv16": ["--bit-depth", "12"], "yuy2": ["--bit-depth", "16"], "v210": ["--bit-depth", "10"], "p210": ["--bit-depth", "10"]}
    for r in (_encode(tmp_path, ["--src-type", src_type] + extra.get(src_type, [])),
              _decode(tmp_path, ["--src-type", src_type] + extra.get(src_type, []))):
        assert r.returncode == 2 and "cannot open" in r.stderr and "missing.dcvw" in r.stderr, r.stderr
