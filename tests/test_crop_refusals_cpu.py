"""dcvc_crop_stats and dcvc_window_planes refuse a bad argument before any device work (crop_stats_validate,
window_planes_validate): every call below passes never-dereferenced device pointers on a box without a GPU, must
return < 0 and must name the kernel in dcvc_last_error."""
import ctypes

import pytest

vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
U8, F16, U16, F32 = 0, 1, 3, 4
SRC, DST, OUT = 0x100000, 0x300000, 0x400000          # never dereferenced; at least 1 MiB apart


def _stats(luma=SRC, rs=64, dtype=U8, bit_depth=8, H=48, W=64, limit=24, counts=OUT):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_crop_stats", ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp])
    rc = f(vp(luma) if luma else None, rs, dtype, bit_depth, H, W, limit, vp(counts) if counts else None, None)
    return rc, _lib.lib().dcvc_last_error().decode()


def _window(src=SRC, srs=64, sps=64 * 48, Hs=48, Ws=64, dst=DST, drs=32, dps=32 * 24, Hd=24, Wd=32, dtype=U8, n_planes=1, ox=16, oy=12,
            fill=(16,)):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_window_planes", ci, [vp, ci, cll, ci, ci, vp, ci, cll, ci, ci, ci, ci, ci, ci, ctypes.POINTER(ci), vp])
    fills = (ci * len(fill))(*fill) if fill is not None else None
    rc = f(vp(src) if src else None, srs, sps, Hs, Ws, vp(dst) if dst else None, drs, dps, Hd, Wd, dtype, n_planes, ox, oy, fills, None)
    return rc, _lib.lib().dcvc_last_error().decode()


STATS_REFUSED = [
    ("null luma", dict(luma=0), "null operand"),
    ("null counts", dict(counts=0), "null operand"),
    ("fp16 samples", dict(dtype=F16), "sample type"),
    ("fp32 samples", dict(dtype=F32), "sample type"),
    ("sample type 2", dict(dtype=2), "sample type"),
    ("sample type -1", dict(dtype=-1), "sample type"),
    ("u8 at 10 bits", dict(bit_depth=10), "bit_depth must be 8 (u8) or 9..16 (u16), got 10"),
    ("u8 at 7 bits", dict(bit_depth=7), "got 7"),
    ("u16 at 8 bits", dict(dtype=U16, bit_depth=8), "got 8"),
    ("u16 at 17 bits", dict(dtype=U16, bit_depth=17), "got 17"),
    ("H = 0", dict(H=0), "the plane must be in 1..16384 a side, got 64x0"),
    ("H = -1", dict(H=-1), "the plane must be in 1..16384 a side"),
    ("H = 16385", dict(H=16385), "the plane must be in 1..16384 a side"),
    ("W = 0", dict(W=0), "the plane must be in 1..16384 a side, got 0x48"),
    ("W = 16385", dict(W=16385, rs=16385), "the plane must be in 1..16384 a side"),
    ("limit = -1", dict(limit=-1), "limit must be in 0..255, got -1"),
    ("limit = 256", dict(limit=256), "limit must be in 0..255, got 256"),
    ("row stride below W", dict(rs=63), "the row stride is below the width"),
    ("u16 luma at an odd address", dict(dtype=U16, bit_depth=10, luma=SRC + 1), "a 16-bit plane must be 2-byte aligned"),
    ("counts at 2 bytes", dict(counts=OUT + 2), "counts must be 4-byte aligned"),
    ("counts at an odd address", dict(counts=OUT + 1), "counts must be 4-byte aligned"),
]


@pytest.mark.parametrize("why,kwargs,words", STATS_REFUSED, ids=[r[0].replace(" ", "_") for r in STATS_REFUSED])
def test_crop_stats_refuses_before_any_launch(why, kwargs, words):
    rc, err = _stats(**kwargs)
    assert rc < 0, why
    assert err.startswith("crop_stats:") and words in err, err


def test_crop_stats_takes_the_edges_as_far_as_the_last_check():
    # 1 x 1 and 16384 x 16384 at limit 0 / 255 pass every check but the one provoked last
    for kw in (dict(H=1, W=1, rs=1, limit=0), dict(H=16384, W=16384, rs=16384, limit=255), dict(dtype=U16, bit_depth=16),
               dict(dtype=U16, bit_depth=9)):
        rc, err = _stats(counts=OUT + 2, **kw)
        assert rc < 0 and "counts must be 4-byte aligned" in err, err


WINDOW_REFUSED = [
    ("null src", dict(src=0), "null operand"),
    ("null dst", dict(dst=0), "null operand"),
    ("null fill", dict(fill=None), "null operand"),
    ("fp16 samples", dict(dtype=F16), "sample type"),
    ("sample type 2", dict(dtype=2), "sample type"),
    ("sample type -1", dict(dtype=-1), "sample type"),
    ("Hs = 0", dict(Hs=0), "the source must be in 1..16384 a side"),
    ("Hs = 16385", dict(Hs=16385), "the source must be in 1..16384 a side"),
    ("Ws = 0", dict(Ws=0), "the source must be in 1..16384 a side"),
    ("Ws = 16385", dict(Ws=16385, srs=16385), "the source must be in 1..16384 a side"),
    ("Hd = 0", dict(Hd=0), "the window must be in 1..16384 a side"),
    ("Hd = 16385", dict(Hd=16385), "the window must be in 1..16384 a side"),
    ("Wd = -1", dict(Wd=-1), "the window must be in 1..16384 a side"),
    ("Wd = 16385", dict(Wd=16385, drs=16385), "the window must be in 1..16384 a side"),
    ("n_planes = 0", dict(n_planes=0), "n_planes must be in 1..65535"),
    ("n_planes = 65536", dict(n_planes=65536), "n_planes must be in 1..65535"),
    ("ox = 16385", dict(ox=16385), "the offsets must be in -16384..16384, got 16385, 12"),
    ("ox = -16385", dict(ox=-16385), "the offsets must be in -16384..16384"),
    ("oy = 16385", dict(oy=16385), "the offsets must be in -16384..16384"),
    ("oy = -16385", dict(oy=-16385), "the offsets must be in -16384..16384, got 16, -16385"),
    ("u8 fill 256", dict(fill=(256,)), "fill value 256 of plane 0 is outside 0..255"),
    ("fill -1", dict(fill=(-1,)), "fill value -1 of plane 0 is outside 0..255"),
    ("u16 fill 65536", dict(dtype=U16, fill=(65536,)), "fill value 65536 of plane 0 is outside 0..65535"),
    ("second plane's fill", dict(n_planes=2, fill=(0, 300)), "fill value 300 of plane 1 is outside 0..255"),
    ("src row stride below Ws", dict(srs=63), "a row stride is below the width"),
    ("dst row stride below Wd", dict(drs=31), "a row stride is below the width"),
    ("src plane stride below the plane", dict(n_planes=2, fill=(0, 0), sps=64 * 48 - 1), "a plane stride is below the plane"),
    ("dst plane stride below the plane", dict(n_planes=2, fill=(0, 0), dps=32 * 24 - 1), "a plane stride is below the plane"),
    ("u16 src at an odd address", dict(dtype=U16, src=SRC + 1), "16-bit planes must be 2-byte aligned"),
    ("u16 dst at an odd address", dict(dtype=U16, dst=DST + 1), "16-bit planes must be 2-byte aligned"),
    ("dst is src", dict(dst=SRC), "dst overlaps src"),
    ("dst starts inside src", dict(dst=SRC + 64 * 48 - 1), "dst overlaps src"),
    ("dst ends inside src", dict(dst=SRC - 32 * 24 + 1), "dst overlaps src"),
    ("dst starts inside src's second plane", dict(n_planes=2, fill=(0, 0), dst=SRC + 2 * 64 * 48 - 1), "dst overlaps src"),
]


@pytest.mark.parametrize("why,kwargs,words", WINDOW_REFUSED, ids=[r[0].replace(" ", "_") for r in WINDOW_REFUSED])
def test_window_planes_refuses_before_any_launch(why, kwargs, words):
    rc, err = _window(**kwargs)
    assert rc < 0, why
    assert err.startswith("window_planes:") and words in err, err


def test_window_planes_does_not_read_plane_strides_for_one_plane_and_takes_the_largest_offsets():
    # a plane stride of 0 and offsets of +-16384 get as far as the overlap check, the last
    for ox, oy in ((16384, -16384), (-16384, 16384), (0, 0)):
        rc, err = _window(sps=0, dps=0, ox=ox, oy=oy, dst=SRC + 64 * 48 - 1)
        assert rc < 0 and "dst overlaps src" in err, err
