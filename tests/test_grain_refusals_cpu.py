"""dcvc_grain_apply and dcvc_grain_stats refuse a bad argument before any device work (grain_apply_validate,
grain_stats_validate): every call below passes never-dereferenced device pointers on a box without a GPU, must
return < 0 and must name the kernel in dcvc_last_error. (dcvc_grain_template and dcvc_grain_fit: test_grain_cpu.py.)"""
import ctypes

import pytest

vp, ci, cll, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_uint32
U8, F16, U16, F32 = 0, 1, 3, 4
REC, LUMA, DST, TPL, SRC, DEN, WORDS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000      # never dereferenced
LUT = bytes(range(27))


def _apply(rec=REC, rrs=64, rps=64 * 48, luma=LUMA, lrs=128, Hl=96, Wl=128, dst=DST, drs=64, dps=64 * 48, dtype=U8, bit_depth=8, H=48, W=64,
           n_planes=2, first_plane=1, sx=1, sy=1, ty=TPL, tu=TPL + 8192, tv=TPL + 16384, lut=LUT, seed=1, pic=0):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_grain_apply", ci, [vp, ci, cll, vp, ci, ci, ci, vp, ci, cll, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, ctypes.c_char_p,
                                         u32, u32, vp])
    p = lambda a: vp(a) if a else None          # noqa: E731
    rc = f(p(rec), rrs, rps, p(luma), lrs, Hl, Wl, p(dst), drs, dps, dtype, bit_depth, H, W, n_planes, first_plane, sx, sy, p(ty), p(tu), p(tv),
           lut, seed, pic, None)
    return rc, _lib.lib().dcvc_last_error().decode()


def _stats(src=SRC, srs=64, sps=64 * 48, den=DEN, drs=64, dps=64 * 48, luma=LUMA, lrs=128, Hl=96, Wl=128, dtype=U8, bit_depth=8, H=48, W=64,
           n_planes=2, sx=1, sy=1, flat=4, accumulate=0, words=WORDS):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_grain_stats", ci, [vp, ci, cll, vp, ci, cll, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp])
    p = lambda a: vp(a) if a else None          # noqa: E731
    rc = f(p(src), srs, sps, p(den), drs, dps, p(luma), lrs, Hl, Wl, dtype, bit_depth, H, W, n_planes, sx, sy, flat, accumulate, p(words), None)
    return rc, _lib.lib().dcvc_last_error().decode()


BOTH = [
    ("null luma", dict(luma=0)),
    ("fp16 samples", dict(dtype=F16)),
    ("fp32 samples", dict(dtype=F32)),
    ("sample type 2", dict(dtype=2)),
    ("sample type -1", dict(dtype=-1)),
    ("u8 at 10 bits", dict(bit_depth=10)),
    ("u8 at 7 bits", dict(bit_depth=7)),
    ("u16 at 8 bits", dict(dtype=U16, bit_depth=8)),
    ("u16 at 17 bits", dict(dtype=U16, bit_depth=17)),
    ("H = 0", dict(H=0)),
    ("W = 0", dict(W=0)),
    ("H = -1", dict(H=-1)),
    ("H = 16385", dict(H=16385, Hl=32768)),
    ("W = 16385", dict(W=16385, Wl=32768, lrs=32768)),
    ("n_planes = 0", dict(n_planes=0)),
    ("sx = 2", dict(sx=2)),
    ("sx = -1", dict(sx=-1)),
    ("sy = 2", dict(sy=2)),
    ("sy = -1", dict(sy=-1)),
    ("luma one row short", dict(Hl=94)),
    ("luma one column short", dict(Wl=126)),
    ("luma of the plane's size at sx = sy = 1", dict(Hl=48, Wl=64)),
    ("luma above 32768", dict(Hl=32769)),
    ("luma row stride below Wl", dict(lrs=127)),
    ("u16 luma at an odd address", dict(dtype=U16, bit_depth=10, luma=LUMA + 1)),
]
APPLY = BOTH + [
    ("null rec", dict(rec=0)),
    ("null dst", dict(dst=0)),
    ("null lut", dict(lut=None)),
    ("null template of a plane of the call", dict(tu=0)),
    ("null template of the last plane", dict(tv=0)),
    ("a template at an odd address", dict(tv=TPL + 1)),
    ("n_planes = 4", dict(n_planes=4, first_plane=0)),
    ("first_plane = -1", dict(first_plane=-1)),
    ("first_plane = 3", dict(first_plane=3, n_planes=1)),
    ("first_plane + n_planes = 4", dict(first_plane=2)),
    ("rec row stride below W", dict(rrs=63)),
    ("dst row stride below W", dict(drs=63)),
    ("rec plane stride below the plane", dict(rps=64 * 48 - 1)),
    ("dst plane stride below the plane", dict(dps=64 * 48 - 1)),
    ("u16 rec at an odd address", dict(dtype=U16, bit_depth=10, rec=REC + 1)),
    ("u16 dst at an odd address", dict(dtype=U16, bit_depth=10, dst=DST + 1)),
    ("dst starts inside rec", dict(dst=REC + 64 * 48 - 1)),
    ("dst ends inside rec", dict(dst=REC - 1)),
    ("dst is rec at another row stride", dict(dst=REC, drs=65, dps=65 * 48)),
    ("dst is rec at another plane stride", dict(dst=REC, dps=64 * 48 + 1)),
    ("dst is the luma", dict(dst=LUMA)),
    ("dst ends inside the luma", dict(dst=LUMA - 1)),
    ("dst is the luma of several planes", dict(rec=LUMA, dst=LUMA, sx=0, sy=0, n_planes=2, first_plane=0, lrs=64, Hl=48, Wl=64)),
    ("dst is the luma, rec is not", dict(dst=LUMA, sx=0, sy=0, n_planes=1, first_plane=0, lrs=64, Hl=48, Wl=64)),
    ("dst overlaps a template", dict(dst=TPL + 8192 - 4)),
]
STATS = BOTH + [
    ("null src", dict(src=0)),
    ("null den", dict(den=0)),
    ("null words", dict(words=0)),
    ("n_planes = 3", dict(n_planes=3)),
    ("flat = -1", dict(flat=-1)),
    ("flat = 256", dict(flat=256)),
    ("accumulate = 2", dict(accumulate=2)),
    ("accumulate = -1", dict(accumulate=-1)),
    ("src row stride below W", dict(srs=63)),
    ("den row stride below W", dict(drs=63)),
    ("src plane stride below the plane", dict(sps=64 * 48 - 1)),
    ("den plane stride below the plane", dict(dps=64 * 48 - 1)),
    ("u16 src at an odd address", dict(dtype=U16, bit_depth=10, src=SRC + 1)),
    ("u16 den at an odd address", dict(dtype=U16, bit_depth=10, den=DEN + 1)),
    ("words at a 4-byte address", dict(words=WORDS + 4)),
]


@pytest.mark.parametrize("why,kwargs", APPLY, ids=[r[0].replace(" ", "_") for r in APPLY])
def test_apply_refused_before_any_launch(why, kwargs):
    rc, err = _apply(**kwargs)
    assert rc < 0, why
    assert err.startswith("grain_apply:") and "launch" not in err, err


@pytest.mark.parametrize("why,kwargs", STATS, ids=[r[0].replace(" ", "_") for r in STATS])
def test_stats_refused_before_any_launch(why, kwargs):
    rc, err = _stats(**kwargs)
    assert rc < 0, why
    assert err.startswith("grain_stats:") and "launch" not in err, err


def test_each_refusal_has_its_own_message():
    msgs = {}
    for why, kwargs in (("null", dict(rec=0)), ("type", dict(dtype=F16)), ("depth", dict(bit_depth=10)), ("side", dict(H=16385, Hl=32768)),
                        ("planes", dict(n_planes=4, first_plane=0)), ("sub", dict(sx=2)), ("luma", dict(Hl=94)), ("row", dict(rrs=63)),
                        ("plane", dict(rps=1)), ("odd", dict(dtype=U16, bit_depth=10, rec=REC + 1)), ("rec", dict(dst=REC + 2)),
                        ("lum", dict(dst=LUMA)), ("tpl", dict(dst=TPL + 8192)), ("tnull", dict(tu=0))):
        msgs[why] = _apply(**kwargs)[1]
    assert len(set(msgs.values())) == len(msgs), msgs
    assert "got 10" in msgs["depth"] and "1..16384" in msgs["side"] and "127x95" in msgs["luma"] and "got 128x94" in msgs["luma"]
    assert "overlaps rec" in msgs["rec"] and "overlaps the luma" in msgs["lum"] and "overlaps a template" in msgs["tpl"]
    assert "got 256" in _stats(flat=256)[1] and "8-byte" in _stats(words=WORDS + 4)[1] and "got 3" in _stats(n_planes=3)[1]


def test_what_is_allowed_gets_as_far_as_the_last_check():
    """nothing here may be accepted (the pointers are not memory): what is allowed is shown to pass every check but the last
    one - the template overlap in apply, the words' alignment in stats - which the call is made to fail"""
    y = dict(sx=0, sy=0, n_planes=1, first_plane=0, lrs=64, Hl=48, Wl=64, tu=0, tv=0)
    allowed = [
        dict(dst=REC),                                                               # U and V in place
        dict(rec=LUMA, dst=LUMA, **y),                                               # Y in place: rec, luma and dst are one plane
        dict(rec=LUMA, **y),                                                         # Y out of place
        dict(n_planes=1, first_plane=2, tu=0, rps=0, dps=0),                          # one plane: plane strides and other templates unread
        dict(Hl=95, Wl=127),                                                         # the smallest luma plane
    ]
    for kwargs in allowed:
        first = kwargs.get("first_plane", 1)
        kwargs[("ty", "tu", "tv")[first + kwargs.get("n_planes", 2) - 1]] = kwargs.get("dst", DST) + 2
        rc, err = _apply(**kwargs)
        assert rc < 0 and "overlaps a template" in err, (kwargs, err)
    for kwargs in (dict(), dict(accumulate=1), dict(flat=0), dict(flat=255), dict(Hl=95, Wl=127), dict(n_planes=1, sps=0, dps=0),
                   dict(den=LUMA, sx=0, sy=0, n_planes=1, lrs=64, Hl=48, Wl=64)):
        rc, err = _stats(words=WORDS + 4, **kwargs)
        assert rc < 0 and "8-byte" in err, (kwargs, err)
