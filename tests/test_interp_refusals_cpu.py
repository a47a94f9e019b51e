"""dcvc_interp_select and dcvc_interp_planes refuse a bad argument before any device work (interp_select_validate,
interp_planes_validate): every call below passes never-dereferenced device pointers on a box without a GPU, must
return < 0 and must name the entry in dcvc_last_error."""
import ctypes

import pytest

vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
U8, F16, U16, F32 = 0, 1, 3, 4
A, B, MV, PLAN, WB, SAD, FALLEN, DST = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000    # never dereferenced
H, W = 48, 64                                          # 3 x 4 blocks


def _p(v):
    return vp(v) if v else None


def _select(a=A, ars=W, b=B, brs=W, dtype=U8, bit_depth=8, H=H, W=W, mv=MV, mbh=3, mbw=4, k=1, n=2, limit=8, plan=PLAN, wb=WB, bh=3, bw=4,
            sad=SAD, fallen=FALLEN):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_interp_select", ci, [vp, ci, vp, ci, ci, ci, ci, ci, vp, ci, ci, ci, ci, ci, vp, vp, ci, ci, vp, vp, vp])
    rc = f(_p(a), ars, _p(b), brs, dtype, bit_depth, H, W, _p(mv), mbh, mbw, k, n, limit, _p(plan), _p(wb), bh, bw, _p(sad), _p(fallen), None)
    return rc, _lib.lib().dcvc_last_error().decode()


def _planes(a=A, ars=W, aps=H * W, b=B, brs=W, bps=H * W, dst=DST, drs=W, dps=H * W, dtype=U8, H=H, W=W, n_planes=1, sx=0, sy=0, plan=PLAN,
            wb=WB, bh=3, bw=4, k=1, n=2, fallen=0, n_blocks=0):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_interp_planes", ci, [vp, ci, cll, vp, ci, cll, vp, ci, cll, ci, ci, ci, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp, ci, vp])
    rc = f(_p(a), ars, aps, _p(b), brs, bps, _p(dst), drs, dps, dtype, H, W, n_planes, sx, sy, _p(plan), _p(wb), bh, bw, k, n, _p(fallen),
           n_blocks, None)
    return rc, _lib.lib().dcvc_last_error().decode()


SELECT_REFUSED = [
    ("null a", dict(a=0)),
    ("null b", dict(b=0)),
    ("null mv", dict(mv=0)),
    ("null plan", dict(plan=0)),
    ("null wb", dict(wb=0)),
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
    ("H = 16385", dict(H=16385, mbh=1025, bh=1025)),
    ("W = 16385", dict(W=16385, ars=16385, brs=16385, mbw=1025, bw=1025)),
    ("n = 1", dict(n=1, k=1)),
    ("n = 9", dict(n=9)),
    ("n = 0", dict(n=0, k=0)),
    ("k = 0", dict(k=0)),
    ("k = n", dict(k=2)),
    ("k = n at n = 8", dict(k=8, n=8)),
    ("k = -1", dict(k=-1, n=3)),
    ("limit = -1", dict(limit=-1)),
    ("limit = 256", dict(limit=256)),
    ("mv grid one row short", dict(mbh=2)),
    ("mv grid one column short", dict(mbw=3)),
    ("plan grid one row short", dict(bh=2)),
    ("plan grid one column short", dict(bw=3)),
    ("plan grid 0 x 0", dict(bh=0, bw=0)),
    ("a row stride below W", dict(ars=W - 1)),
    ("b row stride below W", dict(brs=W - 1)),
    ("u16 a at an odd address", dict(dtype=U16, bit_depth=10, a=A + 1)),
    ("u16 b at an odd address", dict(dtype=U16, bit_depth=10, b=B + 1)),
    ("mv at an odd address", dict(mv=MV + 1)),
    ("plan at an odd address", dict(plan=PLAN + 1)),
    ("sad at an address that is no multiple of 4", dict(sad=SAD + 2)),
    ("fallen at an address that is no multiple of 4", dict(fallen=FALLEN + 2)),
]

PLANES_REFUSED = [
    ("null a", dict(a=0)),
    ("null b", dict(b=0)),
    ("null dst", dict(dst=0)),
    ("null plan", dict(plan=0)),
    ("null wb", dict(wb=0)),
    ("fp16 samples", dict(dtype=F16)),
    ("fp32 samples", dict(dtype=F32)),
    ("sample type 2", dict(dtype=2)),
    ("H = 0", dict(H=0)),
    ("W = 0", dict(W=0)),
    ("H = 16385", dict(H=16385, bh=1025)),
    ("W = 16385", dict(W=16385, ars=16385, brs=16385, drs=16385, bw=1025)),
    ("n = 1", dict(n=1)),
    ("n = 9", dict(n=9)),
    ("k = 0", dict(k=0)),
    ("k = n", dict(k=3, n=3)),
    ("sx = 2", dict(sx=2)),
    ("sx = -1", dict(sx=-1)),
    ("sy = 2", dict(sy=2)),
    ("sy = -1", dict(sy=-1)),
    ("n_planes = 0", dict(n_planes=0)),
    ("n_planes = 65536", dict(n_planes=65536)),
    ("plan grid one row short", dict(bh=2)),
    ("plan grid one column short", dict(bw=3)),
    ("plan grid too small for a chroma plane of this size", dict(sx=1, sy=1, bh=5, bw=8)),      # 48 / 8 = 6 rows are needed
    ("fallen without n_blocks", dict(fallen=FALLEN, n_blocks=0)),
    ("fallen at an address that is no multiple of 4", dict(fallen=FALLEN + 2, n_blocks=12)),
    ("a row stride below W", dict(ars=W - 1)),
    ("b row stride below W", dict(brs=W - 1)),
    ("dst row stride below W", dict(drs=W - 1)),
    ("a plane stride below the plane", dict(n_planes=2, aps=H * W - 1)),
    ("b plane stride below the plane", dict(n_planes=2, bps=H * W - 1)),
    ("dst plane stride below the plane", dict(n_planes=2, dps=H * W - 1)),
    ("u16 a at an odd address", dict(dtype=U16, a=A + 1)),
    ("u16 b at an odd address", dict(dtype=U16, b=B + 1)),
    ("u16 dst at an odd address", dict(dtype=U16, dst=DST + 1)),
    ("plan at an odd address", dict(plan=PLAN + 1)),
    ("dst is a", dict(dst=A)),
    ("dst is b", dict(dst=B)),
    ("dst starts inside a", dict(dst=A + H * W - 1)),
    ("dst ends inside b", dict(dst=B - H * W + 1)),
    ("dst starts inside b's second plane", dict(n_planes=2, dst=B + 2 * H * W - 1)),
    ("dst is plan", dict(dst=PLAN)),
    ("dst ends inside plan", dict(dst=PLAN - H * W + 1)),
    ("dst starts inside plan", dict(dst=PLAN + 3 * 4 * 8 - 1)),
    ("dst is wb", dict(dst=WB)),
    ("dst ends inside wb", dict(dst=WB - H * W + 1)),
    ("dst starts inside wb", dict(dst=WB + 3 * 4 - 1)),
]


@pytest.mark.parametrize("why,kwargs", SELECT_REFUSED, ids=[r[0].replace(" ", "_") for r in SELECT_REFUSED])
def test_the_selection_refuses_before_any_launch(why, kwargs):
    rc, err = _select(**kwargs)
    assert rc < 0, why
    assert err.startswith("interp_select:"), err


@pytest.mark.parametrize("why,kwargs", PLANES_REFUSED, ids=[r[0].replace(" ", "_") for r in PLANES_REFUSED])
def test_the_interpolation_refuses_before_any_launch(why, kwargs):
    rc, err = _planes(**kwargs)
    assert rc < 0, why
    assert err.startswith("interp_planes:"), err


def test_the_messages_say_what_is_wrong():
    assert "got 9" in _select(n=9)[1] and "2..8" in _select(n=9)[1]
    assert "got 2" in _select(k=2)[1] and "1..1" in _select(k=2)[1]
    assert "got 256" in _select(limit=256)[1] and "0..255" in _select(limit=256)[1]
    assert "1..16384" in _select(H=16385, mbh=1025, bh=1025)[1]
    assert "mv grid" in _select(mbw=3)[1] and "needs 4x3" in _select(mbw=3)[1]
    assert "plan grid" in _select(bw=3)[1] and "needs 4x3" in _select(bw=3)[1]
    assert "got 10" in _select(bit_depth=10)[1]
    for name, at in (("a", A), ("b", B), ("plan", PLAN), ("wb", WB)):
        assert ("overlaps " + name) in _planes(dst=at)[1]
    assert "needs 8x6" in _planes(sx=1, sy=1, bh=5, bw=8)[1]
    assert "n_blocks" in _planes(fallen=FALLEN, n_blocks=0)[1]
