"""dcvc_motion_search and dcvc_motion_compensate_planes refuse a bad argument before any device work (motion_search_validate,
motion_compensate_validate): every call below passes never-dereferenced device pointers on a box without a GPU,
must return < 0 and must name the entry in dcvc_last_error."""
import ctypes

import pytest

vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
U8, F16, U16, F32 = 0, 1, 3, 4
CUR, REF, MV, SAD, WS, DST, MOVED = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000    # never dereferenced
H, W = 48, 64                                          # 3 x 4 blocks; the half-resolution planes take 2 * 24 * 32 * 2 bytes
WS_BYTES = 2 * 24 * 32 * 2


def _p(v):
    return vp(v) if v else None


def _search(cur=CUR, crs=W, ref=REF, rrs=W, dtype=U8, bit_depth=8, H=H, W=W, R=7, lam=4, mv=MV, bh=3, bw=4, sad=SAD, moved=0, ws=WS,
            ws_bytes=WS_BYTES):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_motion_search", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp, vp, vp, cll, vp])
    rc = f(_p(cur), crs, _p(ref), rrs, dtype, bit_depth, H, W, R, lam, _p(mv), bh, bw, _p(sad), _p(moved), _p(ws), ws_bytes, None)
    return rc, _lib.lib().dcvc_last_error().decode()


def _comp(prev=REF, prs=W, pps=H * W, dst=DST, drs=W, dps=H * W, dtype=U8, H=H, W=W, n_planes=1, sx=0, sy=0, mv=MV, bh=3, bw=4):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_motion_compensate_planes", ci, [vp, ci, cll, vp, ci, cll, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp])
    rc = f(_p(prev), prs, pps, _p(dst), drs, dps, dtype, H, W, n_planes, sx, sy, _p(mv), bh, bw, None)
    return rc, _lib.lib().dcvc_last_error().decode()


SEARCH_REFUSED = [
    ("null cur", dict(cur=0)),
    ("null ref", dict(ref=0)),
    ("null mv", dict(mv=0)),
    ("null workspace", dict(ws=0)),
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
    ("H = 16385", dict(H=16385, bh=1025, ws_bytes=1 << 30)),
    ("W = 16385", dict(W=16385, crs=16385, rrs=16385, bw=1025, ws_bytes=1 << 30)),
    ("R = -1", dict(R=-1)),
    ("R = 16", dict(R=16)),
    ("lambda = -1", dict(lam=-1)),
    ("lambda = 256", dict(lam=256)),
    ("mv grid one row short", dict(bh=2)),
    ("mv grid one column short", dict(bw=3)),
    ("mv grid 0 x 0", dict(bh=0, bw=0)),
    ("cur row stride below W", dict(crs=W - 1)),
    ("ref row stride below W", dict(rrs=W - 1)),
    ("u16 cur at an odd address", dict(dtype=U16, bit_depth=10, cur=CUR + 1)),
    ("u16 ref at an odd address", dict(dtype=U16, bit_depth=10, ref=REF + 1)),
    ("mv at an odd address", dict(mv=MV + 1)),
    ("sad at an address that is no multiple of 4", dict(sad=SAD + 2)),
    ("moved at an address that is no multiple of 4", dict(moved=MOVED + 2)),
    ("workspace one byte short", dict(ws_bytes=WS_BYTES - 1)),
    ("workspace of 0 bytes", dict(ws_bytes=0)),
    ("workspace of negative size", dict(ws_bytes=-1)),
    ("workspace at an odd address", dict(ws=WS + 1)),
]

COMP_REFUSED = [
    ("null prev", dict(prev=0)),
    ("null dst", dict(dst=0)),
    ("null mv", dict(mv=0)),
    ("fp16 samples", dict(dtype=F16)),
    ("fp32 samples", dict(dtype=F32)),
    ("sample type 2", dict(dtype=2)),
    ("H = 0", dict(H=0)),
    ("W = 0", dict(W=0)),
    ("H = 16385", dict(H=16385, bh=1025)),
    ("W = 16385", dict(W=16385, prs=16385, drs=16385, bw=1025)),
    ("sx = 2", dict(sx=2)),
    ("sx = -1", dict(sx=-1)),
    ("sy = 2", dict(sy=2)),
    ("sy = -1", dict(sy=-1)),
    ("n_planes = 0", dict(n_planes=0)),
    ("n_planes = 65536", dict(n_planes=65536)),
    ("mv grid one row short", dict(bh=2)),
    ("mv grid one column short", dict(bw=3)),
    ("mv grid too small for a chroma plane of this size", dict(sx=1, sy=1, bh=5, bw=8)),      # 48 / 8 = 6 rows are needed
    ("prev row stride below W", dict(prs=W - 1)),
    ("dst row stride below W", dict(drs=W - 1)),
    ("prev plane stride below the plane", dict(n_planes=2, pps=H * W - 1)),
    ("dst plane stride below the plane", dict(n_planes=2, dps=H * W - 1)),
    ("u16 prev at an odd address", dict(dtype=U16, prev=REF + 1)),
    ("u16 dst at an odd address", dict(dtype=U16, dst=DST + 1)),
    ("mv at an odd address", dict(mv=MV + 1)),
    ("dst is prev", dict(dst=REF)),
    ("dst starts inside prev", dict(dst=REF + H * W - 1)),
    ("dst ends inside prev", dict(dst=REF - H * W + 1)),
    ("dst starts inside prev's second plane", dict(n_planes=2, dst=REF + 2 * H * W - 1)),
    ("dst is mv", dict(dst=MV)),
    ("dst ends inside mv", dict(dst=MV - H * W + 1)),
    ("dst starts inside mv", dict(dst=MV + 3 * 4 * 4 - 1)),
]


@pytest.mark.parametrize("why,kwargs", SEARCH_REFUSED, ids=[r[0].replace(" ", "_") for r in SEARCH_REFUSED])
def test_the_search_refuses_before_any_launch(why, kwargs):
    rc, err = _search(**kwargs)
    assert rc < 0, why
    assert err.startswith("motion_search:"), err


@pytest.mark.parametrize("why,kwargs", COMP_REFUSED, ids=[r[0].replace(" ", "_") for r in COMP_REFUSED])
def test_the_compensation_refuses_before_any_launch(why, kwargs):
    rc, err = _comp(**kwargs)
    assert rc < 0, why
    assert err.startswith("motion_compensate:"), err


def test_the_messages_say_what_is_wrong():
    assert "got 16" in _search(R=16)[1] and "0..15" in _search(R=16)[1]
    assert "got 256" in _search(lam=256)[1]
    assert "1..16384" in _search(H=16385, bh=1025, ws_bytes=1 << 30)[1]
    assert "needs 4x3" in _search(bw=3)[1]
    assert "got 10" in _search(bit_depth=10)[1]
    assert "dcvc_motion_search_workspace_bytes" in _search(ws_bytes=WS_BYTES - 1)[1]
    assert "overlaps prev" in _comp(dst=REF)[1] and "overlaps mv" in _comp(dst=MV)[1]
    assert "needs 8x6" in _comp(sx=1, sy=1, bh=5, bw=8)[1]


def test_the_workspace_query():
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_motion_search_workspace_bytes", cll, [ci, ci])
    assert f(H, W) == WS_BYTES
    assert f(1, 1) == 4 and f(17, 33) == 2 * 9 * 17 * 2          # the half-resolution sides round up
    assert f(0, 64) == 0 and f(64, 0) == 0 and f(-1, 64) == 0 and f(16385, 64) == 0 and f(64, 16385) == 0
    assert f(16384, 16384) == 2 * 8192 * 8192 * 2
