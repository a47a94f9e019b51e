"""dcvc_resample_planes on a real MI355X against the numpy restatement (tests/resample_np.py) with ==: u8, 10-bit and 16-bit
u16 samples over sizes that take every path of the two kernels (both vector paths and both element paths, rows and widths
that are no multiple of a tile, several workgroups along every grid axis, a copy), random samples, an all-max_val plane and a
0 / max_val checkerboard (the accumulator bound and both clamps), strided operands with guard samples, a non-default stream,
and the refusals that need a plan."""
import numpy as np
import pytest
import torch

import resample_np
from dcvc_amd import _lib, resample
from dcvc_amd.yuv16 import DCVC_SAMPLE_U8, DCVC_SAMPLE_U16

pytestmark = pytest.mark.gpu

# (H, W) -> (h, w)
SIZES = [((48, 96), (24, 48)), ((24, 48), (48, 96)), ((72, 120), (48, 80)), ((48, 64), (72, 96)), ((96, 120), (48, 80)),
         ((50, 46), (25, 23)), ((64, 64), (64, 64))]
KINDS = [("u8", np.uint8, 255), ("u10", np.uint16, 1023), ("u16", np.uint16, 65535)]


def _dev(a):
    """numpy u8 / u16 -> CUDA tensor (16-bit samples as int16 storage, which every torch has)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).cuda()


def _host(t, dtype):
    if dtype == np.uint8:
        return t.cpu().numpy()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _inputs(H, W, dtype, max_val, seed):
    """[3, H, W]: random samples, all max_val, a 0 / max_val checkerboard"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([rng.integers(0, max_val + 1, (H, W)), np.full((H, W), max_val), ((yy + xx) & 1) * max_val]).astype(dtype)


def _reference(planes, h, w, max_val):
    return np.stack([resample_np.resample_plane(p, h, w, max_val) for p in planes])


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d-%dx%d" % (s[0] + s[1]) for s in SIZES])
def test_planes_equal_the_numpy_restatement(size, kind):
    (H, W), (h, w) = size
    _, dtype, max_val = kind
    src = _inputs(H, W, dtype, max_val, seed=H * 1000 + w)
    want = _reference(src, h, w, max_val)
    got = _host(resample.resample_planes(_dev(src), h, w, max_val), dtype)
    assert got.shape == want.shape
    for p, name in enumerate(("random", "all max_val", "checkerboard")):
        bad = np.argwhere(got[p] != want[p])
        assert bad.size == 0, (name, len(bad), bad[:4].tolist())
    if (H, W) == (h, w):
        assert np.array_equal(got, src)                       # the copy
    # one plane on its own, as a 2-D tensor, gives the same plane
    one = _host(resample.resample_planes(_dev(src[0]), h, w, max_val), dtype)
    assert np.array_equal(one, want[0])


def test_1080p_to_540p_u8():
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, (1080, 1920)).astype(np.uint8)
    want = resample_np.resample_plane(src, 540, 960, 255)
    got = _host(resample.resample_planes(_dev(src), 540, 960, 255), np.uint8)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist())


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("strides", [(51, 29), (64, 32), (48, 24)], ids=["odd", "vector", "tail"])
@pytest.mark.parametrize("size", [((50, 46), (25, 23)), ((24, 40), (36, 20))], ids=["down", "mixed"])
def test_strided_planes_leave_the_guard_samples_alone(size, strides, kind):
    """row strides above the widths and n_planes = 2 at a plane stride; the vector paths with a ragged last thread included"""
    (H, W), (h, w) = size
    _, dtype, max_val = kind
    s_row, d_row = strides
    s_rows, d_rows = H + 3, h + 2                              # rows a plane stride spans
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5
    src_full = np.random.default_rng(7).integers(0, max_val + 1, (2, s_rows, s_row)).astype(dtype)
    dst_full = np.full((2, d_rows, d_row), guard, dtype)
    want = _reference(src_full[:, :H, :W], h, w, max_val)
    t, o = _dev(src_full), _dev(dst_full)
    plan = resample.Plan(H, W, h, w)
    plan.run(t[:, :H, :W], max_val, out=o[:, :h, :w])
    got = _host(o, dtype)
    plan.close()
    assert np.array_equal(got[:, :h, :w], want)
    mask = np.ones(dst_full.shape, bool)
    mask[:, :h, :w] = False
    assert (got[mask] == guard).all(), "samples outside the destination planes were written"
    assert np.array_equal(_host(t, dtype), src_full)


def test_a_plan_serves_call_after_call_and_a_side_stream():
    (H, W), (h, w) = (72, 120), (48, 80)
    src = _inputs(H, W, np.uint16, 1023, seed=5)
    want = _reference(src, h, w, 1023)
    plan = resample.Plan(H, W, h, w)
    base = _dev(src)
    first = _host(plan.run(base, 1023), np.uint16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the input is made on the side stream right before the call and read right after it: only stream order protects them
        t = (base.to(torch.int32) + 0).to(torch.int16)
        got = plan.run(t, 1023).clone()
        t.zero_()
    side.synchronize()
    plan.close()
    assert np.array_equal(first, want) and np.array_equal(_host(got, np.uint16), want)


def test_refusals_come_before_any_launch():
    H, W, h, w = 24, 48, 12, 24
    plan = resample.Plan(H, W, h, w)
    fn = resample._fn("dcvc_resample_planes")
    src = torch.zeros((2, H, W), dtype=torch.uint8, device="cuda")
    dst = torch.full((2, h, w), 7, dtype=torch.uint8, device="cuda")
    need = plan.workspace_bytes(2)
    assert need >= 2 * H * w * 2 and plan.workspace_bytes(0) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ok = dict(src=src.data_ptr(), sdt=DCVC_SAMPLE_U8, srow=W, splane=H * W, dst=dst.data_ptr(), ddt=DCVC_SAMPLE_U8, drow=w,
              dplane=h * w, n=2, max_val=255, ws=ws.data_ptr(), ws_bytes=need)

    def call(**kw):
        a = dict(ok, **kw)
        return fn(plan._p, a["src"], a["sdt"], a["srow"], a["splane"], a["dst"], a["ddt"], a["drow"], a["dplane"], a["n"], a["max_val"],
                  a["ws"], a["ws_bytes"], stream)

    bad = [dict(src=None), dict(dst=None), dict(ws=None), dict(sdt=1, ddt=1), dict(sdt=4, ddt=4), dict(sdt=2, ddt=2),
           dict(ddt=DCVC_SAMPLE_U16), dict(max_val=0), dict(max_val=256), dict(sdt=DCVC_SAMPLE_U16, ddt=DCVC_SAMPLE_U16, max_val=65536),
           dict(srow=W - 1), dict(drow=w - 1), dict(splane=H * W - 1), dict(dplane=h * w - 1), dict(n=0), dict(n=-1),
           dict(ws_bytes=need - 1), dict(ws_bytes=-1), dict(dst=src.data_ptr()), dict(dst=src.data_ptr() + 2 * H * W - 1),
           dict(n=1, dst=src.data_ptr() + H * W - 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "resample" in _lib.lib().dcvc_last_error().decode(), kw
    torch.cuda.synchronize()
    assert (dst == 7).all() and not src.any()                 # nothing ran
    assert call() == 0
    assert call(n=1, dst=src.data_ptr() + H * W) == 0          # the second source plane as the first one's destination: no overlap
    torch.cuda.synchronize()
    assert not dst.any()
    with pytest.raises(_lib.DcvcError):
        resample.Plan(64, 64, 64, 7)
    with pytest.raises(TypeError):
        plan.run(torch.zeros((H, W), dtype=torch.float16, device="cuda"), 255)
    plan.close()
