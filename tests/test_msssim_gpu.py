"""MS-SSIM on a real MI355X (dcvc_msssim, msssim.hip): the reference's calc_msssim values stored in
tests/golden/msssim_golden.npz, decoded pictures at 1080p and 4K against the fp64 numpy restatement (tests/msssim_np.py),
batching, determinism, stream order, argument errors and the dcvc_amd.metrics wrappers."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import msssim_np
from codec_util import dmci_model
from dcvc_amd import _lib, metrics, synthetic

pytestmark = pytest.mark.gpu

vp, ci = ctypes.c_void_p, ctypes.c_int
TOL = 1e-10


def _abi():
    return _lib.fn("dcvc_msssim", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ctypes.c_longlong, vp, vp])


def _cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "msssim_golden.npz"))
    names = sorted(k[:-len("_value")] for k in z.files if k.endswith("_value"))
    return [(n, z[n + "_src"], z[n + "_rec"], float(z[n + "_value"])) for n in names]


def _close(got, want, what):
    if math.isnan(want):
        assert math.isnan(got), what
    else:
        assert abs(got - want) <= TOL, (what, got, want)


def test_golden_cases_every_dtype(golden_dir):
    for name, src, rec, want in _cases(golden_dir):
        s8 = torch.from_numpy(src).cuda()
        r = torch.from_numpy(rec).cuda()
        # the fixture's dtypes (u8 source; fp16 or u8 reconstruction) and the source as fp16 (exact for 0..255)
        for a, b in [(s8, r), (s8.half(), r), (r, s8)]:
            if src.ndim == 3:
                got = metrics.msssim_rgb(a, b)
            else:
                got = float(metrics.msssim(a, b)[0])
            if name == "same_120x128":
                assert got == 1.0, (name, a.dtype, b.dtype, got)
            elif name == "inv_120x128":
                assert math.isnan(got)
            else:
                _close(got, want, (name, a.dtype, b.dtype))


def _gpu_intra():
    g = copy.deepcopy(dmci_model(skip_thres=0.15)).half().cuda()
    g.proxy = None
    return g


def _decoded_planes(g, y, uv, qp):
    """one intra picture through the codec, then dcvc_x_to_yuv420's fp16 distortion planes (get_distortion)"""
    H, W = y.shape
    x = synthetic.yuv420_to_x(y, uv).half().cuda().contiguous(memory_format=torch.channels_last)
    pr, pb = g.get_padding_size(H, W, 16)
    x_hat = g.compress(x, qp, pb, pr)["x_hat"]
    xh = x_hat[0].permute(1, 2, 0).contiguous()
    y16 = torch.empty((H, W), dtype=torch.float16, device="cuda")
    uv16 = torch.empty((2, H // 2, W // 2), dtype=torch.float16, device="cuda")
    fn = _lib.fn("dcvc_x_to_yuv420", ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp])
    _lib.check(fn(vp(xh.data_ptr()), xh.shape[1], H, W, vp(y16.data_ptr()), vp(uv16.data_ptr()), None, None,
                  vp(torch.cuda.current_stream().cuda_stream)))
    return y16, uv16


@pytest.mark.parametrize("H,W", [(1080, 1920), (2160, 3840)])
def test_decoded_pictures_against_numpy(H, W):
    y, uv = synthetic.synthetic_frame_yuv420(1080, 1920, index=0, seed=5)
    if H == 2160:         # tiled from 1080p pictures (the generator is slow at 8 M pixels)
        y2, uv2 = synthetic.synthetic_frame_yuv420(1080, 1920, index=1, seed=5)
        y = np.block([[y, y2], [y2, y]])
        uv = np.concatenate([np.block([[uv[i], uv2[i]], [uv2[i], uv[i]]])[None] for i in range(2)])
    y, uv = np.ascontiguousarray(y), np.ascontiguousarray(uv)
    g = _gpu_intra()
    y16, uv16 = _decoded_planes(g, y, uv, qp=40)
    got = metrics.msssim_yuv420(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda(), y16, uv16)
    yr, uvr = y16.cpu().numpy(), uv16.cpu().numpy()
    want = [msssim_np.msssim(y, yr), msssim_np.msssim(uv[0], uvr[0]), msssim_np.msssim(uv[1], uvr[1])]
    for k in range(3):
        _close(got[1 + k], want[k], ("plane", k))
    assert got[0] == (6 * got[1] + got[2] + got[3]) / 8
    # synthetic weights reconstruct poorly (PSNR ~16 dB): a low but finite value, not the identity case
    assert all(math.isfinite(v) and v < 1.0 for v in got)


def _pair(P, H, W, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (P, H, W), dtype=np.uint8)
    rec = np.clip(src + rng.normal(0, 20, src.shape), 0, 255).astype(np.float16)
    return torch.from_numpy(src).cuda(), torch.from_numpy(rec).cuda()


def test_batched_planes_equal_single_calls_and_repeat_bitwise():
    src, rec = _pair(3, 200, 300, 0)
    batched = metrics.msssim(src, rec)
    single = np.array([metrics.msssim(src[i], rec[i])[0] for i in range(3)])
    assert batched.tobytes() == single.tobytes()
    assert metrics.msssim(src, rec).tobytes() == batched.tobytes()
    # a plane stride with a gap between the planes (and rows wider than W): the same values
    big_s = torch.zeros((3, 210, 320), dtype=torch.uint8, device="cuda")
    big_r = torch.zeros((3, 210, 320), dtype=torch.float16, device="cuda")
    big_s[:, :200, :300], big_r[:, :200, :300] = src, rec
    assert metrics.msssim(big_s[:, :200, :300], big_r[:, :200, :300]).tobytes() == batched.tobytes()
    for i in range(3):
        _close(float(batched[i]), msssim_np.msssim(src[i].cpu().numpy(), rec[i].cpu().numpy()), i)


def test_non_default_stream_is_ordered_after_queued_work():
    src, rec = _pair(1, 540, 960, 1)
    want = metrics.msssim(src, rec)
    stale = torch.zeros_like(rec)
    big = torch.randn(4096, 4096, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(4):
            big = big @ big * 1e-3          # keeps the stream busy in front of the copy
        stale.copy_(rec)
        got = metrics.msssim(src, stale)
    assert got.tobytes() == want.tobytes()


def test_abi_errors_and_wrapper_agree_with_abi():
    f = _abi()
    src, rec = _pair(2, 120, 160, 2)
    out = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    args = lambda **kw: dict(dict(s=vp(src.data_ptr()), sd=0, r=vp(rec.data_ptr()), rd=1, n=2, H=120, W=160, rs=160,
                                  ps=120 * 160), **kw)
    call = lambda a: f(a["s"], a["sd"], a["r"], a["rd"], a["n"], a["H"], a["W"], a["rs"], a["ps"], vp(out.data_ptr()), st)
    assert call(args()) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == metrics.msssim(src, rec).tobytes()
    for bad, msg in [(dict(H=87), "88"), (dict(W=80, rs=80), "88"), (dict(sd=3), "sample type"), (dict(rd=-1), "sample type"),
                     (dict(rs=159), "row_stride")]:
        assert call(args(**bad)) == -1
        assert msg in _lib.lib().dcvc_last_error().decode()
    with pytest.raises(_lib.DcvcError, match="88"):
        metrics.msssim(src[:, :80], rec[:, :80])
    with pytest.raises(TypeError):
        metrics.msssim(src.float(), rec)
