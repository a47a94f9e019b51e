"""dcvc_msssim_range_ws on a real MI355X: MS-SSIM on a workspace the caller owns gives the bits of dcvc_msssim_range and of
dcvc_msssim (data_range 255), call after call on one workspace, and refuses a workspace that is missing, too small or
misaligned before anything is enqueued. dcvc decode --out-size measures every picture through it."""
import ctypes

import numpy as np
import pytest
import torch

import msssim_np
from dcvc_amd import _lib, yuv16

pytestmark = pytest.mark.gpu

vp, ci, ll, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double


def _fns():
    size = _lib.fn("dcvc_msssim_workspace_bytes", ll, [ci, ci, ci])
    run = _lib.fn("dcvc_msssim_range_ws", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, dbl, vp, vp, ll, vp])
    return size, run


def test_the_callers_workspace_gives_the_bits_of_the_allocating_entries():
    size, run = _fns()
    rng = np.random.default_rng(21)
    H, W = 180, 200
    src = rng.integers(0, 256, (2, H, W)).astype(np.uint8)
    rec = np.clip(src.astype(np.int64) + rng.integers(-9, 10, src.shape), 0, 255).astype(np.uint8)
    s, r = torch.from_numpy(src).cuda(), torch.from_numpy(rec).cuda()
    need = size(2, H, W)
    assert need > 0 and size(1, H, W) <= need and size(1, 87, W) == 0 and size(0, H, W) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    stream = vp(torch.cuda.current_stream().cuda_stream)
    want = yuv16.msssim(s, r, 255.0)
    for _ in range(3):                                           # one workspace, call after call
        out.zero_()
        _lib.check(run(vp(s.data_ptr()), 0, vp(r.data_ptr()), 0, 2, H, W, W, H * W, 255.0, vp(out.data_ptr()), vp(ws.data_ptr()),
                       need, stream))
        got = out.cpu().numpy()
        assert got.tolist() == want.tolist()
    for p in range(2):
        assert abs(got[p] - msssim_np.msssim(src[p], rec[p])) <= 1e-10


def test_a_bad_workspace_is_refused():
    size, run = _fns()
    H, W = 96, 120
    s = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
    need = size(1, H, W)
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    out = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    stream = vp(torch.cuda.current_stream().cuda_stream)
    for w, n in ((None, need), (ws.data_ptr(), need - 1), (ws.data_ptr(), -1), (ws.data_ptr() + 8, need)):
        rc = run(vp(s.data_ptr()), 0, vp(s.data_ptr()), 0, 1, H, W, W, H * W, 255.0, vp(out.data_ptr()), w, n, stream)
        assert rc == -1 and "workspace" in _lib.lib().dcvc_last_error().decode(), (w, n)
    torch.cuda.synchronize()
    assert out.item() == 7.0
