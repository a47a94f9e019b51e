"""The RGB picture kernels (rgb_cs.hip and sse.hip through dcvc_amd.rgb) on a real MI355X, against the reference's op chains evaluated by
torch on the GPU (test_video.py:55-64, 87-122; transforms.py:17-27, 53-66) and against the numpy restatement in the same
division convention (tests/rgb_np.py, div="recip"): bit for bit on all 2^24 colours in packed, planar and chunk-slot layouts,
on random and clamp-edge x_hat with padded rows; the fp64 sums of squares against numpy, their reproducibility across runs
and batch sizes, and stream order on a non-default stream."""
import ctypes

import numpy as np
import pytest
import torch

import rgb_np
from dcvc_amd import rgb

pytestmark = pytest.mark.gpu

KR, KG, KB = 0.2126, 0.7152, 0.0722


def _torch_rgb_to_x(u8_chw):
    """get_src_frame's png branch as torch ops on the GPU -> [H, W, 3] fp16"""
    x = u8_chw.unsqueeze(0).float() / 255.0
    r, g, b = x.chunk(3, -3)
    y = KR * r + KG * g + KB * b
    cb = 0.5 * (b - y) / (1 - KB) + 0.5
    cr = 0.5 * (r - y) / (1 - KR) + 0.5
    x = torch.clamp(torch.cat((y, cb, cr), dim=-3), 0., 1.).half() - 0.5
    return x[0].permute(1, 2, 0)


def _torch_x_to_rgb(x_hat_hw3, H, W):
    """get_distortion's png branch and the writer as torch ops on the GPU -> ([3, H, W] fp16, [H, W, 3] u8)"""
    t = x_hat_hw3[:H, :W].permute(2, 0, 1).unsqueeze(0) + 0.5
    y, cb, cr = t.float().chunk(3, -3)
    r = y + (2 - 2 * KR) * (cr - 0.5)
    b = y + (2 - 2 * KB) * (cb - 0.5)
    g = (y - KR * r - KB * b) / KG
    rec = torch.clamp(torch.cat((r, g, b), dim=-3), 0., 1.).half()
    rec16 = torch.clamp(rec * 255, 0, 255)
    return rec16[0], rec16.round().byte()[0].permute(1, 2, 0)


def _eq(a, b):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    b = b.cpu().numpy() if torch.is_tensor(b) else b
    if a.dtype == np.float16:
        a, b = a.view(np.uint16), b.view(np.uint16)
    return a.shape == b.shape and np.array_equal(a, b)


def test_rgb_to_x_all_colours_packed_and_planar():
    cube = rgb_np.all_colours()                                     # [3, 4096, 4096]
    planar = torch.from_numpy(cube).cuda()
    packed = planar.permute(1, 2, 0).contiguous()
    want = _torch_rgb_to_x(planar)
    assert _eq(want, rgb_np.rgb_to_x(cube, "recip"))                 # torch on the GPU multiplies by the reciprocal
    x, copy = rgb.rgb_to_x(packed, planar=True)                      # packed HWC, 16-B path
    assert _eq(x, want) and _eq(copy, planar)
    assert _eq(rgb.rgb_to_x(planar), want)                          # planar CHW
    assert _eq(rgb.rgb_to_x(packed.permute(2, 0, 1)), want)          # packed memory seen as [3, H, W]
    # element paths: a width that is no multiple of 8, and rows with a pitch
    assert _eq(rgb.rgb_to_x(packed[:64, :1022]), want[:64, :1022])
    assert _eq(rgb.rgb_to_x(planar[:, 8:72, 16:1040]), want[8:72, 16:1040])


def test_rgb_to_x_chunk_slot():
    cube = torch.from_numpy(rgb_np.all_colours()[:, :256, :512]).cuda()
    want = _torch_rgb_to_x(cube)
    H, W = 256, 512
    buf = torch.full((H, W, 24), 7.0, dtype=torch.float16, device="cuda")
    flat = buf.view(-1)
    for j in (0, 3, 7):
        rgb.rgb_to_x(cube.permute(1, 2, 0).contiguous(), ldx=24, x=flat[3 * j:])
        assert _eq(buf[..., 3 * j:3 * j + 3], want), j
    untouched = [c for c in range(24) if c // 3 not in (0, 3, 7)]
    assert bool((buf[..., untouched] == 7.0).all())


@pytest.mark.parametrize("H,W,Hp,Wp", [(256, 480, 272, 496), (270, 490, 272, 496), (1080, 1920, 1088, 1920)])
def test_x_to_rgb_random_and_clamp_edges(H, W, Hp, Wp):
    g = torch.Generator(device="cuda").manual_seed(H + W)
    x_hat = (torch.rand((Hp, Wp, 3), generator=g, device="cuda") * 1.5 - 0.75).half()
    edges = torch.tensor([-0.5, 0.5, -0.501, 0.499, 0.5005, -0.4995, 0.75, -0.75, 0.0, 0.25], dtype=torch.float16, device="cuda")
    x_hat[0, :edges.numel()] = edges[:, None]
    x_hat[1, :edges.numel()] = edges.flip(0)[:, None]
    want16, want8 = _torch_x_to_rgb(x_hat, H, W)
    n16, n8 = rgb_np.x_to_rgb(x_hat.cpu().numpy(), H, W, "recip")
    assert _eq(want16, n16) and _eq(want8, n8)
    assert bool((want16 == 0).any()) and bool((want16 == 255).any())
    got16, got8 = rgb.x_to_rgb(x_hat, H, W)
    assert _eq(got16, want16) and _eq(got8, want8)
    got16b, got8b = rgb.x_to_rgb(x_hat.permute(2, 0, 1).unsqueeze(0), H, W)     # [1, 3, Hp, Wp] channels-last view
    assert _eq(got16b, want16) and _eq(got8b, want8)


def test_sse_against_numpy_and_reproducible():
    g = torch.Generator(device="cuda").manual_seed(1)
    src = torch.randint(0, 256, (3, 1080, 1920), generator=g, device="cuda", dtype=torch.uint8)
    rec16 = (src.float() + torch.randn(src.shape, generator=g, device="cuda") * 4).clamp(0, 255).half()
    rec8 = rec16.round().byte()
    s64 = src.cpu().numpy().astype(np.float64)
    for rec in (rec16, rec8):
        want = ((s64 - rec.cpu().numpy().astype(np.float64)) ** 2).sum(axis=(1, 2))
        got = rgb.sse(src, rec)
        assert np.allclose(got, want, rtol=1e-9, atol=0), (got, want)
        again = rgb.sse(src, rec)
        assert got.tobytes() == again.tobytes()
        single = np.array([rgb.sse(src[c], rec[c])[0] for c in range(3)])
        assert got.tobytes() == single.tobytes()                      # one plane per call = three planes per call
        assert rgb.sse(src[:2], rec[:2]).tobytes() == got[:2].tobytes()
    assert rgb.sse(rec16, rec16).tolist() == [0.0, 0.0, 0.0]
    # the caller-workspace entry gives the same bits, call after call on one workspace
    from dcvc_amd import _lib
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    f = _lib.fn("dcvc_sse_ws", ci, [vp, ci, vp, ci, ci, ci, ci, ci, ll, vp, vp, ll, vp])
    nbytes = _lib.fn("dcvc_sse_workspace_bytes", ll, [ci, ci, ci])(3, 1080, 1920)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    for rec in (rec16, rec8, rec16):
        _lib.check(f(vp(src.data_ptr()), 0, vp(rec.data_ptr()), 1 if rec.dtype == torch.float16 else 0, 3, 1080, 1920, 1920,
                     1080 * 1920, vp(out.data_ptr()), vp(ws.data_ptr()), nbytes, st))
        assert out.cpu().numpy().tobytes() == rgb.sse(src, rec).tobytes()
    # element path: a width that is no multiple of 8
    want = ((s64[:, :100, :1914] - rec16[:, :100, :1914].cpu().numpy().astype(np.float64)) ** 2).sum(axis=(1, 2))
    assert np.allclose(rgb.sse(src[:, :100, :1914], rec16[:, :100, :1914]), want, rtol=1e-9, atol=0)
    # calc_psnr semantics
    p = rgb.psnr_rgb(src, rec16)
    mse = float(((s64 - rec16.cpu().numpy().astype(np.float64)) ** 2).mean())
    assert abs(p - 10 * np.log10(255.0 ** 2 / mse)) < 1e-9
    assert rgb.psnr_rgb(src, src.half()) == 99.9


def test_stream_order_on_a_non_default_stream():
    s = torch.cuda.Stream()
    cube = torch.from_numpy(rgb_np.all_colours()).cuda()
    want = _torch_rgb_to_x(cube)
    want16, want8 = _torch_x_to_rgb(want, 4096, 4096)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        src = cube.permute(1, 2, 0).contiguous() + 0           # produced on s, consumed on s without a host sync
        x = rgb.rgb_to_x(src)
        x16, x8 = rgb.x_to_rgb(x, 4096, 4096)
        total = rgb.sse(cube, x16)
    s.synchronize()
    assert _eq(x, want) and _eq(x16, want16) and _eq(x8, want8)
    ref = ((cube.cpu().numpy().astype(np.float64) - want16.cpu().numpy().astype(np.float64)) ** 2).sum(axis=(1, 2))
    assert np.allclose(total, ref, rtol=1e-9, atol=0)
