"""The high-bit-depth YUV420 kernels (picture_yuv.hip through dcvc_amd.yuv16) on a real MI355X, against the numpy restatement
(tests/yuv16_np.py): yuv420p16_to_x bit for bit over every code at 10, 12 and 16 bits in the packed (ldx = 3) and chunk-slot
layouts, x_to_yuv420p16 bit for bit on random and clamp-edge x_hat with padded rows, the fp64 sums of squares with u16 / fp32
samples against numpy and their reproducibility, dcvc_msssim_range at 255 against dcvc_msssim, 10-bit MS-SSIM against a
restatement with a data range (tests/msssim_range_np.py), and stream order on a non-default stream."""
import numpy as np
import pytest
import torch

import msssim_range_np
import yuv16_np
from dcvc_amd import metrics, yuv16

pytestmark = pytest.mark.gpu


def _dev(a):
    """a uint16 numpy array as int16 storage on the GPU (read as unsigned by the kernels)"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _host(t):
    a = t.cpu().view(torch.int16).numpy() if t.dtype != torch.float16 and t.element_size() == 2 else t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _eq(a, b):
    a = _host(a) if torch.is_tensor(a) else a
    b = _host(b) if torch.is_tensor(b) else b
    if a.dtype == np.float16:
        a, b = a.view(np.uint16), b.view(np.uint16)
    elif a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("bits", [10, 12, 16])
def test_yuv420p16_to_x_all_codes(bits):
    y, uv = yuv16_np.all_codes(bits)                      # W = 512: the 16-B path
    want = yuv16_np.yuv420p16_to_x(y, uv, bits)
    assert _eq(yuv16.yuv420p16_to_x(_dev(y), _dev(uv), bits), want)
    if hasattr(torch, "uint16"):                          # the same bits through torch.uint16 tensors
        yt = torch.from_numpy(y).cuda()
        uvt = torch.from_numpy(uv).cuda()
        assert _eq(yuv16.yuv420p16_to_x(yt, uvt, bits), want)
    # element path: a width that is no multiple of 8
    yc, uvc = np.ascontiguousarray(y[:, :500]), np.ascontiguousarray(uv[:, :, :250])
    assert _eq(yuv16.yuv420p16_to_x(_dev(yc), _dev(uvc), bits), yuv16_np.yuv420p16_to_x(yc, uvc, bits))
    # chunk slots at ldx = 24
    H, W = y.shape
    buf = torch.full((H, W, 24), 7.0, dtype=torch.float16, device="cuda")
    flat = buf.view(-1)
    for j in (0, 3, 7):
        yuv16.yuv420p16_to_x(_dev(y), _dev(uv), bits, ldx=24, x=flat[3 * j:])
        assert _eq(buf[..., 3 * j:3 * j + 3].contiguous(), want), j
    untouched = [c for c in range(24) if c // 3 not in (0, 3, 7)]
    assert bool((buf[..., untouched] == 7.0).all())


@pytest.mark.parametrize("H,W,Hp,Wp", [(256, 480, 272, 496), (270, 490, 272, 496), (1080, 1920, 1088, 1920)])
@pytest.mark.parametrize("bits", [10, 16])
def test_x_to_yuv420p16_random_and_clamp_edges(H, W, Hp, Wp, bits):
    g = torch.Generator(device="cuda").manual_seed(H + W + bits)
    x_hat = (torch.rand((Hp, Wp, 3), generator=g, device="cuda") * 1.5 - 0.75).half()
    edges = torch.tensor([-0.5, 0.5, -0.501, 0.499, 0.5005, -0.4995, 0.75, -0.75, 0.0, 0.25], dtype=torch.float16, device="cuda")
    x_hat[0, :edges.numel()] = edges[:, None]
    x_hat[1, :edges.numel()] = edges.flip(0)[:, None]
    want = yuv16_np.x_to_yuv420p16(x_hat.cpu().numpy(), H, W, bits)
    m = (1 << bits) - 1
    assert (want[0] == 0).any() and (want[0] == m).any() and (want[1] == 0).any() and (want[1] == m).any()
    got = yuv16.x_to_yuv420p16(x_hat, H, W, bits)
    for a, b in zip(got, want):
        assert _eq(a, b)
    got_cl = yuv16.x_to_yuv420p16(x_hat.permute(2, 0, 1).unsqueeze(0), H, W, bits)      # [1, 3, Hp, Wp] channels-last view
    for a, b in zip(got_cl, want):
        assert _eq(a, b)


def test_sse_u16_f32_against_numpy_and_reproducible():
    g = torch.Generator(device="cuda").manual_seed(2)
    src16 = torch.randint(0, 1024, (3, 540, 960), generator=g, device="cuda", dtype=torch.int32)
    rec32 = (src16.float() + torch.randn(src16.shape, generator=g, device="cuda") * 5).clamp(0, 1023)
    src = src16.to(torch.int16)
    rec16 = rec32.round().to(torch.int16)
    s64 = src16.cpu().numpy().astype(np.float64)
    for rec, r64 in ((rec32, rec32.cpu().numpy().astype(np.float64)), (rec16, rec32.round().cpu().numpy().astype(np.float64))):
        want = ((s64 - r64) ** 2).sum(axis=(1, 2))
        got = yuv16.sse(src, rec)
        assert np.allclose(got, want, rtol=1e-12, atol=0), (got, want)
        assert got.tobytes() == yuv16.sse(src, rec).tobytes()
        single = np.array([yuv16.sse(src[c], rec[c])[0] for c in range(3)])
        assert got.tobytes() == single.tobytes()
    # fp32 against u16 (operands swapped), and samples above 32767 are read as unsigned
    assert yuv16.sse(rec32, src).tobytes() == yuv16.sse(src, rec32).tobytes()
    hi = torch.full((8, 16), -1, dtype=torch.int16, device="cuda")            # 65535
    assert yuv16.sse(hi, torch.zeros((8, 16), dtype=torch.float32, device="cuda"))[0] == 128 * 65535.0 ** 2
    # element path: a width that is no multiple of 8
    want = ((s64[:, :100, :954] - rec32[:, :100, :954].cpu().numpy().astype(np.float64)) ** 2).sum(axis=(1, 2))
    assert np.allclose(yuv16.sse(src[:, :100, :954], rec32[:, :100, :954]), want, rtol=1e-12, atol=0)
    # the PSNR wrapper
    y, uv = src[0, :540, :960], src[1:, :270, :480].contiguous()
    dy, duv = rec32[0], rec32[1:, :270, :480].contiguous()
    want = yuv16_np.psnr_yuv420(_host(y), _host(uv), dy.cpu().numpy(), duv.cpu().numpy(), 10)
    got = yuv16.psnr_yuv420p16(y, uv, dy, duv, 10)
    assert np.allclose(got, want, rtol=1e-12, atol=0)


def test_msssim_range_255_equals_msssim_and_10_bit_against_numpy():
    g = torch.Generator(device="cuda").manual_seed(3)
    src8 = torch.randint(0, 256, (2, 192, 176), generator=g, device="cuda", dtype=torch.uint8)
    rec16 = (src8.float() + torch.randn(src8.shape, generator=g, device="cuda") * 8).clamp(0, 255).half()
    for a, b in ((src8, rec16), (src8, rec16.round().byte()), (rec16, src8), (rec16, rec16.flip(1).contiguous())):
        assert yuv16.msssim(a, b, 255).tobytes() == metrics.msssim(a, b).tobytes()
    # 10 bit: a smooth picture, so that the metric is far from 0 and 1
    yy, xx = torch.meshgrid(torch.arange(192, device="cuda"), torch.arange(208, device="cuda"), indexing="ij")
    base = 512 + 300 * torch.sin(yy / 9.0) * torch.cos(xx / 13.0)
    src = base.round().clamp(0, 1023).to(torch.int16)
    rec = (base + torch.randn(base.shape, generator=g, device="cuda") * 12).clamp(0, 1023).float()
    got = float(yuv16.msssim(src, rec, 1023)[0])
    want = msssim_range_np.msssim(_host(src).astype(np.float64), rec.cpu().numpy(), 1023.0)
    assert abs(got - want) <= 1e-10, (got, want)
    assert abs(got - float(yuv16.msssim(src, rec, 255)[0])) > 1e-4        # the range matters
    # the picture wrapper: 5 levels on Y, 4 on the chroma planes
    uv = src[:96 * 2].reshape(2, 96, 208)[:, :, :104].contiguous()
    duv = rec[:96 * 2].reshape(2, 96, 208)[:, :, :104].contiguous()
    v = yuv16.msssim_yuv420p16(src, uv, rec, duv, 10)
    assert abs(v[1] - want) <= 1e-10 and v[0] == (6 * v[1] + v[2] + v[3]) / 8
    assert abs(v[2] - msssim_range_np.msssim(_host(uv[0]).astype(np.float64), duv[0].cpu().numpy(), 1023.0)) <= 1e-10


def test_stream_order_on_a_non_default_stream():
    s = torch.cuda.Stream()
    y, uv = yuv16_np.all_codes(16)                     # 512 x 512
    want_x = yuv16_np.yuv420p16_to_x(y, uv, 16)
    want = yuv16_np.x_to_yuv420p16(want_x, 512, 512, 12)
    yd, uvd = _dev(y), _dev(uv)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        y2, uv2 = yd + 0, uvd + 0                      # produced on s, consumed on s without a host sync
        x = yuv16.yuv420p16_to_x(y2, uv2, 16)
        dy, duv, y16, uv16 = yuv16.x_to_yuv420p16(x, 512, 512, 12)
        total = yuv16.sse(y16, dy)
    s.synchronize()
    assert _eq(x, want_x) and _eq(dy, want[0]) and _eq(duv, want[1]) and _eq(y16, want[2]) and _eq(uv16, want[3])
    assert np.allclose(total[0], yuv16_np.sse(want[2], want[0]), rtol=1e-12, atol=0)
