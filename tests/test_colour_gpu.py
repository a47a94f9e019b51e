"""The colour-matrix / range kernels (rgb_cs.hip through dcvc_amd.rgb) on a real MI355X, bit for bit against the numpy
restatement (tests/colour_np.py): all 2^24 colours in packed and planar layouts, the element paths, a chunk slot and the
planar copy; x_hat with padded rows, the clamp edges and every fp16 bit pattern; the old entry points at bt709 / full; a
torch op chain for bt601 / limited; stream order on a non-default stream."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import colour_np
import rgb_np
from dcvc_amd import _lib, rgb

pytestmark = pytest.mark.gpu

COMBOS = [(m, r, d) for m in ("bt601", "bt709", "bt2020") for r, d in (("full", 8), ("limited", 8), ("limited", 10), ("limited", 16))]
vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong


@functools.lru_cache(maxsize=None)
def _cube():
    c = rgb_np.all_colours()                                        # [3, 4096, 4096]
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _small():
    """cube[:, :512, :512] on the host and on the device (planar): r 0..31, every g, every b"""
    c = np.ascontiguousarray(_cube()[:, :512, :512])
    c.setflags(write=False)
    return c, torch.from_numpy(c).cuda()


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _eq(a, b):
    """bit for bit; the payload of a NaN is not part of the definition: NaN must sit where NaN is expected"""
    a, b = _np(a), _np(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float16:
        na, nb = np.isnan(a), np.isnan(b)
        return np.array_equal(na, nb) and np.array_equal(a.view(np.uint16)[~na], b.view(np.uint16)[~nb])
    return np.array_equal(a, b)


@pytest.mark.parametrize("matrix,range_,depth", [("bt601", "limited", 8), ("bt2020", "limited", 10)])
def test_rgb_to_x_cs_all_colours_packed_and_planar(matrix, range_, depth):
    cube = _cube()
    kw = dict(matrix=matrix, range=range_, yuv_depth=depth)
    want = colour_np.rgb_to_x(cube, matrix, range_, depth)
    planar = torch.from_numpy(cube).cuda()
    packed = planar.permute(1, 2, 0).contiguous()
    x, copy = rgb.rgb_to_x(packed, planar=True, **kw)               # packed HWC, 16-B path, with the planar copy
    assert _eq(x, want) and _eq(copy, planar)
    assert _eq(rgb.rgb_to_x(planar, **kw), want)                    # planar CHW
    # element paths: a width that is no multiple of 8, and rows with a pitch
    x, copy = rgb.rgb_to_x(packed[:64, :1022], planar=True, **kw)
    assert _eq(x, want[:64, :1022]) and _eq(copy, planar[:, :64, :1022])
    assert _eq(rgb.rgb_to_x(planar[:, 8:72, 16:1040], **kw), want[8:72, 16:1040])


@pytest.mark.parametrize("matrix,range_,depth", COMBOS, ids=["%s-%s-%d" % c for c in COMBOS])
def test_rgb_to_x_cs_every_combination(matrix, range_, depth):
    host, planar = _small()
    kw = dict(matrix=matrix, range=range_, yuv_depth=depth)
    want = colour_np.rgb_to_x(host, matrix, range_, depth)
    assert _eq(rgb.rgb_to_x(planar.permute(1, 2, 0).contiguous(), **kw), want)
    assert _eq(rgb.rgb_to_x(planar, **kw), want)
    assert _eq(rgb.rgb_to_x(planar[:, 3:37, 5:507], **kw), want[3:37, 5:507])      # element path


def test_rgb_to_x_cs_chunk_slot():
    host, planar = _small()
    host, planar = host[:, :128], planar[:, :128]
    want = colour_np.rgb_to_x(host, "bt601", "limited", 8)
    H, W = 128, 512
    buf = torch.full((H, W, 24), 7.0, dtype=torch.float16, device="cuda")
    flat = buf.view(-1)
    for j in (0, 3, 7):
        rgb.rgb_to_x(planar.permute(1, 2, 0).contiguous(), ldx=24, x=flat[3 * j:], matrix="bt601", range="limited")
        assert _eq(buf[..., 3 * j:3 * j + 3], want), j
    untouched = [c for c in range(24) if c // 3 not in (0, 3, 7)]
    assert bool((buf[..., untouched] == 7.0).all())


def _x_hat(Hp, Wp, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x_hat = (torch.rand((Hp, Wp, 3), generator=g, device="cuda") * 1.5 - 0.75).half()
    edges = torch.tensor([-0.5, 0.5, -0.501, 0.499, 0.5005, -0.4995, 0.75, -0.75, 0.0, 0.25], dtype=torch.float16, device="cuda")
    x_hat[0, :edges.numel()] = edges[:, None]
    x_hat[1, :edges.numel()] = edges.flip(0)[:, None]
    return x_hat


@pytest.mark.parametrize("H,W,Hp,Wp", [(16, 24, 16, 32), (14, 22, 16, 32)])        # the vector path; the element path and the crop
def test_x_to_rgb_cs_random_and_clamp_edges(H, W, Hp, Wp):
    x_hat = _x_hat(Hp, Wp, H + W)
    host = x_hat.cpu().numpy()
    seen0 = seen255 = False
    for matrix, range_, depth in COMBOS:
        want16, want8 = colour_np.x_to_rgb(host, H, W, matrix, range_, depth)
        got16, got8 = rgb.x_to_rgb(x_hat, H, W, matrix=matrix, range=range_, yuv_depth=depth)
        assert _eq(got16, want16) and _eq(got8, want8), (matrix, range_, depth)
        got16b, got8b = rgb.x_to_rgb(x_hat.permute(2, 0, 1).unsqueeze(0), H, W, matrix=matrix, range=range_, yuv_depth=depth)
        assert _eq(got16b, want16) and _eq(got8b, want8), (matrix, range_, depth)
        seen0, seen255 = seen0 or bool((got8 == 0).any()), seen255 or bool((got8 == 255).any())
    assert seen0 and seen255


@pytest.mark.parametrize("matrix,range_,depth", [("bt601", "limited", 8), ("bt2020", "limited", 10), ("bt601", "full", 8)])
def test_x_to_rgb_cs_every_fp16_pattern(matrix, range_, depth):
    """256 x 256: each channel runs through all 65536 fp16 patterns (NaN, +-Inf, subnormals) in its own order"""
    i = np.arange(65536, dtype=np.uint32)
    pat = np.stack([i, 65535 - i, (i * 40503 + 12345) & 65535], axis=-1).astype(np.uint16).reshape(256, 256, 3)
    host = pat.view(np.float16)
    want16, want8 = colour_np.x_to_rgb(host, 256, 256, matrix, range_, depth)
    got16, got8 = rgb.x_to_rgb(torch.from_numpy(host).cuda(), 256, 256, matrix=matrix, range=range_, yuv_depth=depth)
    assert _eq(got16, want16) and _eq(got8, want8)
    nan = np.isnan(want16).transpose(1, 2, 0)
    assert nan.any() and (_np(got8)[nan] == 0).all()
    assert (_np(got8) == 0).any() and (_np(got8) == 255).any()
    assert bool((got16 == 0).any()) and bool((got16 == 255).any())


def test_old_and_new_entry_points_agree_at_bt709_full():
    """dcvc_rgb_to_x_cs / dcvc_x_to_rgb_cs at (DCVC_MATRIX_BT709, DCVC_RANGE_FULL, 8) through ctypes - dcvc_amd.rgb sends the
    defaults to the old entry points - against dcvc_rgb_to_x / dcvc_x_to_rgb"""
    to_x = _lib.fn("dcvc_rgb_to_x_cs", ci, [vp, ll, ll, ll, ci, ci, vp, ci, vp, ci, ci, ci, vp])
    to_rgb = _lib.fn("dcvc_x_to_rgb_cs", ci, [vp, ci, ci, ci, vp, vp, ci, ci, ci, vp])
    st = vp(torch.cuda.current_stream().cuda_stream)
    planar = torch.from_numpy(_cube()).cuda()
    packed = planar.permute(1, 2, 0).contiguous()
    H = W = 4096
    for src, strides in ((packed, (3 * W, 3, 1)), (planar, (W, 1, H * W))):
        x = torch.empty((H, W, 3), dtype=torch.float16, device="cuda")
        _lib.check(to_x(vp(src.data_ptr()), *strides, H, W, vp(x.data_ptr()), 3, None, 1, 0, 8, st))
        assert _eq(x, rgb.rgb_to_x(src))
    for Hc, Wc, x_hat in ((4096, 4096, x), (270, 490, _x_hat(272, 496, 3))):
        r16 = torch.empty((3, Hc, Wc), dtype=torch.float16, device="cuda")
        r8 = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device="cuda")
        _lib.check(to_rgb(vp(x_hat.data_ptr()), x_hat.shape[1], Hc, Wc, vp(r16.data_ptr()), vp(r8.data_ptr()), 1, 0, 8, st))
        old16, old8 = rgb.x_to_rgb(x_hat, Hc, Wc)
        assert _eq(r16, old16) and _eq(r8, old8)
    # and through the wrappers, which reach the new entry points in full range at another depth (ignored there)
    host, small = _small()
    assert _eq(rgb.rgb_to_x(small, yuv_depth=10), rgb.rgb_to_x(small))


def test_a_torch_op_chain_equals_the_kernel_at_bt601_limited():
    """test_rgb_gpu.py's _torch_rgb_to_x with the BT.601 constants and the two extra steps, as torch evaluates it on the GPU"""
    KR, KG, KB = colour_np.MATRICES["bt601"]
    host, planar = _small()
    x = planar.unsqueeze(0).float() / 255.0
    r, g, b = x.chunk(3, -3)
    y = KR * r + KG * g + KB * b
    pb = 0.5 * (b - y) / (1 - KB)
    pr = 0.5 * (r - y) / (1 - KR)
    ycc = torch.cat((y * (219 / 255) + 16 / 255, pb * (224 / 255) + 128 / 255, pr * (224 / 255) + 128 / 255), dim=-3)
    want = (torch.clamp(ycc, 0., 1.).half() - 0.5)[0].permute(1, 2, 0)
    assert _eq(want, colour_np.rgb_to_x(host, "bt601", "limited", 8))
    assert _eq(rgb.rgb_to_x(planar, matrix="bt601", range="limited"), want)
    # the inverse chain on the kernel's own x
    t = want.permute(2, 0, 1).unsqueeze(0) + 0.5
    Y, cb, cr = t.float().chunk(3, -3)
    y, pb, pr = (Y - 16 / 255) * (255 / 219), (cb - 128 / 255) * (255 / 224), (cr - 128 / 255) * (255 / 224)
    r = y + (2 - 2 * KR) * pr
    b = y + (2 - 2 * KB) * pb
    g = (y - KR * r - KB * b) / KG
    rec16 = torch.clamp(torch.clamp(torch.cat((r, g, b), dim=-3), 0., 1.).half() * 255, 0, 255)
    got16, got8 = rgb.x_to_rgb(want.contiguous(), 512, 512, matrix="bt601", range="limited")
    assert _eq(got16, rec16[0]) and _eq(got8, rec16.round().byte()[0].permute(1, 2, 0))
    assert _eq(got8, planar.permute(1, 2, 0))                       # the round trip


def test_stream_order_on_a_non_default_stream():
    host, planar = _small()
    kw = dict(matrix="bt2020", range="limited", yuv_depth=10)
    want = colour_np.rgb_to_x(host, "bt2020", "limited", 10)
    want16, want8 = colour_np.x_to_rgb(want, 512, 512, "bt2020", "limited", 10)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        src = planar.permute(1, 2, 0).contiguous() + 0              # produced on s, consumed on s without a host sync
        x = rgb.rgb_to_x(src, **kw)
        x16, x8 = rgb.x_to_rgb(x, 512, 512, **kw)
    s.synchronize()
    assert _eq(x, want) and _eq(x16, want16) and _eq(x8, want8)
