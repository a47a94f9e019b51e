"""dcvc_luma_sad (csrc/kernels/scene.hip) on a real MI355X (-m gpu) against tests/scene_np.py: the luma plane
bytewise and the SAD exactly, on every path of the kernel - 16-byte loads of packed pixels, the strided path of a chunk
slot, packed and bytewise plane accesses, ragged ends, several workgroups - past 32 bits, without a previous plane, back
to back on one stream, and through scene.luma_sad."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import scene_np
from dcvc_amd import _lib, scene

pytestmark = pytest.mark.gpu

vp, ci = ctypes.c_void_p, ctypes.c_int

# (H, W, ldx, offset of the luma channel in halfs from a 256-byte aligned base)
CASES = [
    (1, 1, 3, 0),
    (18, 22, 3, 0),
    (37, 53, 3, 0),
    (16, 24, 24, 15),        # a chunk slot, pointer not 16-byte aligned
    (144, 176, 6, 3),
    (270, 482, 3, 0),        # several workgroups and a ragged tail
]


def _fn():
    return _lib.fn("dcvc_luma_sad", ci, [vp, ci, ci, ci, vp, vp, vp, vp])


@functools.lru_cache(maxsize=None)
def _case(H, W, ldx, off):
    """(flat fp16 buffer, prev u8 [H, W], want luma u8 [H, W], want sad), numpy, made once per case"""
    rng = np.random.default_rng([H, W, ldx, off])
    buf = rng.uniform(-0.6, 0.6, off + H * W * ldx).astype(np.float16)      # beyond +-0.5: out of range, clamped
    special = np.float16([0.0, -0.0, 1.0, -1.0, 0.75, -0.75, 0.5, -0.5])     # the half-way products, far out of range, the ends
    at = rng.choice(H * W, size=min(H * W, 64), replace=False)
    buf[off + at * ldx] = special[np.arange(at.size) % special.size]
    prev = rng.integers(0, 256, (H, W), dtype=np.uint8)
    luma = scene_np.luma8(buf[off::ldx][:H * W]).reshape(H, W)
    return buf, prev, luma, scene_np.sad(luma, prev)


def _call(x, ldx, H, W, prev, luma, sad, stream=None):
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    _lib.check(_fn()(vp(x), ldx, H, W, None if prev is None else vp(prev), vp(luma), vp(sad), vp(s)))


def _filled_sad():
    return torch.full((1,), -1, dtype=torch.int64, device="cuda")        # 0xFF bytes: the call must not add to them


@pytest.mark.parametrize("with_prev", [True, False])
@pytest.mark.parametrize("H,W,ldx,off", CASES)
def test_luma_and_sad_equal_numpy(H, W, ldx, off, with_prev):
    buf, prev, want_luma, want_sad = _case(H, W, ldx, off)
    x, p = torch.from_numpy(buf).cuda(), torch.from_numpy(prev).cuda()
    assert x.data_ptr() % 256 == 0
    luma = torch.full((H, W), 0xA5, dtype=torch.uint8, device="cuda")
    sad = _filled_sad()
    _call(x.data_ptr() + 2 * off, ldx, H, W, p.data_ptr() if with_prev else None, luma.data_ptr(), sad.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(luma.cpu().numpy(), want_luma)
    assert int(sad.item()) == (want_sad if with_prev else 0)
    assert np.array_equal(p.cpu().numpy(), prev)


@pytest.mark.parametrize("H,W,ldx,off", [(37, 53, 3, 0), (16, 24, 24, 15)])
def test_unaligned_planes_take_the_byte_path(H, W, ldx, off):
    buf, prev, want_luma, want_sad = _case(H, W, ldx, off)
    x = torch.from_numpy(buf).cuda()
    p = torch.zeros(H * W + 8, dtype=torch.uint8, device="cuda")
    p[3:3 + H * W] = torch.from_numpy(prev.reshape(-1)).cuda()
    luma = torch.full((H * W + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    sad = _filled_sad()
    _call(x.data_ptr() + 2 * off, ldx, H, W, p.data_ptr() + 3, luma.data_ptr() + 5, sad.data_ptr())
    torch.cuda.synchronize()
    got = luma.cpu().numpy()
    assert np.array_equal(got[5:5 + H * W].reshape(H, W), want_luma)
    assert (got[:5] == 0xA5).all() and (got[5 + H * W:] == 0xA5).all()      # nothing beside the plane is written
    assert int(sad.item()) == want_sad


def test_sum_past_32_bits():
    H = W = 4200
    x = torch.full((H * W,), 0.5, dtype=torch.float16, device="cuda")
    prev = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    luma = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    sad = _filled_sad()
    _call(x.data_ptr(), 1, H, W, prev.data_ptr(), luma.data_ptr(), sad.data_ptr())
    torch.cuda.synchronize()
    assert int(sad.item()) == 255 * 4200 * 4200 == 4498200000
    assert int(luma.min().item()) == 255


def test_back_to_back_calls_on_one_stream():
    """picture 1 against a plane, picture 2 against picture 1's luma, ping-pong, with and without a synchronisation between"""
    H, W, ldx, off = 270, 482, 3, 0
    buf1, prev, luma1, sad1 = _case(H, W, ldx, off)
    buf2 = np.random.default_rng(7).uniform(-0.5, 0.5, buf1.size).astype(np.float16)
    luma2 = scene_np.luma8(buf2[off::ldx][:H * W]).reshape(H, W)
    sad2 = scene_np.sad(luma2, luma1)
    x1, x2, p = torch.from_numpy(buf1).cuda(), torch.from_numpy(buf2).cuda(), torch.from_numpy(prev).cuda()
    st = torch.cuda.Stream()
    results = []
    for sync in (False, True):
        planes = [p.clone(), torch.zeros((H, W), dtype=torch.uint8, device="cuda")]
        sads = [_filled_sad(), _filled_sad()]
        torch.cuda.synchronize()
        _call(x1.data_ptr(), ldx, H, W, planes[0].data_ptr(), planes[1].data_ptr(), sads[0].data_ptr(), st)
        if sync:
            st.synchronize()
        _call(x2.data_ptr(), ldx, H, W, planes[1].data_ptr(), planes[0].data_ptr(), sads[1].data_ptr(), st)
        st.synchronize()
        results.append((int(sads[0].item()), int(sads[1].item()), planes[1].cpu().numpy(), planes[0].cpu().numpy()))
    for got in results:
        assert got[:2] == (sad1, sad2)
        assert np.array_equal(got[2], luma1) and np.array_equal(got[3], luma2)


@pytest.mark.parametrize("H,W,ldx,off", CASES)
def test_python_wrapper_on_a_side_stream(H, W, ldx, off):
    buf, prev, want_luma, want_sad = _case(H, W, ldx, off)
    # the same memory as a channels_last model input: C = ldx channels, the luma in channel `off`
    x = torch.from_numpy(buf[:H * W * ldx].reshape(1, H, W, ldx)).cuda().permute(0, 3, 1, 2)
    assert off < ldx and x.shape == (1, ldx, H, W) and x.stride(1) == 1
    p = torch.from_numpy(prev).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        luma, sad = scene.luma_sad(x, p, channel=off)
        first, zero = scene.luma_sad(x, channel=off)
    st.synchronize()
    assert np.array_equal(luma.cpu().numpy(), want_luma) and sad == want_sad
    assert zero == 0 and np.array_equal(first.cpu().numpy(), want_luma)
