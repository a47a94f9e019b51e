"""The numpy restatement of the other chroma formats (tests/pixfmt_np.py) tied to what is already pinned: YUV420P at 8 bits is
oracle/frame_io.py and the reference-made vectors of tests/golden/io_golden.npz (truncated chroma included), YUV420P at 9..16
bits is tests/yuv16_np.py, NV12 is YUV420P after de-interleaving and the 16 - b shift, 4:4:4 chroma follows the luma rule and
the 4:2:2 mean lies within half an fp16 ulp of the fp64 mean. No GPU, no library."""
import os

import numpy as np
import pytest

import pixfmt_np as pn
import yuv16_np

f16, f32 = np.float16, np.float32


def _picture(fmt, bits, H, W, seed=0):
    rng = np.random.default_rng(seed)
    (_, _), (hc, wc) = pn.plane_shapes(fmt, H, W)
    y = rng.integers(0, 1 << bits, (H, W)).astype(pn.dtype(bits))
    c = rng.integers(0, 1 << bits, (2, hc, wc)).astype(pn.dtype(bits))
    return y, c


def _x_hat(H, W, seed=1):
    rng = np.random.default_rng(seed)
    return (rng.random((H + 6, W + 8, 3), dtype=f32) * f32(1.3) - f32(0.65)).astype(f16)


def test_picture_samples_and_shapes():
    assert pn.picture_samples(pn.YUV420P, 4, 6) == 36 and pn.picture_samples(pn.NV12, 4, 6) == 36
    assert pn.picture_samples(pn.YUV422P, 4, 6) == 48 and pn.picture_samples(pn.YUV444P, 4, 6) == 72
    assert pn.plane_shapes(pn.YUV422P, 4, 6) == ((4, 6), (4, 3)) and pn.plane_shapes(pn.NV12, 4, 6) == ((4, 6), (2, 3))


def test_yuv420p_8_bits_is_the_oracle_and_the_reference_vectors(golden_dir):
    from oracle import frame_io
    g = np.load(os.path.join(golden_dir, "io_golden.npz"))
    y, uv = g["y"], g["uv"]
    H, W = y.shape
    pic = pn.pack(y, uv, pn.YUV420P, 8)
    assert pic.tobytes() == y.tobytes() + uv.tobytes()
    x = pn.to_x(pic, pn.YUV420P, 8, H, W)
    assert np.array_equal(x, g["x"]) and np.array_equal(x, frame_io.yuv420_to_x(y, uv))
    dist, samples = pn.from_x(g["x_hat"], H, W, pn.YUV420P, 8)
    assert np.array_equal(dist[:H * W].reshape(H, W), g["y16"].astype(f32))
    assert np.array_equal(dist[H * W:].reshape(uv.shape), g["uv16"].astype(f32))
    assert samples.tobytes() == g["y8"].tobytes() + g["uv8"].tobytes()              # uv8: the reference writer's truncation
    xh = _x_hat(18, 40)
    o = frame_io.x_to_yuv420(xh, 18, 40)
    dist, samples = pn.from_x(xh, 18, 40, pn.YUV420P, 8)
    assert np.array_equal(dist, np.concatenate([o["y16"].ravel(), o["uv16"].ravel()]).astype(f32))
    assert samples.tobytes() == o["y8"].tobytes() + o["uv8"].tobytes()
    assert not np.array_equal(o["uv8"], np.rint(o["uv16"].astype(f32)).astype(np.uint8)), "the case must tell truncation from rounding"


@pytest.mark.parametrize("bits", [9, 10, 12, 16])
def test_yuv420p_high_bit_depth_is_yuv16_np(bits):
    H, W = 18, 40
    y, uv = _picture(pn.YUV420P, bits, H, W)
    pic = pn.pack(y, uv, pn.YUV420P, bits)
    assert np.array_equal(pn.to_x(pic, pn.YUV420P, bits, H, W), yuv16_np.yuv420p16_to_x(y, uv, bits))
    xh = _x_hat(H, W)
    dy, duv, y16, uv16 = yuv16_np.x_to_yuv420p16(xh, H, W, bits)
    dist, samples = pn.from_x(xh, H, W, pn.YUV420P, bits)
    assert np.array_equal(dist, np.concatenate([dy.ravel(), duv.ravel()]))
    assert samples.tobytes() == y16.astype("<u2").tobytes() + uv16.astype("<u2").tobytes()


@pytest.mark.parametrize("bits", [8, 10, 16])
def test_nv12_is_yuv420p_deinterleaved_and_shifted(bits):
    H, W = 18, 40
    y, uv = _picture(pn.NV12, bits, H, W)
    s = 16 - bits if bits > 8 else 0
    nv = pn.pack(y, uv, pn.NV12, bits)
    # the layout, spelled out: Y, then Cb Cr pairs, the value in the high bits
    assert np.array_equal(nv[:H * W].reshape(H, W), y << s)
    assert np.array_equal(nv[H * W::2].reshape(H // 2, W // 2), uv[0] << s) and np.array_equal(nv[H * W + 1::2].reshape(H // 2, W // 2), uv[1] << s)
    low = nv | (np.arange(nv.size) % (1 << s)).astype(nv.dtype) if s else nv       # P010: the low bits are ignored
    planar = pn.pack(y, uv, pn.YUV420P, bits)
    assert np.array_equal(pn.to_x(low, pn.NV12, bits, H, W), pn.to_x(planar, pn.YUV420P, bits, H, W))
    assert np.array_equal(pn.planar(low, pn.NV12, bits, H, W), planar)
    xh = _x_hat(H, W)
    d_nv, s_nv = pn.from_x(xh, H, W, pn.NV12, bits)
    d_pl, s_pl = pn.from_x(xh, H, W, pn.YUV420P, bits)
    assert np.array_equal(d_nv, d_pl)
    yy, cc = pn.unpack(s_nv, pn.NV12, bits, H, W)
    assert np.array_equal(np.concatenate([yy.ravel(), cc.ravel()]), s_pl)
    assert np.array_equal(s_nv & ((1 << s) - 1), np.zeros_like(s_nv))


@pytest.mark.parametrize("bits", [8, 10])
def test_444_chroma_follows_the_luma_rule(bits):
    H, W = 6, 10
    y, c = _picture(pn.YUV444P, bits, H, W)
    x = pn.to_x(pn.pack(y, c, pn.YUV444P, bits), pn.YUV444P, bits, H, W)
    same = pn.to_x(pn.pack(c[0], np.stack([y, c[1]]), pn.YUV444P, bits), pn.YUV444P, bits, H, W)
    assert np.array_equal(x[..., 1], same[..., 0]) and np.array_equal(x[..., 0], same[..., 1])
    xh = _x_hat(H, W)
    dist, samples = pn.from_x(xh, H, W, pn.YUV444P, bits)
    swapped = np.ascontiguousarray(xh[..., [1, 0, 2]])
    d2, s2 = pn.from_x(swapped, H, W, pn.YUV444P, bits)
    n = H * W
    assert np.array_equal(dist[n:2 * n], d2[:n]) and np.array_equal(samples[n:2 * n], s2[:n])       # Cb as luma: rint, no truncation


def test_422_mean_is_within_half_an_fp16_ulp_of_the_fp64_mean():
    rng = np.random.default_rng(3)
    t = rng.random((64, 128, 3)).astype(f16)
    got = pn.chroma_t(t, pn.YUV422P).astype(np.float64)
    c = t[..., 1:].astype(np.float64).transpose(2, 0, 1)
    want = (c[:, :, 0::2] + c[:, :, 1::2]) / 2
    ulp = np.spacing(np.abs(got).astype(f16)).astype(np.float64)
    assert got.shape == (2, 64, 64) and np.all(np.abs(got - want) <= 0.5 * ulp)
    # and 4:2:2 / 4:4:4 round every plane half to even: no truncated chroma outside the 4:2:0 layouts
    xh = _x_hat(6, 16)
    for fmt in (pn.YUV422P, pn.YUV444P):
        dist, samples = pn.from_x(xh, 6, 16, fmt, 8)
        assert np.array_equal(samples, np.rint(dist).astype(np.uint8))


def test_nan_and_infinities_give_defined_samples():
    xh = pn.all_halfs()
    for fmt in pn.FORMATS:
        for bits in (8, 10):
            dist, samples = pn.from_x(xh, 256, 256, fmt, bits)
            assert np.all(np.isfinite(dist)) and dist.min() >= 0 and dist.max() <= pn.max_val(bits)
