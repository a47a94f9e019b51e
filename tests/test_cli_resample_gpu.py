"""dcvc encode --scale / dcvc decode --out-size on a real MI355X, against the numpy restatement of the resampler
(tests/resample_np.py) around the tool's own unscaled paths: the stream of a --scale run is the stream of a run on the clip
pre-scaled in numpy (all-intra and LD, 8-bit and 10-bit, and once with a rate target), --out-size writes the resampled bytes
of what plain decode writes, the log's PSNR / MS-SSIM / bpp are those of the output samples at the output size, and --scale at
the source size changes nothing. Seeded synthetic weights and pictures; the clip is 352x288, three pictures."""
import json
import os
import subprocess

import numpy as np
import pytest

import msssim_np
import msssim_range_np
import resample_np
from codec_util import dmc_ld_model, dmci_model
from dcvc_amd import export_weights, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 288, 352, 3
h, w = 144, 176
SFX = ("", "_y", "_u", "_v")


def _run(args, check=True):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, check=check, capture_output=True, text=True, timeout=600)


def _pictures(bits, seed=9):
    """N pictures (y [H, W], uv [2, H/2, W/2]): the synthetic sequence, for bits > 8 scaled up with low-order noise (uint16)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(N):
        y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=seed)
        if bits > 8:
            s = 1 << (bits - 8)
            y, uv = ((p.astype(np.uint16) * s + rng.integers(0, s, p.shape)).astype(np.uint16) for p in (y, uv))
        out.append((np.ascontiguousarray(y), np.ascontiguousarray(uv)))
    return out


def _write(path, pics):
    with open(path, "wb") as f:
        for y, uv in pics:
            for p in (y, uv):
                f.write(p.astype("<u2").tobytes() if p.dtype == np.uint16 else p.tobytes())


def _read(path, hh, ww, bits):
    """the pictures of a raw YUV420 file -> [(y, uv)]"""
    dt = np.dtype("<u2") if bits > 8 else np.dtype(np.uint8)
    raw = np.fromfile(path, dtype=dt)
    per = hh * ww * 3 // 2
    assert raw.size % per == 0
    out = []
    for k in range(raw.size // per):
        pic = raw[k * per:(k + 1) * per]
        out.append((pic[:hh * ww].reshape(hh, ww), pic[hh * ww:].reshape(2, hh // 2, ww // 2)))
    return out


def _scaled(pics, hh, ww, bits):
    """every plane on its own, as the tool does it: Y to hh x ww, U and V to hh/2 x ww/2"""
    m = (1 << bits) - 1
    return [(resample_np.resample_plane(y, hh, ww, m),
             np.stack([resample_np.resample_plane(c, hh // 2, ww // 2, m) for c in uv])) for y, uv in pics]


def _models(tmp_path, inter):
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    args = ["--intra", str(tmp_path / "i.dcvw")]
    if inter:
        export_weights.write_dcvw(str(tmp_path / "p.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
        args += ["--inter", str(tmp_path / "p.dcvw")]
    return args


def _depth(bits):
    return ["--bit-depth", str(bits)] if bits > 8 else []


def _both_encodes(tmp_path, inter, bits, coding):
    pics = _pictures(bits)
    _write(tmp_path / "in.yuv", pics)
    _write(tmp_path / "small.yuv", _scaled(pics, h, w, bits))
    args = _models(tmp_path, inter) + _depth(bits) + coding
    r = _run(["encode"] + args + ["-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H), "--scale", "%dx%d" % (w, h),
                                  "-o", str(tmp_path / "scaled.bin")])
    assert "(%dx%d)" % (w, h) in r.stdout, r.stdout
    _run(["encode"] + args + ["-i", str(tmp_path / "small.yuv"), "-W", str(w), "-H", str(h), "-o", str(tmp_path / "pre.bin")])
    return (tmp_path / "scaled.bin").read_bytes(), (tmp_path / "pre.bin").read_bytes()


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("inter", [False, True], ids=["intra", "ld"])
def test_scale_writes_the_stream_of_the_prescaled_clip(tmp_path, inter, bits):
    got, want = _both_encodes(tmp_path, inter, bits, ["--qp-i", "30", "--qp-p", "36"])
    assert len(want) > 100 and got == want


def test_scale_with_a_rate_target(tmp_path):
    got, want = _both_encodes(tmp_path, False, 8, ["--target-bpp", "0.4", "--rc-log", str(tmp_path / "rc.json")])
    assert got == want
    log = json.loads((tmp_path / "rc.json").read_text())
    assert (log["width"], log["height"], log["pictures"]) == (w, h, N)       # the controller saw the coded size


def test_scale_at_the_source_size_changes_nothing(tmp_path):
    _write(tmp_path / "in.yuv", _pictures(8))
    base = ["encode"] + _models(tmp_path, True) + ["-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H), "--qp-i", "30"]
    _run(base + ["-o", str(tmp_path / "plain.bin")])
    _run(base + ["--scale", "%dx%d" % (W, H), "-o", str(tmp_path / "same.bin")])
    assert (tmp_path / "same.bin").read_bytes() == (tmp_path / "plain.bin").read_bytes()


def _psnr(src, rec, peak):
    """metrics.py calc_psnr of integer samples: the sum of squares is an exact integer, so only log10 can differ"""
    se = int(((src.astype(np.int64) - rec.astype(np.int64)) ** 2).sum())
    mse = se / src.size
    p = 10 * np.log10(peak * peak / mse) if mse > 1e-10 else 999.9
    return float(min(p, 99.9))


@pytest.mark.parametrize("bits", [8, 10])
def test_out_size_writes_and_measures_the_resampled_reconstruction(tmp_path, bits):
    pics = _pictures(bits)
    peak = float((1 << bits) - 1)
    _write(tmp_path / "in.yuv", pics)
    args = _models(tmp_path, True) + _depth(bits)
    _run(["encode"] + args + ["-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H), "--scale", "%dx%d" % (w, h), "--qp-i", "30",
                              "--qp-p", "36", "-o", str(tmp_path / "out.bin")])
    dec = ["decode"] + args + ["-i", str(tmp_path / "out.bin")]
    _run(dec + ["-o", str(tmp_path / "small.yuv")])
    r = _run(dec + ["--out-size", "%dx%d" % (W, H), "-o", str(tmp_path / "big.yuv"), "--ref", str(tmp_path / "in.yuv"),
                    "--json", str(tmp_path / "log.json"), "--calc-ssim", "1", "--verbose-json", "1"])
    assert "output at %dx%d" % (W, H) in r.stdout
    small = _read(tmp_path / "small.yuv", h, w, bits)
    assert len(small) == N
    want = _scaled(small, H, W, bits)
    want_bytes = b"".join(p.astype("<u2" if bits > 8 else np.uint8).tobytes() for y, uv in want for p in (y, uv))
    assert (tmp_path / "big.yuv").read_bytes() == want_bytes, "--out-size does not write the resampled samples of plain decode"

    log = json.loads((tmp_path / "log.json").read_text())
    keys = ({"arith_policy", "frame_pixel_num", "i_frame_num", "p_frame_num", "test_time", "coded_width", "coded_height",
             "frame_bpp", "frame_type", "ave_i_frame_bpp", "ave_p_frame_bpp", "ave_all_frame_bpp"}
            | {"ave_%s_frame_%s%s" % (c, m, s) for c in ("i", "p", "all") for m in ("psnr", "msssim") for s in SFX}
            | {"frame_%s%s" % (m, s) for m in ("psnr", "msssim") for s in SFX})
    assert set(log) == keys, set(log) ^ keys
    assert (log["coded_width"], log["coded_height"], log["frame_pixel_num"]) == (w, h, W * H)
    assert log["frame_type"] == [0, 1, 1]
    size = os.path.getsize(tmp_path / "out.bin")
    assert sum(log["frame_bpp"]) == pytest.approx(8.0 * size / (W * H), rel=1e-12)
    assert log["ave_all_frame_bpp"] == pytest.approx(8.0 * size / (N * W * H), rel=1e-8)      # 9 digits in the log
    for i, ((y, uv), (ry, ruv)) in enumerate(zip(pics, want)):
        p = [_psnr(y, ry, peak), _psnr(uv[0], ruv[0], peak), _psnr(uv[1], ruv[1], peak)]
        p = [(6 * p[0] + p[1] + p[2]) / 8] + p
        if bits > 8:
            s = [msssim_range_np.msssim(y, ry, peak)] + [msssim_range_np.msssim(uv[c], ruv[c], peak) for c in range(2)]
        else:
            s = [msssim_np.msssim(y, ry)] + [msssim_np.msssim(uv[c], ruv[c]) for c in range(2)]
        s = [(6 * s[0] + s[1] + s[2]) / 8] + s
        for k, sfx in enumerate(SFX):
            print(i, sfx, log["frame_psnr" + sfx][i], p[k], log["frame_msssim" + sfx][i], s[k])
            assert log["frame_psnr" + sfx][i] == pytest.approx(p[k], rel=1e-12, abs=0), (i, sfx)
            assert abs(log["frame_msssim" + sfx][i] - s[k]) <= 1e-10, (i, sfx, log["frame_msssim" + sfx][i], s[k])
    for k, sfx in enumerate(SFX):
        assert log["ave_all_frame_psnr" + sfx] == pytest.approx(np.mean(log["frame_psnr" + sfx]), rel=1e-8)


def test_out_size_without_a_reference_only_writes(tmp_path):
    _write(tmp_path / "in.yuv", _pictures(8))
    args = _models(tmp_path, False)
    _run(["encode"] + args + ["-i", str(tmp_path / "in.yuv"), "-W", str(W), "-H", str(H), "-n", "1", "--scale", "%dx%d" % (w, h),
                              "--qp-i", "30", "-o", str(tmp_path / "out.bin")])
    dec = ["decode"] + args + ["-i", str(tmp_path / "out.bin")]
    _run(dec + ["-o", str(tmp_path / "small.yuv")])
    _run(dec + ["--out-size", "200x360", "-o", str(tmp_path / "odd.yuv")])          # another ratio per side, both upwards
    (y, uv), = _read(tmp_path / "small.yuv", h, w, 8)
    (gy, guv), = _read(tmp_path / "odd.yuv", 360, 200, 8)
    (wy, wuv), = _scaled([(y, uv)], 360, 200, 8)
    assert np.array_equal(gy, wy) and np.array_equal(guv, wuv)
    # a ratio outside [1/8, 8] is known only once the stream's size is: refused then, nothing written past the header
    r = _run(dec + ["--out-size", "1600x144", "-o", str(tmp_path / "far.yuv")], check=False)
    assert r.returncode == 2 and "ratio must lie in [1/8, 8]" in r.stderr, r.stderr
