"""dcvc encode | decode --batch N on a real MI355X: N intra pictures per codec call give the file, the reconstructions and the
log of --batch 1 (test_time aside), a short last batch included, for 8-bit and 10-bit YUV420 and PNG sources. (The log is
compared without --calc-ssim: the tool's per-picture MS-SSIM varies from run to run at --batch 1 as well.)
(--batch 1 itself is held to the plugin path by test_cli_gpu.py, test_cli_yuv16_gpu.py and test_cli_rgb_gpu.py.)"""
import json
import os
import subprocess

import numpy as np
import pytest

from codec_util import dmc_ld_model, dmci_model
from dcvc_amd import export_weights, rgb, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 240, 416, 7          # 7 = 4 + a short batch of 3


def _run(args, check=True):
    return subprocess.run([TOOL] + args, check=check, capture_output=True, text=True, timeout=600)


def _sources(tmp_path, kind):
    pics = [synthetic.synthetic_frame_yuv420(H, W, index=i, seed=9) for i in range(N)]
    if kind == "png":
        d = tmp_path / "src"
        d.mkdir()
        for i, (y, uv) in enumerate(pics):
            up = np.repeat(np.repeat(uv, 2, axis=1), 2, axis=2)
            rgb.write_png(str(d / ("im%05d.png" % (i + 1))), np.stack([y, up[0], up[1]], axis=-1).astype(np.uint8))
        return str(d), ["--src-type", "png"]
    path = tmp_path / "in.yuv"
    with open(path, "wb") as f:
        for y, uv in pics:
            if kind == "yuv10":
                rng = np.random.default_rng(3)
                for p in (y, uv):
                    f.write((p.astype(np.uint16) * 4 + rng.integers(0, 4, p.shape)).astype("<u2").tobytes())
            else:
                f.write(y.astype(np.uint8).tobytes())
                f.write(uv.astype(np.uint8).tobytes())
    return str(path), (["--bit-depth", "10"] if kind == "yuv10" else []) + ["-W", str(W), "-H", str(H)]


def _rec_bytes(path):
    if os.path.isdir(path):
        return [open(os.path.join(path, n), "rb").read() for n in sorted(os.listdir(path))]
    return open(path, "rb").read()


@pytest.mark.parametrize("kind", ["yuv8", "yuv10", "png"])
def test_batch_4_equals_batch_1(tmp_path, kind):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    src, fmt = _sources(tmp_path, kind)
    model = ["--intra", str(tmp_path / "i.dcvw")]
    dec_fmt = [a for a in fmt if a not in ("-W", "-H", str(W), str(H))]
    out = {}
    for batch in (1, 4):
        b = str(batch)
        binf, rec, log = (str(tmp_path / ("%s.%s" % (name, b))) for name in ("out_bin", "rec", "log"))
        _run(["encode"] + model + fmt + ["-i", src, "-n", str(N), "--qp-i", "37", "-o", binf, "--batch", b])
        _run(["decode"] + model + dec_fmt + ["-i", binf, "-o", rec, "--ref", src, "--json", log, "--verbose-json", "1",
                                             "--batch", b])
        out[batch] = (open(binf, "rb").read(), _rec_bytes(rec), json.loads(open(log).read()))
    assert out[4][0] == out[1][0], "--batch 4 wrote another file than --batch 1"
    assert out[4][1] == out[1][1], "--batch 4 decoded other pictures than --batch 1"
    l1, l4 = out[1][2], out[4][2]
    assert l1["i_frame_num"] == N and len(l1["frame_psnr"]) == N
    assert {k: v for k, v in l4.items() if k != "test_time"} == {k: v for k, v in l1.items() if k != "test_time"}
    # a decoder limit inside a batch: the first 5 pictures, as --batch 1 gives them
    _run(["decode"] + model + dec_fmt + ["-i", str(tmp_path / "out_bin.1"), "-o", str(tmp_path / "rec5"), "-n", "5",
                                         "--batch", "4"])
    want = out[1][1]
    got = _rec_bytes(str(tmp_path / "rec5"))
    assert got == (want[:5] if isinstance(want, list) else want[:len(want) // N * 5])


def test_refusals(tmp_path):
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(tmp_path / "p.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    src, fmt = _sources(tmp_path, "yuv8")
    base = ["encode", "--intra", str(tmp_path / "i.dcvw"), "-i", src, "-o", str(tmp_path / "o.bin")] + fmt
    r = _run(base + ["--inter", str(tmp_path / "p.dcvw"), "--batch", "2"], check=False)
    assert r.returncode == 2 and "all-intra runs" in r.stderr
    for v in ("0", "17"):
        r = _run(base + ["--batch", v], check=False)
        assert r.returncode == 2 and "--batch must be in 1..16" in r.stderr
    # an inter model with --intra-period 1 is an all-intra run: accepted, and the file is --batch 1's
    ok = base + ["--inter", str(tmp_path / "p.dcvw"), "--intra-period", "1", "-n", "3"]
    _run(ok + ["--batch", "2"])
    a = open(tmp_path / "o.bin", "rb").read()
    _run(ok + ["--batch", "1"])
    assert open(tmp_path / "o.bin", "rb").read() == a
