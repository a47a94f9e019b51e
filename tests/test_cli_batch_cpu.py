"""dcvc encode | decode --batch: the refusals run before the tool loads a model or touches the device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("mode", ["encode", "decode"])
@pytest.mark.parametrize("value", ["0", "17", "-1", "4x", ""])
def test_batch_out_of_range_is_refused(tmp_path, mode, value):
    r = _run([mode, "--intra", str(tmp_path / "missing.dcvw"), "-i", str(tmp_path / "missing"), "-o", str(tmp_path / "o"),
              "--batch", value])
    assert r.returncode == 2 and "--batch must be in 1..16" in r.stderr, r.stderr


@pytest.mark.parametrize("period", [None, "-1", "32"])
def test_batch_with_an_inter_model_is_refused(tmp_path, period):
    args = ["encode", "--intra", str(tmp_path / "i.dcvw"), "--inter", str(tmp_path / "p.dcvw"), "-i", str(tmp_path / "in.yuv"),
            "-W", "64", "-H", "64", "-o", str(tmp_path / "o.bin"), "--batch", "2"]
    if period is not None:
        args += ["--intra-period", period]
    r = _run(args)
    assert r.returncode == 2 and "all-intra runs" in r.stderr, r.stderr
