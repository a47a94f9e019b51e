"""dcvc encode --target-bpp on a real MI355X (-m gpu), DESIGN.md 15.

All-intra: every picture's q_index is the one rate_control.pick_qp_for_budget picks when driven with
DMCIProxy.estimate_bits on the same pictures, the log's predictions are the plug-in's, the budget is used (the probe one
q_index up does not fit) and kept (within the prediction bound), and an unchanged dcvc decode reads every unit's q_index
from the container. With the LD model: the q_index list of rate_control.code_sequence with TargetBpp on the plug-in."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from codec_util import dmc_ld_model, dmci_model
from dcvc_amd import export_weights, rate_control as rc
from oracle import frame_io
from test_cli_gpu import _gpu, _planes, _write_yuv
from test_code_length_cpu import R_BOUND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 144, 176, 16
PROBE_CAP = 7                     # ceil(log2(63 - 0 + 2)), the bisection of rate_control.pick_qp_for_budget over 0 .. 63


def _run(args):
    return subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=900)


def _x(frames, i):
    return torch.from_numpy(frame_io.yuv420_to_x(*frames[i])).permute(2, 0, 1)[None].cuda().contiguous(
        memory_format=torch.channels_last)


def _predict(proxy, x, qp, pb, pr):
    """(predicted stream bytes, ideal bits) of the plug-in's probe"""
    y_units, z_units, symbols = proxy.estimate_bits(x, qp, pb, pr)
    return rc.predicted_stream_bytes(y_units, z_units, rc.ec_parallel_for(symbols)), (y_units + z_units) / rc.CODE_LENGTH_UNIT


def test_all_intra_run_codes_to_the_target(tmp_path):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    mi = dmci_model(skip_thres=0.15)
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", mi, 0.15)
    src = str(tmp_path / "in.yuv")
    frames = _write_yuv(src, H, W, N)
    model = _gpu(mi)
    pr, pb = model.get_padding_size(H, W, 16)
    proxy = model._ensure_proxy()
    xs = [_x(frames, i) for i in range(N)]
    pixels = H * W
    # the range the clip can reach: its rate at q 8, 32 and 56
    targets = []
    for qp in (8, 32, 56):
        bits = sum(8 * len(proxy.compress(x, qp, pb, pr)[0]) for x in xs)
        targets.append(bits / (N * pixels))
    print("targets (bpp at q 8, 32, 56):", targets)
    assert targets[0] < targets[1] < targets[2]

    for target in targets:
        tag = "%.6f" % target
        binf, log, rec = (str(tmp_path / (name + tag)) for name in ("out.bin", "log.json", "rec.yuv"))
        r = _run(["encode", "--intra", str(tmp_path / "i.dcvw"), "-i", src, "-W", str(W), "-H", str(H), "-o", binf,
                  "--target-bpp", repr(float(target)), "--rc-log", log])
        print(r.stdout)
        got = json.loads(open(log).read())
        units = got["units"]
        assert got["mode"] == "probe" and len(units) == N and all(u["type"] == "I" for u in units)

        # the reference loop in Python on the plug-in's probe
        spent, want_qp, want_rec, bound_bits = 0, [], b"", 0.0
        for k, x in enumerate(xs):
            budget = rc.intra_budget_bits(target, pixels, k, spent)
            assert budget == int(np.floor(target * pixels * (k + 1) - spent)), "picture %d: the budget floor was reached" % k
            trace = []
            qp = rc.pick_qp_for_budget(lambda q: 8 * _predict(proxy, x, q, pb, pr)[0], budget, 0, 63, trace=trace)
            want_qp.append(qp)
            predicted, ideal = _predict(proxy, x, qp, pb, pr)
            u = units[k]
            # ... never at qp_min with a stream that does not fit (the targets are chosen so)
            assert 8 * predicted <= budget, "picture %d: nothing fits the budget" % k
            assert u["probes"] == len(trace) and 1 <= u["probes"] <= PROBE_CAP
            assert u["qp"] == qp, (k, [v["qp"] for v in units], want_qp)
            assert u["predicted_bytes"] == predicted
            if qp < 63:                                   # the budget is used: one q_index up does not fit
                assert 8 * _predict(proxy, x, qp + 1, pb, pr)[0] > budget, k
            bs, x_hat, ec = proxy.compress(x, qp, pb, pr)
            torch.cuda.synchronize()
            assert u["bytes"] == len(bs)
            coded, fixed = 8 * len(bs), rc.stream_fixed_bits(ec)
            print("picture %2d: q %2d, %d probes, budget %d bits, predicted %d bytes, coded %d bytes, ideal %.1f bits"
                  % (k, qp, len(trace), budget, predicted, len(bs), ideal))
            assert coded >= ideal
            assert coded <= ideal + fixed + R_BOUND * ideal
            bound_bits += R_BOUND * ideal
            spent += coded
            _, _, y8, uv8 = _planes(x_hat, H, W)
            want_rec += y8.tobytes() + uv8.tobytes()
        assert [u["qp"] for u in units] == want_qp
        assert len(set(want_qp)) >= 1
        # the budget is kept: the clip's bits against target * pictures, within the prediction bound
        assert spent <= target * pixels * N + bound_bits, (spent, target * pixels * N, bound_bits)
        assert got["achieved_bpp"] == pytest.approx(spent / (N * pixels), rel=1e-12)
        assert got["target_bpp"] == target
        # an unchanged decoder: every unit's q_index comes from the container
        d = _run(["decode", "--intra", str(tmp_path / "i.dcvw"), "-i", binf, "-o", rec, "-n", str(N)])
        print(d.stdout)
        assert open(rec, "rb").read() == want_rec, "the decoded pictures are not the encoder's reconstructions"
    # the three targets ask for three different codings
    assert len({tuple(json.loads(open(str(tmp_path / ("log.json%.6f" % t))).read())["units"][0].items()) for t in targets}) == 3


def test_qp_range_is_respected(tmp_path):
    mi = dmci_model(skip_thres=0.15)
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", mi, 0.15)
    src = str(tmp_path / "in.yuv")
    _write_yuv(src, H, W, 4)
    log = str(tmp_path / "log.json")
    _run(["encode", "--intra", str(tmp_path / "i.dcvw"), "-i", src, "-W", str(W), "-H", str(H), "-o", str(tmp_path / "o.bin"),
          "--target-bpp", "100", "--qp-min", "20", "--qp-max", "29", "--rc-log", log])
    units = json.loads(open(log).read())["units"]
    assert [u["qp"] for u in units] == [29] * 4                         # everything fits: the top of the range
    assert all(u["probes"] <= 4 for u in units)                         # ceil(log2(29 - 20 + 2))
    _run(["encode", "--intra", str(tmp_path / "i.dcvw"), "-i", src, "-W", str(W), "-H", str(H), "-o", str(tmp_path / "o.bin"),
          "--target-bpp", "0.000001", "--qp-min", "20", "--qp-max", "29", "--rc-log", log])
    units = json.loads(open(log).read())["units"]
    assert [u["qp"] for u in units] == [20] * 4                         # nothing fits: qp_min
    assert all(u["predicted_bytes"] > 0 and 8 * u["bytes"] > 0.000001 * H * W for u in units)


def test_ld_run_follows_the_feedback_controller(tmp_path):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    n, reset_interval, qp0 = 14, 4, 36
    mi, mp = dmci_model(skip_thres=0.15), dmc_ld_model(skip_thres=0.15)
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", mi, 0.15)
    export_weights.write_dcvw(str(tmp_path / "p.dcvw"), "ld", mp, 0.15)
    src = str(tmp_path / "in.yuv")
    frames = _write_yuv(src, H, W, n)
    base = ["encode", "--intra", str(tmp_path / "i.dcvw"), "--inter", str(tmp_path / "p.dcvw"), "-i", src, "-W", str(W), "-H", str(H),
            "--reset-interval", str(reset_interval)]
    # a target below what the constant q_index gives, so that the controller has to move
    _run(base + ["--qp-i", str(qp0), "-o", str(tmp_path / "const.bin")])
    target = 0.6 * 8 * os.path.getsize(str(tmp_path / "const.bin")) / (n * H * W)
    for bonus in (0, 3):
        log, binf = str(tmp_path / ("log%d.json" % bonus)), str(tmp_path / ("out%d.bin" % bonus))
        _run(base + ["--qp-i", str(qp0), "-o", binf, "--target-bpp", repr(float(target)), "--rc-horizon", "4",
                     "--rc-intra-bonus", str(bonus), "--rc-log", log])
        got = json.loads(open(log).read())
        assert got["mode"] == "feedback"

        i_enc, p_enc = _gpu(mi), _gpu(mp)
        pr, pb = i_enc.get_padding_size(H, W, 16)

        def code_intra(idx, qp):
            enc = i_enc.compress(_x(frames, idx), qp, pb, pr)
            p_enc.add_ref_feature_from_frame(enc["x_hat"])
            return enc["bit_stream"]

        def code_inter(idx, count, qp, reset):
            return p_enc.compress(_x(frames, idx), qp, 1 if reset else 0, pb, pr)["bit_stream"]

        ctl = rc.TargetBpp(target, H * W, qp0=qp0, horizon=4, intra_bonus=bonus)
        want = rc.code_sequence(n, 1, code_intra, code_inter, ctl, intra_period=-1, reset_interval=reset_interval)
        assert [u["qp"] for u in got["units"]] == [u[1] for u in want]
        assert [u["type"] for u in got["units"]] == ["I" if u[0] else "P" for u in want]
        assert [u["bytes"] for u in got["units"]] == [len(u[3]) for u in want]
        assert all(u["probes"] == 0 and u["predicted_bytes"] is None for u in got["units"])
        assert len({u[1] for u in want}) > 1, "the controller never moved"
        d = _run(["decode", "--intra", str(tmp_path / "i.dcvw"), "--inter", str(tmp_path / "p.dcvw"), "-i", binf,
                  "-o", str(tmp_path / "rec.yuv"), "-n", str(n)])
        assert "decoded %d pictures" % n in d.stdout
        assert os.path.getsize(str(tmp_path / "rec.yuv")) == n * H * W * 3 // 2
