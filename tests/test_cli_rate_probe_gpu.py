"""dcvc encode --target-bpp --rc-mode probe on a real MI355X (-m gpu), DESIGN.md 15: with an inter model every P unit's
q_index is the one rate_control.code_sequence_probed picks when it is driven with the plug-in's estimate_bits / compress
on the same pictures - the same q_index, probe count, predicted bytes and bytes, unit for unit; the budget is kept (the
prediction fits) and used (the probe one q_index up does not), the unchanged decoder reads the file, and --rc-mode
feedback is the run without the flag, byte for byte."""
import json
import os
import subprocess

import pytest
import torch

from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, rate_control as rc
from oracle import frame_io
from test_cli_gpu import _gpu, _write_yuv
from test_code_length_cpu import R_BOUND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W = 144, 176


def _run(args):
    return subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=900)


def _x(frames, ids):
    xs = [torch.from_numpy(frame_io.yuv420_to_x(*frames[i])).permute(2, 0, 1)[None].cuda() for i in ids]
    return torch.cat(xs, dim=1).contiguous(memory_format=torch.channels_last)


# LD: 14 pictures, a reset every 4; HT-S: 1 + 8 + 8 + 7 pictures, a ragged last chunk (coded as 8 pictures on the budget
# of 7). The horizon is longer than the clip, so that the I picture (many times a P picture at this size) is paid back
# over all of it and the P budgets stay above the floor.
@pytest.mark.parametrize("inter,n,reset_interval,horizon,bonus", [("ld", 14, 4, 16, 2), ("hts", 24, 32, 32, 0)])
def test_probe_mode_equals_the_python_loop(tmp_path, inter, n, reset_interval, horizon, bonus):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    mi = dmci_model(skip_thres=0.15)
    mp = dmc_ld_model(skip_thres=0.15) if inter == "ld" else dmc_ht_model(inter, skip_thres=0.15)
    delay = 1 if inter == "ld" else 8
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", mi, 0.15)
    export_weights.write_dcvw(str(tmp_path / "p.dcvw"), inter, mp, 0.15)
    src = str(tmp_path / "in.yuv")
    frames = _write_yuv(src, H, W, n)
    base = ["encode", "--intra", str(tmp_path / "i.dcvw"), "--inter", str(tmp_path / "p.dcvw"), "-i", src, "-W", str(W), "-H", str(H),
            "--reset-interval", str(reset_interval)]
    pixels = H * W
    qp_lists = []
    for qp0 in (20, 46):
        # the target: what the clip takes at the constant q_index the search starts from
        const = str(tmp_path / ("const%d.bin" % qp0))
        _run(base + ["--qp-i", str(qp0), "-o", const])
        target = 8 * os.path.getsize(const) / (n * pixels)
        log, binf, rec = (str(tmp_path / (name + str(qp0))) for name in ("log.json", "out.bin", "rec.yuv"))
        r = _run(base + ["--qp-i", str(qp0), "-o", binf, "--target-bpp", repr(float(target)), "--rc-mode", "probe",
                         "--rc-horizon", str(horizon), "--rc-intra-bonus", str(bonus), "--rc-log", log])
        print(r.stdout)
        got = json.loads(open(log).read())
        assert got["mode"] == "probe"

        # the loop of rate_control.py on the plug-in
        i_enc, p_enc = _gpu(mi), _gpu(mp)
        pr, pb = i_enc.get_padding_size(H, W, 16)
        probed, coded = {}, {}

        def ids_of(idx, count):
            ids = list(range(idx, idx + count))
            return ids + [ids[-1]] * (delay - count)                 # a short chunk repeats its last picture

        def code_intra(idx, qp):
            enc = i_enc.compress(_x(frames, [idx]), qp, pb, pr)
            p_enc.add_ref_feature_from_frame(enc["x_hat"])
            return enc["bit_stream"]

        def probe_inter(idx, count, qp):
            y_units, z_units, symbols = p_enc.estimate_bits(_x(frames, ids_of(idx, count)), qp, pb, pr)
            probed[(idx, qp)] = (y_units, z_units, symbols)
            return 8 * rc.predicted_stream_bytes(y_units, z_units, rc.ec_parallel_for(symbols))

        def code_inter(idx, count, qp, reset):
            enc = p_enc.compress(_x(frames, ids_of(idx, count)), qp, 1 if reset else 0, pb, pr)
            coded[idx] = enc["ec_parallel"]
            return enc["bit_stream"]

        want_log = []
        want = rc.code_sequence_probed(n, delay, code_intra, code_inter, probe_inter, target, pixels, qp_i=qp0, horizon=horizon,
                                       intra_bonus=bonus, intra_period=-1, reset_interval=reset_interval, log=want_log)
        units = got["units"]
        assert [u["type"] for u in units] == ["I" if u[0] else "P" for u in want]
        assert [u["qp"] for u in units] == [u[1] for u in want]
        assert [u["probes"] for u in units] == [e["probes"] for e in want_log]
        assert [u["bytes"] for u in units] == [len(u[3]) for u in want]
        assert [u["predicted_bytes"] for u in units] == [None if e["predicted_bits"] is None else e["predicted_bits"] // 8
                                                         for e in want_log]
        idx, above_floor = 0, 0
        for u, (intra, qp, reset, payload), e in zip(units, want, want_log):
            if intra:
                assert u["probes"] == 0 and u["predicted_bytes"] is None
                idx += 1
                continue
            assert 1 <= u["probes"] <= 12
            budget, fits = e["budget_bits"], dict(e["trace"])
            print("%s unit at %2d: q %2d, %2d probes, budget %d bits, predicted %d bytes, coded %d bytes"
                  % (inter, idx, qp, u["probes"], budget, u["predicted_bytes"], u["bytes"]))
            # ... never at qp_min with a stream that does not fit (the clips and targets are chosen so: the search then ends
            # with "qp_min was probed and does not fit", which test_rate_probe_search_cpu.py covers)
            assert 8 * u["predicted_bytes"] <= budget, "unit at %d: nothing fits the budget" % idx
            if qp != 0:                                             # kept: the prediction fits
                above_floor += 1
            if qp != 63:                                            # used: one q_index up was probed and does not fit
                assert qp + 1 in fits and fits[qp + 1] > budget
            y_units, z_units, symbols = probed[(idx, qp)]
            ideal = (y_units + z_units) / rc.CODE_LENGTH_UNIT
            ec = coded[idx]
            assert ec == rc.ec_parallel_for(symbols)
            assert 8 * len(payload) >= ideal
            assert 8 * len(payload) <= ideal + rc.stream_fixed_bits(ec) + R_BOUND * ideal
            idx += delay
        assert above_floor > 0, "every P unit sat at qp_min: the run shows nothing"
        qp_lists.append([u["qp"] for u in units])
        # an unchanged decoder: every unit's q_index comes from the container
        d = _run(["decode", "--intra", str(tmp_path / "i.dcvw"), "--inter", str(tmp_path / "p.dcvw"), "-i", binf, "-o", rec,
                  "-n", str(n)])
        assert "decoded %d pictures" % n in d.stdout
        assert os.path.getsize(rec) == n * H * W * 3 // 2
    assert qp_lists[0] != qp_lists[1]


def test_feedback_mode_is_the_run_without_the_flag(tmp_path):
    n = 6
    mi, mp = dmci_model(skip_thres=0.15), dmc_ld_model(skip_thres=0.15)
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", mi, 0.15)
    export_weights.write_dcvw(str(tmp_path / "p.dcvw"), "ld", mp, 0.15)
    src = str(tmp_path / "in.yuv")
    _write_yuv(src, H, W, n)
    base = ["encode", "--intra", str(tmp_path / "i.dcvw"), "--inter", str(tmp_path / "p.dcvw"), "-i", src, "-W", str(W), "-H", str(H),
            "--qp-i", "36", "--target-bpp", "0.3", "--rc-horizon", "4"]
    _run(base + ["-o", str(tmp_path / "a.bin"), "--rc-log", str(tmp_path / "a.json")])
    _run(base + ["-o", str(tmp_path / "b.bin"), "--rc-log", str(tmp_path / "b.json"), "--rc-mode", "feedback"])
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes()
    assert (tmp_path / "a.json").read_text() == (tmp_path / "b.json").read_text()
    assert json.loads((tmp_path / "a.json").read_text())["mode"] == "feedback"
    # an all-intra run probes already and ignores the flag
    intra = ["encode", "--intra", str(tmp_path / "i.dcvw"), "-i", src, "-W", str(W), "-H", str(H), "--target-bpp", "1.5"]
    _run(intra + ["-o", str(tmp_path / "c.bin")])
    _run(intra + ["-o", str(tmp_path / "d.bin"), "--rc-mode", "feedback"])
    assert (tmp_path / "c.bin").read_bytes() == (tmp_path / "d.bin").read_bytes()
