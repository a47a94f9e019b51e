"""dcvc encode --scene-cut on a real MI355X (-m gpu), DESIGN.md 16: on a clip with two cuts the tool's log carries the SADs
of tests/scene_np.py and the scores of scene.SceneCut bit for bit, the I pictures sit where the detector puts them, the
file is the one rate_control.code_sequence(..., intra_at=...) writes through the plug-in with the same decisions, the
unchanged decoder reads it, and without a cut to find nothing changes."""
import io
import json
import os
import subprocess

import pytest
import torch

import scene_np
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, rate_control as rc, scene, stream_helper as sh
from oracle import frame_io
from test_cli_gpu import _gpu, _planes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 144, 176, 20
QP_I, QP_P, RESET = 30, 36, 8        # resets at pictures 8 and 16 by the index, wherever the I pictures fall


def _run(args, check=True):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, check=check, capture_output=True, text=True, timeout=600)


class Clip:
    """the worked clip on disk, its exported models, the plug-in codecs and the numpy SADs, made once for the module"""

    def __init__(self, d):
        self.dir = d
        self.frames = scene_np.clip(H, W)
        self.sads = scene_np.clip_sads(self.frames)
        self.src = str(d / "in.yuv")
        with open(self.src, "wb") as f:
            for y, uv in self.frames:
                f.write(y.tobytes())
                f.write(uv.tobytes())
        self.mi, self.mp = dmci_model(skip_thres=0.15), dmc_ld_model(skip_thres=0.15)
        export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", self.mi, 0.15)
        export_weights.write_dcvw(str(d / "p.dcvw"), "ld", self.mp, 0.15)
        self.models = ["--intra", str(d / "i.dcvw"), "--inter", str(d / "p.dcvw")]
        self.base = ["encode"] + self.models + ["-i", self.src, "-W", str(W), "-H", str(H), "--qp-i", str(QP_I),
                                                "--reset-interval", str(RESET)]
        self.i_enc, self.p_enc = _gpu(self.mi), _gpu(self.mp)
        self.pr, self.pb = self.i_enc.get_padding_size(H, W, 16)

    def x(self, idx):
        t = torch.from_numpy(frame_io.yuv420_to_x(*self.frames[idx])).permute(2, 0, 1)[None].cuda()
        return t.contiguous(memory_format=torch.channels_last)

    def python_stream(self, threshold, min_gap, intra_period):
        """(file bytes, I picture indexes) of the loop of rate_control.py on the plug-in, the detector fed with numpy's SADs"""
        sc = scene.SceneCut(threshold, min_gap, H * W)
        ecs = []

        def code_intra(idx, qp):
            enc = self.i_enc.compress(self.x(idx), qp, self.pb, self.pr)
            self.p_enc.add_ref_feature_from_frame(enc["x_hat"])
            ecs.append(enc["ec_parallel"])
            return enc["bit_stream"]

        def code_inter(idx, count, qp, reset):
            enc = self.p_enc.compress(self.x(idx), qp, 1 if reset else 0, self.pb, self.pr)
            ecs.append(enc["ec_parallel"])
            return enc["bit_stream"]

        units = rc.code_sequence(N, 1, code_intra, code_inter, rc.ConstantQP(QP_I, QP_P), intra_period=intra_period,
                                 reset_interval=RESET, intra_at=lambda idx, scheduled: sc.push(idx, self.sads[idx], scheduled))
        out = io.BytesIO()
        helper = sh.SPSHelper()
        for (intra, qp, reset, payload), ec in zip(units, ecs):
            sps_id, new = helper.get_sps_id({"sps_id": -1, "height": H, "width": W})
            if new:
                sh.write_sps(out, {"sps_id": sps_id, "height": H, "width": W})
            sh.write_ip(out, intra, sps_id, qp, ec, 1 if reset else 0, payload)
        return out.getvalue(), [i for i, u in enumerate(units) if u[0]]

    def python_decode(self, data):
        """the reconstruction file of the plug-in's decoders, following the NAL type of every unit (test_video.py:300-399)"""
        i_dec, p_dec = _gpu(self.mi), _gpu(self.mp)
        f, helper, rec = io.BytesIO(data), sh.SPSHelper(), b""
        for _ in range(N):
            h = sh.read_header(f)
            while h["nal_type"] == sh.NalType.NAL_SPS:
                helper.add_sps_by_id(sh.read_sps_remaining(f, h["sps_id"]))
                h = sh.read_header(f)
            sps = helper.get_sps_by_id(h["sps_id"])
            qp, ec, reset, payload = sh.read_ip_remaining(f)
            if h["nal_type"] == sh.NalType.NAL_I:
                x_hat = i_dec.decompress(payload, sps, qp, ec)["x_hat"]
                p_dec.add_ref_feature_from_frame(x_hat, apply_feature_adaptor=False)
            else:
                x_hat = p_dec.decompress(payload, sps, qp, ec, reset)["x_hat"]
            _, _, y8, uv8 = _planes(x_hat, H, W)
            rec += y8.tobytes() + uv8.tobytes()
        return rec


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    return Clip(tmp_path_factory.mktemp("scene_clip"))


def _encode_with_log(clip, tmp_path, extra):
    binf, log = str(tmp_path / "out.bin"), str(tmp_path / "scene.json")
    r = _run(clip.base + ["--qp-p", str(QP_P), "-o", binf, "--scene-log", log] + extra)
    print(r.stdout)
    return open(binf, "rb").read(), json.loads(open(log).read())


def _check_log(clip, log, threshold, min_gap, scheduled):
    """the log against numpy's SADs and the Python detector, with =="""
    assert (log["threshold"], log["min_gap"], log["width"], log["height"]) == (threshold, min_gap, W, H)
    pics = log["pictures"]
    assert [p["idx"] for p in pics] == list(range(N))
    assert [p["sad"] for p in pics] == clip.sads
    sc = scene.SceneCut(threshold, min_gap, H * W)
    for p in pics:
        intra = sc.push(p["idx"], clip.sads[p["idx"]], p["idx"] in scheduled)
        assert p["mafd"] == sc.mafd and p["score"] == sc.score and p["detected"] == sc.detected, p
        assert p["type"] == ("I" if intra else "P"), p
    return [p["idx"] for p in pics if p["type"] == "I"], {p["idx"]: p["reason"] for p in pics if p["reason"] is not None}


def test_cut_becomes_an_i_picture_and_the_gap_holds(clip, tmp_path):
    got_bin, log = _encode_with_log(clip, tmp_path, ["--scene-cut", "5", "--scene-min-gap", "8"])
    intra, reasons = _check_log(clip, log, 5, 8, (0,))
    assert intra == [0, 9] and reasons == {0: "first", 9: "cut"}
    assert [p["idx"] for p in log["pictures"] if p["detected"]] == [9, 12]        # 12 is detected but stays a P picture
    want_bin, want_intra = clip.python_stream(5, 8, -1)
    assert want_intra == [0, 9]
    assert got_bin == want_bin, "the tool's stream differs from the plug-in loop's"
    # the unchanged decoder follows the NAL types
    rec, dlog = str(tmp_path / "rec.yuv"), str(tmp_path / "dec.json")
    d = _run(["decode"] + clip.models + ["-i", str(tmp_path / "out.bin"), "-o", rec, "--ref", clip.src, "--json", dlog,
                                         "--verbose-json", "1", "-n", str(N)])
    assert "decoded %d pictures" % N in d.stdout
    assert open(rec, "rb").read() == clip.python_decode(want_bin), "reconstruction file differs"
    dec = json.loads(open(dlog).read())
    assert dec["i_frame_num"] == 2 and dec["p_frame_num"] == N - 2
    assert [i for i, t in enumerate(dec["frame_type"]) if t == 0] == [0, 9]


def test_min_gap_one_codes_both_cuts(clip, tmp_path):
    got_bin, log = _encode_with_log(clip, tmp_path, ["--scene-cut", "5", "--scene-min-gap", "1"])
    intra, reasons = _check_log(clip, log, 5, 1, (0,))
    assert intra == [0, 9, 12] and reasons == {0: "first", 9: "cut", 12: "cut"}
    want_bin, want_intra = clip.python_stream(5, 1, -1)
    assert want_intra == intra
    assert got_bin == want_bin, "the tool's stream differs from the plug-in loop's"


def test_intra_period_stays_index_based(clip, tmp_path):
    got_bin, log = _encode_with_log(clip, tmp_path, ["--scene-cut", "5", "--scene-min-gap", "2", "--intra-period", "8"])
    intra, reasons = _check_log(clip, log, 5, 2, (0, 9, 17))
    assert intra == [0, 9, 12, 17] and reasons == {0: "first", 9: "period", 12: "cut", 17: "period"}
    want_bin, want_intra = clip.python_stream(5, 2, 8)
    assert want_intra == intra
    assert got_bin == want_bin, "the tool's stream differs from the plug-in loop's"


def test_a_threshold_never_reached_changes_nothing(clip, tmp_path):
    got_bin, log = _encode_with_log(clip, tmp_path, ["--scene-cut", "100"])
    intra, reasons = _check_log(clip, log, 100, 8, (0,))
    assert intra == [0] and reasons == {0: "first"} and not any(p["detected"] for p in log["pictures"])
    plain = str(tmp_path / "plain.bin")
    _run(clip.base + ["--qp-p", str(QP_P), "-o", plain])
    assert got_bin == open(plain, "rb").read()


def test_composes_with_target_bpp(clip, tmp_path):
    binf, rlog, slog = (str(tmp_path / n) for n in ("out.bin", "rc.json", "scene.json"))
    _run(clip.base + ["-o", binf, "--target-bpp", "0.4", "--rc-horizon", "8", "--rc-log", rlog, "--scene-cut", "5", "--scene-log", slog])
    units = json.loads(open(rlog).read())["units"]
    assert len(units) == N and [i for i, u in enumerate(units) if u["type"] == "I"] == [0, 9]
    assert [p["idx"] for p in json.loads(open(slog).read())["pictures"] if p["type"] == "I"] == [0, 9]
    rec = str(tmp_path / "rec.yuv")
    d = _run(["decode"] + clip.models + ["-i", binf, "-o", rec, "-n", str(N)])
    assert "decoded %d pictures" % N in d.stdout and os.path.getsize(rec) == N * H * W * 3 // 2


def test_eight_picture_models_are_refused(clip, tmp_path):
    export_weights.write_dcvw(str(tmp_path / "hts.dcvw"), "hts", dmc_ht_model("hts", skip_thres=0.15), 0.15)
    r = _run(["encode", "--intra", str(clip.dir / "i.dcvw"), "--inter", str(tmp_path / "hts.dcvw"), "-i", clip.src, "-W", str(W),
              "-H", str(H), "-o", str(tmp_path / "o.bin"), "--scene-cut", "5"], check=False)
    assert r.returncode == 2, r.stderr
    assert "chunks of 8 pictures" in r.stderr and "cannot be cut short" in r.stderr
    assert not os.path.exists(str(tmp_path / "o.bin"))
