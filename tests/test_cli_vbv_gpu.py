"""dcvc encode --vbv-maxrate / --vbv-bufsize on a real MI355X (-m gpu), DESIGN.md 25.

Seeded synthetic weights, 176x144 pictures; three runs - LD at a constant q_index, all-intra --target-bpp, HT-S --target-bpp
--rc-mode probe with a ragged last chunk. The bucket comes from plain runs by rule: maxrate = 0.7 of the plain run's mean
P-unit (all-intra: picture) bits per picture and pixel; bufsize = the smallest whole number of picture periods at which the
plain run at the floor q_index conforms under rate_control.vbv_replay - the precondition that makes "no violation" reachable,
asserted with its own message. Then:

  1. the tool's --vbv-log equals rate_control's loop with vbv= on the plug-in (compress, estimate_bits, export_state,
     import_state) on the same pictures, unit for unit: qp_mode, qp, probes, recodes, bytes, and the fullness as == on doubles;
  2. vbv_replay on the unit sizes parsed from the output file: no unit above avail, no violation;
  3. the bound was used: a unit with qp < qp_mode and a unit with qp == qp_mode;
  4. the unchanged decoder reads the file and writes n pictures;
  5. with a bucket ten times larger the file is the plain run's, byte for byte, and no unit is coded twice.

Measured on an MI355X, with the bucket the rule gives:

  ld-constant   maxrate 0.7077 bpp = 17937 bits per period, bufsize 2: the I picture (30056 bits at q 40) is left alone, the 9 P
                units are lowered from q 40 to q 5 .. 20 with one recode each (10 probes), the coded unit 3 or 4 bytes above its
                prediction, minimum fullness 18002 bits.
  intra-target  maxrate 0.7040 bpp = 17842 bits per period; the floor's pictures (q 20) take 16840 .. 17368 bits, bufsize 2. The
                first picture is left alone (q 35, 24896 bits of 32114), the other three are held under the bucket by their own
                search (q 36 -> 35, 30 -> 23, 41 -> 24; no recode), minimum fullness 17953 bits.
  hts-probe     maxrate 0.2236 bpp = 5667 bits per period, bufsize 9. The I picture sits at the floor (q 2, 13000 bits), the chunk
                of 8 is held from q 36 to q 9 (38456 bits of 38564), the ragged chunk of 7 from q 16 to q 14. With the I picture at
                the P units' start value (q 36, 25960 bits; no --rc-intra-bonus) the first chunk finds 23624 bits, takes 31920 at
                the floor, and is a violation of 8296 bits although the floor run conforms."""
import json
import os
import subprocess

import pytest
import torch

from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, rate_control as rc, stream_helper as sh
from oracle import frame_io
from test_cli_gpu import _gpu, _write_yuv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W = 144, 176
PIXELS = H * W


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=900)


def _x(frames, ids):
    xs = [torch.from_numpy(frame_io.yuv420_to_x(*frames[i])).permute(2, 0, 1)[None].cuda() for i in ids]
    return torch.cat(xs, dim=1).contiguous(memory_format=torch.channels_last)


def _file_units(path, delay, n):
    """[(bits, pictures, is_intra)] of a stream file: a parameter set counts with the unit behind it"""
    units, pending, idx = [], 0, 0
    with open(path, "rb") as f:
        for u in sh.iter_units(f):
            if u["nal_type"] == sh.NalType.NAL_SPS:
                pending += sh.unit_overhead(0, u) - sh.unit_overhead(0)
                continue
            intra = u["nal_type"] == sh.NalType.NAL_I
            count = 1 if intra else min(delay, n - idx)
            units.append((8 * (pending + len(u["payload"]) + sh.unit_overhead(len(u["payload"]))), count, intra))
            pending, idx = 0, idx + (1 if intra else delay)
    assert pending == 0 and 8 * os.path.getsize(path) == sum(u[0] for u in units)
    return units


# (name, inter model, pictures, the rate mode's flags, the flags of the plain run at the floor q_index, floor q_index)
CASES = [
    ("ld-constant", "ld", 10, ["--qp-i", "40", "--qp-p", "40", "--reset-interval", "4"], ["--qp-i", "0", "--qp-p", "0", "--reset-interval", "4"], 0),
    # All-intra --target-bpp gives every picture the q_index that fills its budget, so the plain run's pictures are of one size p
    # and a period brings r = 0.7 p. A unit can be left alone only if the bucket holds more than one period, and the rule gives it
    # two exactly when the floor's pictures take more than 0.9 r (the start fullness of one period is too little for the first);
    # behind a lowered unit the bucket holds at least r, so nothing sticks out as long as they take less than r. The floor q_index
    # 20 puts them there: the plain run codes at q 33 .. 36, a picture's size rises by 2 to 3 % per q_index at this picture size,
    # so about 15 steps down it is near 0.67 p = 0.95 r (measured: 0.94 .. 0.97 r). The test says so if that moves.
    ("intra-target", None, 4, ["--target-bpp", None, "--qp-min", "20"], ["--qp-i", "20"], 20),
    # The procedure fits one unit at a time: an I picture that fits at its mode's q_index is not held back for the chunk of 8
    # behind it, and the smallest bucket in which the floor run conforms has no room for more than the floor run's I picture in
    # front of that chunk. --rc-intra-bonus is the user's handle for it, and the case uses it: the I picture
    # is coded 34 steps under the P units' start value, at the floor.
    ("hts-probe", "hts", 16, ["--qp-i", "36", "--target-bpp", None, "--rc-mode", "probe", "--rc-horizon", "32", "--qp-min", "2",
                              "--rc-intra-bonus", "-34"], ["--qp-i", "2"], 2),
]


@pytest.mark.parametrize("name,inter,n,mode,floor_flags,floor_q", CASES, ids=[c[0] for c in CASES])
def test_capped_run(tmp_path, name, inter, n, mode, floor_flags, floor_q):
    mi = dmci_model(skip_thres=0.15)
    export_weights.write_dcvw(str(tmp_path / "i.dcvw"), "dmci", mi, 0.15)
    models = ["--intra", str(tmp_path / "i.dcvw")]
    mp, delay = None, 1
    if inter:
        mp = dmc_ld_model(skip_thres=0.15) if inter == "ld" else dmc_ht_model(inter, skip_thres=0.15)
        delay = 1 if inter == "ld" else 8
        export_weights.write_dcvw(str(tmp_path / "p.dcvw"), inter, mp, 0.15)
        models += ["--inter", str(tmp_path / "p.dcvw")]
    src = str(tmp_path / "in.yuv")
    frames = _write_yuv(src, H, W, n)
    base = ["encode"] + models + ["-i", src, "-W", str(W), "-H", str(H)]
    target = None
    if "--target-bpp" in mode:
        # the target: what the clip takes at a constant q_index in the middle of the range
        _run(base + ["--qp-i", "36", "-o", str(tmp_path / "const.bin")])
        target = 8 * os.path.getsize(str(tmp_path / "const.bin")) / (n * PIXELS)
        mode = [repr(float(target)) if m is None else m for m in mode]

    # the plain runs, and the bucket by rule
    plain, floor = str(tmp_path / "plain.bin"), str(tmp_path / "floor.bin")
    _run(base + mode + ["-o", plain])
    _run(base + floor_flags + ["-o", floor])
    plain_units = _file_units(plain, delay, n)
    counted = [u for u in plain_units if not u[2]] or plain_units                  # P units; all-intra: the pictures
    maxrate = 0.7 * sum(u[0] for u in counted) / (sum(u[1] for u in counted) * PIXELS)
    floor_units = [u[:2] for u in _file_units(floor, delay, n)]
    bufsize = next((b for b in range(1, 4096) if not rc.vbv_replay(floor_units, maxrate, b, PIXELS)[2]), None)
    assert bufsize is not None and rc.vbv_replay(floor_units, maxrate, bufsize, PIXELS)[1] >= 0, \
        "precondition: the plain run at the floor q_index %d does not conform under any bucket tried" % floor_q
    if name == "intra-target":
        period = maxrate * PIXELS
        assert bufsize == 2 and all(0.9 * period < u[0] < period for u in floor_units[1:]), \
            "the floor's pictures no longer take between 0.9 and 1.0 of a period's bits: choose the floor q_index of this case again"
    print("%s: maxrate %.6f bpp (%.1f bits per picture), bufsize %d pictures, plain units %s, floor units %s"
          % (name, maxrate, maxrate * PIXELS, bufsize, [u[0] for u in plain_units], [u[0] for u in floor_units]))

    capped, vlog, rlog, rec = (str(tmp_path / f) for f in ("capped.bin", "vbv.json", "rc.json", "rec.yuv"))
    vbv_flags = ["--vbv-maxrate", repr(float(maxrate)), "--vbv-bufsize", str(bufsize)]
    r = _run(base + mode + vbv_flags + ["--vbv-log", vlog, "-o", capped] + (["--rc-log", rlog] if target else []))
    print(r.stdout, r.stderr)
    got = json.loads(open(vlog).read())
    vbv = rc.Vbv(maxrate, bufsize, PIXELS)
    assert (got["maxrate_bpp"], got["bufsize_pictures"], got["init"], got["width"], got["height"]) == (maxrate, bufsize, 0.9, W, H)
    assert (got["rate_bits"], got["capacity_bits"]) == (vbv.rate, vbv.capacity)

    # 1. the loop of rate_control.py on the plug-in
    i_enc = _gpu(mi)
    pr, pb = i_enc.get_padding_size(H, W, 16)
    p_enc = _gpu(mp) if mp is not None else None
    proxy = p_enc._ensure_proxy() if p_enc is not None else None
    kept = {}

    def ids_of(idx, count):
        ids = list(range(idx, idx + count))
        return ids + [ids[-1]] * (delay - count)                                   # a short chunk repeats its last picture

    def predicted_bits(estimate):
        y_units, z_units, symbols = estimate
        return 8 * rc.predicted_stream_bytes(y_units, z_units, rc.ec_parallel_for(symbols))

    def code_intra(idx, qp):
        enc = i_enc.compress(_x(frames, [idx]), qp, pb, pr)
        kept["x_hat"] = enc["x_hat"]
        return enc["bit_stream"]

    def code_inter(idx, count, qp, reset):
        return p_enc.compress(_x(frames, ids_of(idx, count)), qp, 1 if reset else 0, pb, pr)["bit_stream"]

    def probe_intra(idx, qp):
        return predicted_bits(i_enc.estimate_bits(_x(frames, [idx]), qp, pb, pr))

    def probe_inter(idx, count, qp):
        return predicted_bits(p_enc.estimate_bits(_x(frames, ids_of(idx, count)), qp, pb, pr))

    def snapshot():
        kept["state"] = proxy.export_state().clone()

    def restore():
        proxy.import_state(kept["state"], H, W)

    def accept(intra, idx, qp):
        if intra and p_enc is not None:
            p_enc.add_ref_feature_from_frame(kept["x_hat"])

    want_log = []
    hooks = dict(snapshot=snapshot, restore=restore, accept=accept, picture_size=(H, W), vbv_log=want_log)
    if name == "ld-constant":
        want = rc.code_sequence(n, 1, code_intra, code_inter, rc.ConstantQP(40, 40), reset_interval=4, vbv=vbv, probe_intra=probe_intra,
                                probe_inter=probe_inter, **hooks)
    elif name == "intra-target":
        want = rc.code_sequence_intra_search(n, code_intra, probe_intra, target, PIXELS, qp_min=floor_q, vbv=vbv, **hooks)
    else:
        want = rc.code_sequence_probed(n, delay, code_intra, code_inter, probe_inter, target, PIXELS, qp_i=36, horizon=32, intra_bonus=-34, qp_min=floor_q,
                                       vbv=vbv, probe_intra=probe_intra, **hooks)
    units = got["units"]
    for u in units:
        print("%s unit at %2d (%d): q %2d -> %2d, %2d probes, %d recodes, predicted %s, %d bytes, fullness %.1f -> %.1f%s"
              % (u["type"], u["first_picture"], u["pictures"], u["qp_mode"], u["qp"], u["probes"], u["recodes"], u["predicted_bytes"],
                 u["bytes"], u["fullness_before"], u["fullness_after"], ", VIOLATED by %d bits" % u["underflow_bits"] if u["violated"] else ""))
    assert len(units) == len(want_log) == len(want)
    for key in ("type", "first_picture", "pictures", "qp_mode", "qp", "probes", "recodes", "predicted_bytes", "bytes", "fullness_before",
                "fullness_after", "violated", "underflow_bits"):
        assert [u[key] for u in units] == [e[key] for e in want_log], key          # the fullness: == on doubles
    assert got["min_fullness"] == min([0.9 * vbv.capacity] + [u["fullness_after"] for u in units])
    assert got["lowered"] == sum(u["qp"] < u["qp_mode"] for u in units) and got["recodes"] == sum(u["recodes"] for u in units)
    assert got["violations"] == sum(u["violated"] for u in units)
    if target:
        rate_units = json.loads(open(rlog).read())["units"]                        # --rc-log keeps its keys and reports the final q_index
        assert [set(u) for u in rate_units] == [{"type", "qp", "probes", "predicted_bytes", "bytes"}] * len(units)
        assert [(u["qp"], u["bytes"]) for u in rate_units] == [(w[1], len(w[3])) for w in want]

    # 2. the file itself under the model
    file_units = _file_units(capped, delay, n)
    assert [u[0] for u in file_units] == [8 * u["bytes"] for u in units] and [u[1] for u in file_units] == [u["pictures"] for u in units]
    fullness, slack, violations = rc.vbv_replay([u[:2] for u in file_units], maxrate, bufsize, PIXELS)
    assert fullness[1:] == [u["fullness_after"] for u in units]
    assert slack >= 0 and violations == [] and got["violations"] == 0, (slack, violations)

    # 3. the bound was used, and not everywhere
    assert any(u["qp"] < u["qp_mode"] for u in units), "no unit was lowered: the run shows nothing"
    assert any(u["qp"] == u["qp_mode"] for u in units), "every unit was lowered: the run does not show a unit that is left alone"
    assert all(floor_q <= u["qp"] for u in units)

    # 4. the unchanged decoder
    d = _run(["decode"] + models + ["-i", capped, "-o", rec, "-n", str(n)])
    assert "decoded %d pictures" % n in d.stdout
    assert os.path.getsize(rec) == n * H * W * 3 // 2

    # 5. a bucket that never binds: the plain run's file, and nothing is coded twice
    loose, llog = str(tmp_path / "loose.bin"), str(tmp_path / "loose.json")
    _run(base + mode + ["--vbv-maxrate", repr(float(maxrate)), "--vbv-bufsize", str(10 * bufsize), "--vbv-log", llog, "-o", loose])
    assert open(loose, "rb").read() == open(plain, "rb").read()
    loose_log = json.loads(open(llog).read())
    assert all(u["recodes"] == 0 and u["qp"] == u["qp_mode"] and not u["violated"] for u in loose_log["units"])
    assert (loose_log["lowered"], loose_log["recodes"], loose_log["violations"]) == (0, 0, 0)
    assert [8 * u["bytes"] for u in loose_log["units"]] == [u[0] for u in plain_units]
