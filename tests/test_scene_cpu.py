"""Scene-cut detection without a GPU: the luma recovery dcvc_luma_sad is defined by, scene.SceneCut against
dcvc_scd_* (include/dcvc_amd_rc.h) with ==, the worked clip with its two cuts, and every refusal of dcvc_scd_*,
dcvc_luma_sad and dcvc encode --scene-cut that is decided before a model is loaded or the device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import scene_np
from dcvc_amd import _lib, scene
from oracle import frame_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W = 144, 176

_vp, _ci, _cd, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong


def _scd():
    return dict(
        create=_lib.fn("dcvc_scd_create", _vp, [_cd, _ci, _ll]),
        push=_lib.fn("dcvc_scd_push", _ci, [_vp, _ci, _ll, _ci]),
        last=_lib.fn("dcvc_scd_last", _ci, [_vp, ctypes.POINTER(_cd), ctypes.POINTER(_cd), ctypes.POINTER(_ci)]),
        destroy=_lib.fn("dcvc_scd_destroy", None, [_vp]),
    )


def _last(f, h):
    mafd, score, detected = _cd(), _cd(), _ci()
    assert f["last"](h, ctypes.byref(mafd), ctypes.byref(score), ctypes.byref(detected)) == 0
    return mafd.value, score.value, bool(detected.value)


# ---------------------------------------------------------------------------------------------------------------- luma8
def test_luma8_recovers_every_8_bit_sample():
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    uv = np.full((2, 8, 8), 128, dtype=np.uint8)
    x = frame_io.yuv420_to_x(y, uv)
    assert x.dtype == np.float16
    assert np.array_equal(scene_np.luma8(x[..., 0]), y)


def test_luma8_clamps_and_rounds_half_to_even():
    f16 = np.float16
    assert scene_np.luma8(f16([-0.75, 0.75, -0.5, 0.5])).tolist() == [0, 255, 0, 255]
    # a product of exactly k + 0.5 needs x0 + 0.5 to be a multiple of 1 / 2: x0 = +-0 -> 127.5 -> 128 inside the range,
    # x0 = 1 -> 382.5 and x0 = -1 -> -127.5 outside it, where the clamp decides ...
    assert scene_np.luma8(f16([0.0, -0.0, 1.0, -1.0])).tolist() == [128, 128, 255, 0]
    # ... and no other fp16 value of the range gets there, through the fp32 rounding of the product either
    every = np.arange(1 << 16, dtype=np.uint16).view(f16)
    every = every[np.abs(every.astype(np.float32)) <= 0.5]
    v = (every.astype(np.float32) + np.float32(0.5)) * np.float32(255.0)
    assert set(every[v - np.floor(v) == 0.5].tolist()) == {0.0}
    # the rounding rule itself, on fp32 values of the form k + 0.5
    halves = np.float32([0.5, 1.5, 2.5, 126.5, 127.5, 253.5, 254.5])
    assert np.rint(halves).tolist() == [0, 2, 2, 126, 128, 254, 254]
    # just beside the half-way point the nearest sample wins: 127.5 -+ 255 ulp(x0)
    below, above = np.nextafter(f16(0), f16(-1)), np.nextafter(f16(0), f16(1))
    assert scene_np.luma8(np.array([below, above])).tolist() == [127, 128]
    assert scene_np.luma8(f16([np.nan])).tolist() == [0]


def test_sad_is_exact():
    a = np.full((300, 300), 255, dtype=np.uint8)
    assert scene_np.sad(a, np.zeros_like(a)) == 255 * 300 * 300
    assert scene_np.sad(a, a) == 0


# ------------------------------------------------------------------------------------------------- SceneCut == dcvc_scd
def test_python_and_native_detectors_agree_bit_for_bit():
    f = _scd()
    rng = np.random.default_rng(20)
    returned_one, detected_some, gap_held = 0, 0, 0
    for case in range(200):
        pixels = int(rng.choice([1, 7, 144 * 176, 1920 * 1080, 16384 * 16384]))
        threshold = float(rng.choice([0.25, 1.0, 5.0, 12.5, 40.0, 100.0]) * rng.uniform(0.5, 1.0))
        min_gap = int(rng.choice([1, 2, 3, 8, 30]))
        period = int(rng.choice([0, 0, 4, 8, 16]))
        # a motion level with a few spikes, some of them back to back
        level = rng.uniform(0.0, 0.3) * 255 * pixels
        sads = rng.uniform(0.8, 1.2, 64) * level
        for at in rng.choice(np.arange(1, 64), size=int(rng.integers(0, 7)), replace=False):
            sads[at] = rng.uniform(0.3, 1.0) * 255 * pixels
        sads = [min(255 * pixels, int(s)) for s in sads]
        py = scene.SceneCut(threshold, min_gap, pixels)
        ref = scene_np.decisions(sads, threshold, min_gap, pixels,
                                 scheduled={i for i in range(64) if i == 0 or (period and i % period == 1 and i != 1)})
        h = f["create"](threshold, min_gap, pixels)
        assert h
        try:
            for idx, sad in enumerate(sads):
                scheduled = idx == 0 or (period > 0 and idx % period == 1 and idx != 1)
                want = py.push(idx, sad, scheduled)
                got = f["push"](h, idx, sad, 1 if scheduled else 0)
                assert got == (1 if want else 0), (case, idx)
                mafd, score, detected = _last(f, h)
                assert mafd == py.mafd and score == py.score and detected == py.detected, (case, idx)
                assert (mafd, score, detected, bool(got)) == (ref[idx]["mafd"], ref[idx]["score"], ref[idx]["detected"],
                                                             ref[idx]["intra"]), (case, idx)
                returned_one += got
                detected_some += detected
                gap_held += detected and not got
        finally:
            f["destroy"](h)
    assert returned_one > 400 and detected_some > 200 and gap_held > 20      # the cases reach every branch


# ------------------------------------------------------------------------------------------------------ the worked clip
@pytest.fixture(scope="module")
def clip_sads():
    return scene_np.clip_sads(scene_np.clip(H, W))


def test_worked_clip_sads(clip_sads):
    assert len(clip_sads) == 20
    assert clip_sads[1:11] == [655509, 652459, 644830, 641328, 644550, 643639, 642363, 635183, 1354888, 621848]


@pytest.mark.parametrize("gap,scheduled,want_intra", [
    (8, (0,), [0, 9]),
    (1, (0,), [0, 9, 12]),
    (2, (0, 9, 17), [0, 9, 12, 17]),                    # --intra-period 8: I pictures at 9 and 17 by the index
])
def test_worked_clip_decisions(clip_sads, gap, scheduled, want_intra):
    sc = scene.SceneCut(5, gap, H * W)
    intra, detected, scores = [], [], []
    for idx, sad in enumerate(clip_sads):
        if sc.push(idx, sad, idx in scheduled):
            intra.append(idx)
        if sc.detected:
            detected.append(idx)
        scores.append(sc.score)
    print("scores", ["%.2f" % s for s in scores])
    assert detected == [9, 12]
    assert intra == want_intra
    ref = scene_np.decisions(clip_sads, 5, gap, H * W, scheduled)
    assert [r["score"] for r in ref] == scores and [i for i, r in enumerate(ref) if r["intra"]] == want_intra
    # threshold 5 has a wide margin on both sides
    assert min(scores[9], scores[12]) > 10 and max(abs(s) for i, s in enumerate(scores) if i not in (9, 12)) < 0.5


# ------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("threshold,min_gap,pixels", [
    (0.0, 8, 100), (-1.0, 8, 100), (100.5, 8, 100), (float("nan"), 8, 100), (float("inf"), 8, 100),
    (5.0, 0, 100), (5.0, -2, 100), (5.0, 8, 0), (5.0, 8, -5),
])
def test_scd_create_refusals(threshold, min_gap, pixels):
    f = _scd()
    assert not f["create"](threshold, min_gap, pixels)
    assert _lib.lib().dcvc_last_error()
    with pytest.raises(ValueError):
        scene.SceneCut(threshold, min_gap, pixels)


def test_scd_push_refusals_leave_the_detector_unchanged():
    f = _scd()
    assert f["push"](None, 0, 0, 0) < 0 and f["last"](None, None, None, None) < 0
    h = f["create"](100.0, 1, 100)              # 100 is inside (0, 100]
    py = scene.SceneCut(100.0, 1, 100)
    assert h
    try:
        assert f["push"](h, 1, 0, 0) < 0        # picture 0 comes first
        assert b"is next" in _lib.lib().dcvc_last_error()
        assert f["push"](h, 0, -7, 0) == 0      # sad is ignored for picture 0, and nothing is scheduled
        assert py.push(0, -7, False) is False
        assert f["push"](h, 1, 1000, 0) == 0
        assert py.push(1, 1000, False) is False
        before = _last(f, h)
        for idx, sad in [(1, 5), (3, 5), (0, 5), (2, -1), (2, 255 * 100 + 1)]:
            assert f["push"](h, idx, sad, 1) < 0, (idx, sad)
            with pytest.raises(ValueError):
                py.push(idx, sad, True)
            assert _last(f, h) == before == (py.mafd, py.score, py.detected)
        assert f["push"](h, 2, 255 * 100, 0) == 0      # the largest sad there is; the score stays below 100
        assert py.push(2, 255 * 100, False) is False
        assert _last(f, h) == (py.mafd, py.score, py.detected)
        assert f["last"](h, None, None, None) == 0
    finally:
        f["destroy"](h)
    f["destroy"](None)


def test_luma_sad_refusals_come_before_the_device():
    fn = _lib.fn("dcvc_luma_sad", _ci, [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp])
    x, prev, luma, sad = 4096, 8192, 12288, 16384      # never dereferenced: every call below is refused on its arguments
    bad = [
        (None, 3, 16, 16, prev, luma, sad), (x, 3, 16, 16, prev, None, sad), (x, 3, 16, 16, prev, luma, None),
        (x, 3, 0, 16, prev, luma, sad), (x, 3, 16, 0, prev, luma, sad), (x, 0, 16, 16, prev, luma, sad),
        (x, 3, -4, 16, None, luma, sad), (x, -3, 16, 16, None, luma, sad),
        (x, 3, 16385, 16, prev, luma, sad), (x, 3, 16, 16385, prev, luma, sad),
        (x, 3, 16, 16, luma, luma, sad),
    ]
    for args in bad:
        assert fn(*args, None) == -1, args
        assert b"luma_sad" in _lib.lib().dcvc_last_error()


def _run(args):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=120)


def _encode(tmp_path, extra, inter=True):
    args = ["encode", "--intra", str(tmp_path / "missing_i.dcvw"), "-i", str(tmp_path / "missing.yuv"), "-W", "64", "-H", "64",
            "-o", str(tmp_path / "o.bin")]
    if inter:
        args += ["--inter", str(tmp_path / "missing_p.dcvw")]
    return _run(args + extra)


@pytest.mark.parametrize("flag,value", [("--scene-min-gap", "4"), ("--scene-log", "log.json")])
def test_cli_companions_need_scene_cut(tmp_path, flag, value):
    r = _encode(tmp_path, [flag, value])
    assert r.returncode == 2 and flag + " needs --scene-cut" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["0", "-1", "100.5", "nan", "inf", "5x", "", "five"])
def test_cli_threshold_out_of_range_is_refused(tmp_path, value):
    r = _encode(tmp_path, ["--scene-cut", value])
    assert r.returncode == 2 and "--scene-cut must be a threshold in (0, 100]" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["0", "-3", "2x", ""])
def test_cli_min_gap_below_one_is_refused(tmp_path, value):
    r = _encode(tmp_path, ["--scene-cut", "5", "--scene-min-gap", value])
    assert r.returncode == 2 and "--scene-min-gap must be in 1.." in r.stderr, r.stderr


def test_cli_all_intra_runs_are_refused(tmp_path):
    r = _encode(tmp_path, ["--scene-cut", "5"], inter=False)
    assert r.returncode == 2 and "all-intra run" in r.stderr and "--scene-cut" in r.stderr, r.stderr
    r = _encode(tmp_path, ["--scene-cut", "5", "--intra-period", "1"])
    assert r.returncode == 2 and "all-intra run" in r.stderr and "--scene-cut" in r.stderr, r.stderr


def test_cli_batches_are_refused(tmp_path):
    for inter in (True, False):
        r = _encode(tmp_path, ["--scene-cut", "5", "--batch", "2"], inter=inter)
        assert r.returncode == 2 and "--scene-cut cannot be combined with --batch" in r.stderr, r.stderr
