"""numpy reference of the scene-cut measurement and score (TEST INFRASTRUCTURE ONLY): what dcvc_luma_sad
and dcvc_scd_* are defined to compute, written once more, and the clip with two cuts the tests code."""
import numpy as np

from dcvc_amd import synthetic
from oracle import frame_io

# the worked clip: three scenes of synthetic pictures; `index` is the picture index, so every scene pans on and stays
# below the generator's pan wrap at index 24 (itself a jump)
CLIP_SEEDS = [3] * 9 + [11] * 3 + [4] * 8
CLIP_CUTS = (9, 12)


def luma8(x0):
    """fp16 luma channel of the model input (value / max - 0.5) -> uint8: clamp(rint((fp32(x0) + 0.5) * 255), 0, 255), two
    fp32 operations and a round half to even; NaN counts as 0."""
    v = (np.asarray(x0, dtype=np.float16).astype(np.float32) + np.float32(0.5)) * np.float32(255.0)
    assert v.dtype == np.float32
    r = np.rint(v)
    r = np.where(np.isnan(r), np.float32(0), r)
    return np.clip(r, 0, 255).astype(np.uint8)


def sad(a, b):
    """exact sum of absolute differences of two uint8 planes"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())


def decisions(sads, threshold, min_gap, pixels, scheduled=()):
    """The mafd / score loop over sads[idx] = SAD of picture idx against idx - 1 (sads[0] is not read). Returns one
    dict(mafd, score, detected, intra) per picture."""
    out, base, last_intra = [], None, None
    for idx in range(len(sads)):
        if idx == 0:
            mafd, score = 0.0, 0.0
        else:
            mafd = 100.0 * sads[idx] / (256.0 * pixels)
            score = 0.0 if base is None else mafd - base
        detected = idx > 0 and score >= threshold
        if idx > 0 and not detected:
            base = mafd
        intra = idx in scheduled or (detected and (last_intra is None or idx - last_intra >= min_gap))
        if intra:
            last_intra = idx
        out.append(dict(mafd=mafd, score=score, detected=detected, intra=intra))
    return out


def clip(H, W):
    """the 20 pictures [(y u8 [H, W], uv u8 [2, H/2, W/2])] of the worked clip"""
    return [synthetic.synthetic_frame_yuv420(H, W, index=i, seed=s) for i, s in enumerate(CLIP_SEEDS)]


def clip_sads(frames):
    """sads[idx] of pictures as the tool sees them: through the harness's conversion to the model input and back to luma8"""
    planes = [luma8(frame_io.yuv420_to_x(y, uv)[..., 0]) for y, uv in frames]
    return [0] + [sad(planes[i], planes[i - 1]) for i in range(1, len(planes))]
