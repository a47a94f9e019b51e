"""Scene-cut detection of the coding loop (no reference counterpart: test_video.py:204-213 decides picture
types from the picture index alone).

``luma_sad`` is a thin wrapper over the C-ABI entry point ``dcvc_luma_sad`` (include/dcvc_amd_ops.h): the 8-bit luma plane
of a model input and its sum of absolute differences against the previous picture's plane, on the GPU, on
``torch.cuda.current_stream()``. ``SceneCut`` restates ``dcvc_scd_*`` (include/dcvc_amd_rc.h, csrc/codec/rate_control.cpp)
operation for operation, the way rate_control.py restates the controller; the tests hold the two against each other with
``==``. ``rate_control.code_sequence(..., intra_at=...)`` takes the decisions.
"""
import ctypes
import math

from . import _lib

_vp, _ci = ctypes.c_void_p, ctypes.c_int
_fns = {}


def _fn(name, argtypes):
    if name not in _fns:
        _fns[name] = _lib.fn(name, _ci, argtypes)
    return _fns[name]


def luma_sad(x, prev=None, channel=0):
    """x: the model input of one or more pictures, a float16 CUDA tensor [1, C, H, W] in channels_last memory (pixel stride
    C halfs - 3 for one picture, 24 for an 8-picture chunk, where picture j's luma is channel 3 j). prev: the uint8 CUDA
    plane [H, W] a previous call returned, or None. Returns (luma8 [H, W] uint8 CUDA tensor, sad int): luma8 =
    clamp(rint((x[channel] + 0.5) * 255), 0, 255) in fp32, sad = sum |luma8 - prev| (0 without prev). Reading the sum
    waits for the stream."""
    import torch
    if x.dtype != torch.float16 or not x.is_cuda or x.dim() != 4 or x.shape[0] != 1:
        raise ValueError("luma_sad: a float16 CUDA tensor [1, C, H, W] expected, got %s %s" % (x.dtype, tuple(x.shape)))
    _, C, H, W = x.shape
    if not 0 <= channel < C:
        raise ValueError("luma_sad: channel %d outside the %d channels of x" % (channel, C))
    if x.stride(1) != 1 or x.stride(3) != C or x.stride(2) != W * C:
        raise ValueError("luma_sad: x must be dense in channels_last memory ([H][W][C])")
    if prev is not None and (prev.dtype != torch.uint8 or prev.device != x.device or tuple(prev.shape) != (H, W)
                             or not prev.is_contiguous()):
        raise ValueError("luma_sad: prev must be a contiguous uint8 tensor [%d, %d] on x's device" % (H, W))
    luma = torch.empty((H, W), dtype=torch.uint8, device=x.device)
    sad = torch.empty(1, dtype=torch.int64, device=x.device)
    fn = _fn("dcvc_luma_sad", [_vp, _ci, _ci, _ci, _vp, _vp, _vp, _vp])
    _lib.check(fn(_vp(x.data_ptr() + 2 * channel), C, H, W, _vp(prev.data_ptr()) if prev is not None else None,
                  _vp(luma.data_ptr()), _vp(sad.data_ptr()), _vp(torch.cuda.current_stream(x.device).cuda_stream)))
    return luma, int(sad.item())


class SceneCut:
    """dcvc_scd_* in Python. Pictures are pushed in source order with the luma SAD against their predecessor.

    mafd = 100.0 * sad / (256.0 * pixels): the mean absolute luma difference in percent of full range. score = mafd - base,
    base = the mafd of the most recent pushed pair that was not detected; with no base yet the score is 0 and the pair sets
    the base. detected = score >= threshold. A detected pair does not update the base: the picture after a cut is measured
    against the motion level before it, not against the spike."""

    def __init__(self, threshold, min_gap, pixels):
        threshold = float(threshold)
        if not math.isfinite(threshold) or not threshold > 0.0 or threshold > 100.0:
            raise ValueError("the threshold must be in (0, 100] (percent of full range)")
        if int(min_gap) < 1:
            raise ValueError("min_gap must be at least 1")
        if int(pixels) < 1:
            raise ValueError("pixels must be at least 1")
        self.threshold, self.min_gap, self.pixels = threshold, int(min_gap), int(pixels)
        self.mafd, self.score, self.detected = 0.0, 0.0, False
        self._base, self._next, self._last_intra = None, 0, None

    def push(self, idx, sad, scheduled_intra):
        """True: code picture idx as an I picture - it is scheduled as one, or it is detected and at least min_gap pictures
        after the last picture this returned True for (none yet: far enough). A refused push changes nothing."""
        idx, sad = int(idx), int(sad)
        if idx != self._next:
            raise ValueError("picture %d pushed, %d is next" % (idx, self._next))
        if idx > 0 and not 0 <= sad <= 255 * self.pixels:
            raise ValueError("sad %d is outside [0, 255 * pixels]" % sad)
        self._next = idx + 1
        if idx == 0:
            self.mafd, self.score, self.detected = 0.0, 0.0, False
        else:
            self.mafd = 100.0 * float(sad) / (256.0 * float(self.pixels))
            self.score = self.mafd - self._base if self._base is not None else 0.0
            self.detected = self.score >= self.threshold
            if not self.detected:
                self._base = self.mafd
        intra = bool(scheduled_intra) or (self.detected and (self._last_intra is None or idx - self._last_intra >= self.min_gap))
        if intra:
            self._last_intra = idx
        return intra


__all__ = ["luma_sad", "SceneCut"]
