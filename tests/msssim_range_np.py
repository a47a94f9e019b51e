"""fp64 numpy MS-SSIM at a given data range (DCVC-FM src/utils/metrics.py calc_msssim(img1, img2, data_range)): the
restatement of tests/msssim_np.py with C1 = (K1 data_range)^2 and C2 = (K2 data_range)^2. data_range = 255 is msssim_np.msssim."""
import numpy as np

from msssim_np import K1, K2, WEIGHTS_4, WEIGHTS_5, _valid_filter, downsample, gauss_taps


def ssim_cs(a, b, data_range):
    g = gauss_taps()
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    mu1, mu2 = _valid_filter(a, g), _valid_filter(b, g)
    s1 = _valid_filter(a * a, g) - mu1 * mu1
    s2 = _valid_filter(b * b, g) - mu2 * mu2
    s12 = _valid_filter(a * b, g) - mu1 * mu2
    cs = (2 * s12 + c2) / (s1 + s2 + c2)
    ssim = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return ssim.mean(), cs.mean()


def msssim(src, rec, data_range):
    a = np.asarray(src, dtype=np.float64)
    b = np.asarray(rec, dtype=np.float64)
    h, w = a.shape
    if h < 88 or w < 88:
        raise ValueError("MS-SSIM needs both sides >= 88, got %dx%d" % (w, h))
    weights = WEIGHTS_4 if h < 176 or w < 176 else WEIGHTS_5
    ms, mc = [], []
    for _ in range(len(weights)):
        s, c = ssim_cs(a, b, data_range)
        ms.append(s)
        mc.append(c)
        a, b = downsample(a), downsample(b)
    with np.errstate(invalid="ignore"):
        return float(np.prod(np.array(mc[:-1]) ** weights[:-1]) * ms[-1] ** weights[-1])
