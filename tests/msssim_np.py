"""fp64 numpy restatement of the reference's MS-SSIM (src/utils/metrics.py:27-91 calc_msssim, :86-91 calc_msssim_rgb).

Written from the definitions, not from the reference's code: the 11 x 11 Gaussian (sigma 1.5) of fspecial_gauss is the outer
product of the 1-D taps e / sum(e), so it is applied as a row pass and a column pass over the valid region; the
ndimage.convolve(ones((2, 2)) / 4, mode='reflect')[::2, ::2] downsampling is a 2 x 2 block mean with the last row / column
repeated on an odd side. Agrees with the reference's FFT convolution to a few 1e-15.
"""
import numpy as np

K1, K2, DATA_RANGE = 0.01, 0.03, 255.0
WEIGHTS_5 = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333])
WEIGHTS_4 = np.array([0.0517, 0.3295, 0.3462, 0.2726])


def gauss_taps(size=11, sigma=1.5):
    d = np.arange(size, dtype=np.float64) - size // 2
    e = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return e / e.sum()


def _valid_filter(im, g):
    """separable 'valid' correlation with the symmetric taps g: rows, then columns"""
    n = len(g)
    h, w = im.shape
    rows = sum(g[k] * im[:, k:w - n + 1 + k] for k in range(n))
    return sum(g[k] * rows[k:h - n + 1 + k, :] for k in range(n))


def ssim_cs(a, b):
    """means of the ssim map and of the cs map of one level"""
    g = gauss_taps()
    c1, c2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
    mu1, mu2 = _valid_filter(a, g), _valid_filter(b, g)
    s1 = _valid_filter(a * a, g) - mu1 * mu1
    s2 = _valid_filter(b * b, g) - mu2 * mu2
    s12 = _valid_filter(a * b, g) - mu1 * mu2
    cs = (2 * s12 + c2) / (s1 + s2 + c2)
    ssim = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))
    return ssim.mean(), cs.mean()


def downsample(im):
    """2 x 2 block mean, the last row / column repeated when a side is odd; output side ceil(n / 2)"""
    h, w = im.shape
    p = np.pad(im, ((0, h % 2), (0, w % 2)), mode="edge")
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) * 0.25


def msssim(src, rec):
    """calc_msssim(src, rec) of two H x W planes (any numeric dtype, values in 0..255)"""
    a = np.asarray(src, dtype=np.float64)
    b = np.asarray(rec, dtype=np.float64)
    h, w = a.shape
    if h < 88 or w < 88:
        raise ValueError("MS-SSIM needs both sides >= 88 (the reference asserts), got %dx%d" % (w, h))
    weights = WEIGHTS_4 if h < 176 or w < 176 else WEIGHTS_5
    levels = len(weights)
    ms, mc = [], []
    for _ in range(levels):
        s, c = ssim_cs(a, b)
        ms.append(s)
        mc.append(c)
        a, b = downsample(a), downsample(b)
    with np.errstate(invalid="ignore"):          # a negative cs mean gives NaN, as in the reference
        return float(np.prod(np.array(mc[:-1]) ** weights[:-1]) * ms[-1] ** weights[-1])


def msssim_rgb(rgb, rgb_rec):
    """calc_msssim_rgb: the mean over the three planes of 3 x H x W arrays"""
    return sum(msssim(rgb[i], rgb_rec[i]) for i in range(3)) / 3
