"""float64 restatement of SSIM / MS-SSIM for the tests of torch_utils/ops/ssim.py and csrc/ssim.hip.

numpy only, and deliberately NOT separable: every windowed mean is one direct 2-D sum with the outer(g, g) window over
numpy.lib.stride_tricks.sliding_window_view, so that it shares no code path (and no summation order) with the implementation.
"""

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(k=11, sigma=1.5):
    i = np.arange(k, dtype=np.float64) - k // 2
    g = np.exp(-(i * i) / (2.0 * sigma * sigma))
    return g / g.sum()


def _mean2d(a, w2):
    """a [N, C, H, W] -> [N, C, H-k+1, W-k+1]: the outer-product window applied directly in 2-D."""
    k = w2.shape[0]
    n, c, h, w = a.shape
    out = np.empty((n, c, h - k + 1, w - k + 1), dtype=np.float64)
    for i in range(n):
        for j in range(c):
            out[i, j] = np.einsum('hwij,ij->hw', sliding_window_view(a[i, j], (k, k)), w2)
    return out


def ssim_pair(X, Y, data_range=255.0, k=11, sigma=1.5, K=(0.01, 0.03), g=None):
    """(ssim [N, C], cs [N, C]) in float64."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    g = window(k, sigma) if g is None else np.asarray(g, dtype=np.float64)
    w2 = np.outer(g, g)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = _mean2d(X, w2), _mean2d(Y, w2)
    s1 = _mean2d(X * X, w2) - mu1 * mu1
    s2 = _mean2d(Y * Y, w2) - mu2 * mu2
    s12 = _mean2d(X * Y, w2) - mu1 * mu2
    cs_map = (2 * s12 + C2) / (s1 + s2 + C2)
    ssim_map = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs_map
    return ssim_map.mean(axis=(2, 3)), cs_map.mean(axis=(2, 3))


def ssim(X, Y, data_range=255.0, size_average=True, k=11, sigma=1.5, K=(0.01, 0.03), nonnegative=False):
    s, _ = ssim_pair(X, Y, data_range, k, sigma, K)
    if nonnegative:
        s = np.maximum(s, 0.0)
    return s.mean() if size_average else s.mean(axis=1)


def _avg_pool2(a):
    """F.avg_pool2d(kernel 2, padding = side % 2): zero padding that counts in the mean, windows that do not fit are dropped."""
    n, c, h, w = a.shape
    ph, pw = h % 2, w % 2
    a = np.pad(a, ((0, 0), (0, 0), (ph, ph), (pw, pw)))
    oh, ow = (h + 2 * ph) // 2, (w + 2 * pw) // 2
    a = a[:, :, :2 * oh, :2 * ow]
    return a.reshape(n, c, oh, 2, ow, 2).mean(axis=(3, 5))


def ms_ssim(X, Y, data_range=255.0, size_average=True, k=11, sigma=1.5, K=(0.01, 0.03), weights=MS_WEIGHTS):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    value = 1.0
    for level, wt in enumerate(weights):
        s, cs = ssim_pair(X, Y, data_range, k, sigma, K)
        if level < len(weights) - 1:
            value = value * np.maximum(cs, 0.0) ** wt
            X, Y = _avg_pool2(X), _avg_pool2(Y)
        else:
            value = value * np.maximum(s, 0.0) ** wt
    return value.mean() if size_average else value.mean(axis=1)
