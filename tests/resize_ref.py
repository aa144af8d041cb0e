"""float64 numpy restatement of the antialiased resize (F.interpolate(mode='bilinear' | 'bicubic', align_corners=False, antialias=True)),
the case table of its tests and their pointwise error bound.  include/gnerf_hip.h (gnerf_resize_aa_*) states the definition:

    scale = in / out, or 1 / scale_factor where a given scale factor is not recomputed
    S = 2 (bilinear: 1 - |x| on |x| < 1) or 4 (bicubic: Keys' cubic with a = -0.5 on |x| < 2)
    support = S/2 * scale if scale >= 1 else S/2;  invscale = 1 / scale if scale >= 1 else 1
    output i: center = scale * (i + 0.5), xmin = max(int(center - support + 0.5), 0), xsize = min(int(center + support + 0.5), in) - xmin,
              w_j = f((j + xmin - center + 0.5) * invscale), j < xsize, divided by their sum if that is not 0
    y = W_y x W_x^T per (n, c); the gradient is dx = W_y^T dy W_x.
"""

import functools
import math

import numpy as np


def filter_at(mode, x):
    x = abs(x)
    if mode == 'bilinear':
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


@functools.lru_cache(maxsize=None)
def band_matrix(size_in, size_out, mode='bilinear', scale=None):
    """W [size_out, size_in] float64 of one axis; scale: the in / out ratio to use, or None (size_in / size_out).  Read-only (cached)."""
    scale = float(scale) if scale is not None and scale > 0 else size_in / size_out
    half = 2.0 if mode == 'bicubic' else 1.0
    support = half * scale if scale >= 1.0 else half
    invscale = 1.0 / scale if scale >= 1.0 else 1.0
    W = np.zeros([size_out, size_in], dtype=np.float64)
    for i in range(size_out):
        center = scale * (i + 0.5)
        xmin = max(int(center - support + 0.5), 0)
        xsize = min(int(center + support + 0.5), size_in) - xmin
        w = np.array([filter_at(mode, (j + xmin - center + 0.5) * invscale) for j in range(xsize)], dtype=np.float64)
        total = w.sum()
        if total != 0.0:
            w = w / total
        W[i, xmin:xmin + xsize] = w
    W.setflags(write=False)
    return W


def taps(W):
    """The largest number of non-zero band entries of a row (forward) -- K of the bound; of a column: taps(W.T)."""
    return int((W != 0).sum(axis=1).max())


def matrices(in_size, out_size, mode='bilinear', scales=(None, None)):
    return band_matrix(in_size[0], out_size[0], mode, scales[0]), band_matrix(in_size[1], out_size[1], mode, scales[1])


def forward(x, out_size, mode='bilinear', scales=(None, None)):
    """x [..., H, W] float64 -> [..., out_h, out_w]."""
    Wy, Wx = matrices(x.shape[-2:], out_size, mode, scales)
    return Wy @ x @ Wx.T


def transposed(dy, in_size, mode='bilinear', scales=(None, None)):
    """dy [..., out_h, out_w] float64 -> dx [..., H, W]."""
    Wy, Wx = matrices(in_size, dy.shape[-2:], mode, scales)
    return Wy.T @ dy @ Wx


def output_size(in_size, size=None, scale_factor=None):
    if size is not None:
        return tuple(size)
    return tuple(int(math.floor(s * f)) for s, f in zip(in_size, scale_factor))


def kernel_scales(scale_factor):
    """The in / out ratios the resampling uses for a given (not recomputed) scale factor."""
    return (None, None) if scale_factor is None else tuple(1.0 / f for f in scale_factor)


# name -> (in_size, size, scale_factor): the shapes of the issue's case list
CASES = {
    'up2_5x7': ((5, 7), (10, 14), None),                       # the hot upsampling in small
    'up2_8x8': ((8, 8), (16, 16), None),
    'down8_40x24': ((40, 24), (5, 3), None),                   # 16-17 taps
    'frac_down_17x13': ((17, 13), (5, 7), None),
    'frac_up_5x7': ((5, 7), (17, 13), None),
    'mixed_70x45': ((70, 45), (37, 83), None),                 # down in one axis, up in the other, several tiles per axis
    'identity_7x7': ((7, 7), (7, 7), None),
    'one_pixel_1x3': ((1, 3), (4, 2), None),
    'one_pixel_33x40': ((33, 40), (32, 1), None),
    'scale_factor_20x30': ((20, 30), None, (0.37, 0.61)),      # the GIVEN scale is what the resampling uses
}


def case(name):
    """-> (in_size, out_size, scales)"""
    in_size, size, scale_factor = CASES[name]
    return in_size, output_size(in_size, size, scale_factor), kernel_scales(scale_factor)


def image(n, c, size, seed=0):
    """A float64 test image in about [-2, 2] with a smooth part and noise, values exactly representable in float16 (so that float16 and
    float32 kernels see the same numbers as the float64 restatement)."""
    rng = np.random.default_rng(seed + 1000 * n + 31 * c + size[0] * 7 + size[1])
    yy, xx = np.meshgrid(np.linspace(-1, 1, size[0]), np.linspace(-1, 1, size[1]), indexing='ij')
    x = rng.standard_normal([n, c, *size]) * 0.7 + np.sin(3 * yy + 2 * xx) + 0.3
    return x.astype(np.float16).astype(np.float64)


U32 = 2.0 ** -24


def error_bound(Wy, Wx, x, y_ref, half_output):
    """Pointwise bound on |kernel - restatement| for y = Wy x Wx^T evaluated with float32 weights, products and sums:
        gamma * (|Wy| |x| |Wx|^T) + rho,   gamma = (K_y + K_x + 8) * 2^-24,  K = the axis' largest tap count,
        rho = 0 for float32 output, 2^-11 |y| + 2^-24 for float16 output (its one rounding, and the subnormal step).
    Where it comes from: each weight is one float32 rounding of its float64 value (1 u), a K-term float32 dot product loses at most K u
    relative to sum |w| |x| (fmaf: one rounding per term), the horizontal result feeds the vertical one: (K_x + 1) + (K_y + 1) u to first
    order, and the remaining 6 u cover second-order terms and the float32 output rounding.  The transposed operator takes (Wy^T, Wx^T)."""
    gamma = (taps(Wy) + taps(Wx) + 8) * U32
    bound = gamma * (np.abs(Wy) @ np.abs(x) @ np.abs(Wx).T)
    if half_output:
        bound = bound + 2.0 ** -11 * np.abs(y_ref) + 2.0 ** -24
    return bound
