"""Brute-force float64 SSIM (pytorch_msssim.ssim v1.0.0: 11x11 Gaussian window, sigma
1.5, valid padding, mean over the map) in numpy, written from the definition with an
explicit 2-D window over every patch -- no separable filtering, no torch, no code shared
with ``functional.ssim`` -- and the input pairs of the SSIM tests."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

WIN, SIGMA = 11, 1.5


def window2d():
    c = np.arange(WIN, dtype=np.float64) - WIN // 2
    w = np.exp(-(c[:, None] ** 2 + c[None, :] ** 2) / (2.0 * SIGMA ** 2))
    return w / w.sum()


def _wmean(a, w):
    """Weighted mean of every WIN x WIN patch of a [n, c, h, w] array."""
    patches = sliding_window_view(a, (WIN, WIN), axis=(2, 3))      # [n, c, h-10, w-10, 11, 11]
    return (patches * w).sum(axis=(-2, -1))


def ssim(x, y, data_range=1.0):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = window2d()
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = _wmean(x, w), _wmean(y, w)
    vx = _wmean(x * x, w) - mx * mx
    vy = _wmean(y * y, w) - my * my
    cov = _wmean(x * y, w) - mx * my
    smap = ((2 * mx * my + c1) * (2 * cov + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return float(smap.mean())


def ssim_loss(x, y, data_range=1.0):
    return 1.0 - ssim(x, y, data_range)


def make_pair(shape, seed):
    """(pred, clean) as float32 [n, c, h, w]: every clean plane a smooth texture, the sum
    of two sinusoids (amplitude 0.4 each) with seeded frequencies and phases, and
    pred = clean + (25/255*2) * N(0, 1).  No flat planes: there q - m1^2 cancels and an
    fp32 evaluation says nothing about the kernel."""
    n, c, h, w = shape
    rng = np.random.default_rng(seed)
    i = np.arange(h, dtype=np.float64)[:, None]
    j = np.arange(w, dtype=np.float64)[None, :]
    clean = np.empty(shape, np.float64)
    for b in range(n):
        for ch in range(c):
            f = rng.uniform(0.02, 0.2, size=(2, 2))
            ph = rng.uniform(0.0, 2 * np.pi, size=2)
            clean[b, ch] = sum(0.4 * np.sin(2 * np.pi * (f[k, 0] * i + f[k, 1] * j) + ph[k]) for k in range(2))
    pred = clean + (25.0 / 255.0 * 2.0) * rng.standard_normal(shape)
    return pred.astype(np.float32), clean.astype(np.float32)
