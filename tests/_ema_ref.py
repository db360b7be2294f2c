"""CPU reference of the weight EMA (csrc/optim.hip, ema_weight / ema_elem), in float64.

One update is ``e <- e + w * (p - e)`` with ``w = float32(1 - d)`` and ``d = decay``, or with
warm-up ``d = min(decay, (1 + n) / (10 + n))`` for the update after ``n`` earlier ones."""
import numpy as np


def decay_at(decay, warmup, n):
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def weight32(decay, warmup, n):
    """The fp32 weight the kernels use: rounded once from the double ``1 - d``."""
    return np.float32(1.0 - decay_at(decay, warmup, n))


def step(e, p, w):
    """One update of fp32 inputs, evaluated in float64 (``w`` the fp32-rounded weight)."""
    e, p = np.asarray(e, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return e + np.float64(w) * (p - e)


def recurrence(e0, p, w, steps):
    """``steps`` float64 updates towards a constant ``p``."""
    e = np.asarray(e0, dtype=np.float64)
    for _ in range(steps):
        e = step(e, p, w)
    return e


def closed_form(e0, p, w, steps):
    """e_N = p + (1 - w)^N (e_0 - p) for constant p."""
    e0, p = np.asarray(e0, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return p + (1.0 - np.float64(w)) ** steps * (e0 - p)


def ulp32(x):
    """The spacing of fp32 at |x|."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def bound(e, p):
    """2 ulp32(max(|e|, |p|)): the subtraction rounds by at most 1 ulp of that maximum
    (|p - e| <= 2 max, half an ulp of the difference), scaled by w <= 1, and the fma by at
    most half an ulp of its result, which lies between e and p."""
    return 2.0 * ulp32(np.maximum(np.abs(np.asarray(e, dtype=np.float32)), np.abs(np.asarray(p, dtype=np.float32))))
