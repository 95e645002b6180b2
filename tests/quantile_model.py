"""NumPy restatement of the windowed quantiles' contract (include/atsc_hip.h, DESIGN.md "Windowed quantiles"): the
window's non-NaN samples in IEEE total order, the rank rule and NumPy's _lerp evaluated without fused multiply-add."""
import math

import numpy as np

LINEAR, LOWER, HIGHER, NEAREST = 0, 1, 2, 3
METHOD_NAMES = {LINEAR: "linear", LOWER: "lower", HIGHER: "higher", NEAREST: "nearest"}


def keys(x):
    """total-order keys: bits ^ (sign ? 0xFF..FF : 0x80..00); -0.0 sorts before +0.0"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def sort_total(x):
    x = np.asarray(x, dtype=np.float64)
    x = x[~np.isnan(x)]
    return x[np.argsort(keys(x), kind="stable")]


def level(s, q, method):
    """level q of the sorted non-NaN samples s (NaN when s is empty)"""
    n = len(s)
    if n == 0:
        return math.nan
    v = float(n - 1) * float(q)  # one f64 multiply
    if method == LOWER:
        return float(s[math.floor(v)])
    if method == HIGHER:
        return float(s[math.ceil(v)])
    if method == NEAREST:
        return float(s[int(np.rint(v))])  # ties to even, as numpy.around
    lo = math.floor(v)
    hi = min(lo + 1, n - 1)
    t = v - lo
    a = float(s[lo])
    if t == 0.0 or lo == hi:
        return a
    b = float(s[hi])
    d = b - a  # Python floats: each operation rounded on its own, no contraction
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def quantiles(x, levels, method=LINEAR):
    s = sort_total(x)
    return np.array([level(s, q, method) for q in np.atleast_1d(levels)], dtype=np.float64)


def windows(samples, begins, counts, levels, method=LINEAR):
    """(n_windows, n_levels) array of the levels of every window of samples"""
    lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    out = np.empty((len(begins), len(lv)), dtype=np.float64)
    for i, (b, c) in enumerate(zip(begins, counts)):
        out[i] = quantiles(samples[int(b):int(b) + int(c)], lv, method)
    return out
