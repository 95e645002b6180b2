"""NumPy restatement of the windowed aggregates' contract (include/atsc_hip.h, DESIGN.md "Windowed aggregates"):
count / min / max / first / last of a window, and its sum in the documented order, from the full decode's samples."""
import math

import numpy as np

TILE = 2048


def tile_sums(t):
    """sums of tiles t[k, 0..2047] (NaN and out-of-window slots already -0.0): per virtual lane v the pairs
    x[512 q + 2 v] + x[512 q + 2 v + 1] as (p0 + p1) + (p2 + p3), then a halving tree over the 256 lanes"""
    y = np.asarray(t, dtype=np.float64).reshape(-1, 4, 256, 2)
    with np.errstate(invalid="ignore", over="ignore"):  # +Inf + -Inf is NaN, as on the GPU
        p = y[..., 0] + y[..., 1]
        s = (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])
        h = 128
        while h >= 1:
            s = s[:, :h] + s[:, h:2 * h]
            h //= 2
    return s[:, 0]


def pairwise(q):
    """q[i] = q[2 i] + q[2 i + 1] level by level, an odd last entry added to -0.0"""
    q = np.asarray(q, dtype=np.float64)
    if len(q) == 0:
        return -0.0
    with np.errstate(invalid="ignore", over="ignore"):
        while len(q) > 1:
            if len(q) % 2:
                q = np.append(q, -0.0)
            q = q[0::2] + q[1::2]
    return q[0]


def window_sum(x, begin, count):
    """the sum of x[begin:begin + count] in the documented order (NaN excluded; +0.0 when no sample counts)"""
    v = np.asarray(x[begin:begin + count], dtype=np.float64)
    ok = ~np.isnan(v)
    if not ok.any():
        return 0.0
    kb, ke = begin // TILE, (begin + count - 1) // TILE
    seg = np.full((ke - kb + 1) * TILE, -0.0)
    lo = begin - kb * TILE
    seg[lo:lo + count] = np.where(ok, v, -0.0)
    return float(pairwise(tile_sums(seg.reshape(-1, TILE))))


def window_stats(x, begin, count):
    """-> (count, min, max, sum, first, last) of x[begin:begin + count] as the contract defines them"""
    v = np.asarray(x[begin:begin + count], dtype=np.float64)
    ok = ~np.isnan(v)
    n = int(ok.sum())
    nan = float("nan")
    mn = float(np.min(v[ok])) if n else nan
    mx = float(np.max(v[ok])) if n else nan
    first = float(v[0]) if count else nan
    last = float(v[-1]) if count else nan
    return n, mn, mx, window_sum(x, begin, count), first, last


def error_bound(v):
    """(ceil(log2 count) + 2) 2^-53 sum|x| over the finite samples of v"""
    v = np.asarray(v, dtype=np.float64)
    v = v[~np.isnan(v)]
    if len(v) == 0:
        return 0.0
    return (math.ceil(math.log2(max(len(v), 1))) + 2) * 2.0 ** -53 * float(math.fsum(np.abs(v)))
