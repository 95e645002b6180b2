"""NumPy restatement of the windowed pair moments' contract (include/atsc_hip.h, DESIGN.md "Windowed pair moments"): the
windowed moments' nodes and tree (tests/moments_model.py) with the second stream's value y where those have the position
t; the fit read off the record (atsc_pair_fit); exact values in rational arithmetic and the documented error bounds."""
import math
from fractions import Fraction

import numpy as np

from tests import moments_model as M

TILE = M.TILE
U = M.U

FIELDS = ("count", "mean_x", "m2_x", "mean_y", "m2_y", "c_xy")
FIT_FIELDS = ("covariance", "sample_covariance", "correlation", "slope", "intercept", "r2", "mean_diff")
DTYPE = np.dtype([("count", "<u8")] + [(k, "<f8") for k in FIELDS[1:]])


def window_pair(x, y, begin, count):
    """-> (count, mean_x, m2_x, mean_y, m2_y, c_xy) of x[begin:begin + count] and y[begin:begin + count] as the contract
    defines them: a slot counts where it lies in the window and neither value is NaN"""
    nan = float("nan")
    if count == 0:
        return 0, nan, nan, nan, nan, nan
    kb, ke = begin // TILE, (begin + count - 1) // TILE
    n_slots = (ke - kb + 1) * TILE
    lo = begin - kb * TILE
    sx, sy = np.zeros(n_slots), np.zeros(n_slots)
    sx[lo:lo + count] = x[begin:begin + count]
    sy[lo:lo + count] = y[begin:begin + count]
    ok = np.zeros(n_slots, dtype=bool)
    ok[lo:lo + count] = ~(np.isnan(sx[lo:lo + count]) | np.isnan(sy[lo:lo + count]))
    shape = (-1, TILE)
    n, mx, m2x, my, m2y, c = M.pairwise(M.tile_nodes(sx.reshape(shape), sy.reshape(shape), ok.reshape(shape)))
    if int(n) == 0:
        return 0, nan, nan, nan, nan, nan
    return int(n), float(mx), float(m2x), float(my), float(m2y), float(c)


def windows_pair(x, y, wins):
    """-> structured array (the fields of atsc_window_pair) of the windows (begin, count) of x and y"""
    out = np.zeros(len(wins), dtype=DTYPE)
    for i, (b, c) in enumerate(wins):
        out[i] = window_pair(x, y, int(b), int(c))
    return out


def fit(count, mean_x, m2_x, mean_y, m2_y, c_xy):
    """atsc_pair_fit of one record -> (covariance, sample_covariance, correlation, slope, intercept, r2, mean_diff)"""
    nan = np.float64("nan")
    if count == 0:
        return (nan,) * 7
    mean_x, m2_x, mean_y, m2_y, c_xy = (np.float64(v) for v in (mean_x, m2_x, mean_y, m2_y, c_xy))
    with np.errstate(all="ignore"):
        cov = c_xy / np.float64(count)
        scov = c_xy / np.float64(count - 1) if count >= 2 else nan
        if m2_x > 0 and m2_y > 0:
            corr = (c_xy / np.sqrt(m2_x)) / np.sqrt(m2_y)
            corr = np.float64(1.0) if corr > 1.0 else np.float64(-1.0) if corr < -1.0 else corr
        else:
            corr = nan
        slope = c_xy / m2_x if m2_x > 0 else nan
        sm = slope * mean_x
        return cov, scov, corr, slope, mean_y - sm, corr * corr, mean_x - mean_y


def exact_pair(vx, vy):
    """-> (count, mean_x, m2_x, mean_y, m2_y, c_xy, mean|x|, mean|y|) as Fractions, over the slots where neither vx nor vy
    is NaN"""
    vx, vy = np.asarray(vx, dtype=np.float64), np.asarray(vy, dtype=np.float64)
    idx = [i for i in range(len(vx)) if not (math.isnan(vx[i]) or math.isnan(vy[i]))]
    n = len(idx)
    if n == 0:
        return (0,) + (None,) * 7
    xs = [M._scaled_int(vx[i]) for i in idx]
    ys = [M._scaled_int(vy[i]) for i in idx]
    sx, sy = sum(xs), sum(ys)
    sxx, syy, sxy = sum(a * a for a in xs), sum(a * a for a in ys), sum(a * b for a, b in zip(xs, ys))
    one, two = Fraction(1, 1 << 1074), Fraction(1, 1 << 2148)
    return (n, Fraction(sx, n) * one, (Fraction(sxx) - Fraction(sx * sx, n)) * two, Fraction(sy, n) * one,
            (Fraction(syy) - Fraction(sy * sy, n)) * two, (Fraction(sxy) - Fraction(sx * sy, n)) * two,
            Fraction(sum(abs(a) for a in xs), n) * one, Fraction(sum(abs(a) for a in ys), n) * one)


def bounds(n, mean_x, m2_x, mean_y, m2_y):
    """the documented bounds (b_mean / mean|.|, b_m2_x, b_m2_y, b_c_xy) from the exact values: with L = max(1,
    ceil(log2 n)) and kappa = sqrt(1 + n mean^2 / m2), (L + 2) u times (1, kappa_x m2_x, kappa_y m2_y, kappa_x kappa_y
    sqrt(m2_x m2_y)).  kappa^2 m2 = m2 + n mean^2 keeps the products finite where m2 == 0."""
    L = max(1, math.ceil(math.log2(n))) if n > 1 else 1
    k = (L + 2) * U
    ax = float(m2_x) + n * float(mean_x) ** 2  # kappa_x^2 m2_x
    ay = float(m2_y) + n * float(mean_y) ** 2
    return k, k * math.sqrt(float(m2_x) * ax), k * math.sqrt(float(m2_y) * ay), k * math.sqrt(ax * ay)
