"""Vectorised NumPy model of the windowed across quantiles' contract (include/atsc_hip.h, DESIGN.md "Windowed across
quantiles"): per position the samples of the N streams, the NaN ones dropped, in IEEE total order, then the windowed
quantiles' rank rule (tests/quantile_model.py's `level`) with every float64 operation rounded on its own.  Whole arrays
at a time: 10^5 positions take milliseconds.  tests/test_across_quantile_host.py holds it to quantile_model.level
position by position."""
import numpy as np

from tests import across_model
from tests import quantile_model as Q

LINEAR, LOWER, HIGHER, NEAREST = Q.LINEAR, Q.LOWER, Q.HIGHER, Q.NEAREST
KEY_NAN = np.uint64(0xFFFFFFFFFFFFFFFF)  # above every sample's key


def sorted_columns(x):
    """x: (N, P) samples, a column per position.  -> (s, n): the columns sorted by the total-order key with the NaN
    samples behind the others, and the number of samples that are not NaN per position"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    nan = np.isnan(x)
    k = np.where(nan, KEY_NAN, Q.keys(x))
    s = np.take_along_axis(x, np.argsort(k, axis=0, kind="stable"), axis=0)
    return s, (~nan).sum(axis=0)


def _at(s, idx):
    return np.take_along_axis(s, idx[None, :].astype(np.int64), axis=0)[0]


def level(s, n, q, method):
    """level q of every position of sorted_columns' (s, n): quantile_model.level, elementwise"""
    some = n > 0
    m = np.where(some, n, 1)  # (a position without a sample is evaluated as one of a single sample and then set to NaN)
    v = (m - 1).astype(np.float64) * np.float64(q)  # one f64 multiply
    if method == LOWER:
        r = _at(s, np.floor(v))
    elif method == HIGHER:
        r = _at(s, np.ceil(v))
    elif method == NEAREST:
        r = _at(s, np.rint(v))  # ties to even
    else:
        f = np.floor(v)
        lo = f.astype(np.int64)
        hi = np.minimum(lo + 1, m - 1)
        t = v - f
        a, b = _at(s, lo), _at(s, hi)
        with np.errstate(invalid="ignore", over="ignore"):
            d = b - a
            up = b - d * (1.0 - t)  # each operation a ufunc call of its own: no contraction
            down = a + d * t
        r = np.where((t == 0.0) | (lo == hi), a, np.where(t >= 0.5, up, down))
    return np.where(some, r, np.nan)


def rows(x, levels, method=LINEAR):
    """x: (N, P) samples.  -> (P, n_q) array: row p the levels of position p"""
    s, n = sorted_columns(x)
    lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    return np.stack([level(s, n, q, method) for q in lv], axis=1) if len(lv) else np.empty((s.shape[1], 0))


def across_quantiles(fulls, begins, counts, levels, stride=1, method=LINEAR):
    """-> (rows, off) of the call over the decoded streams `fulls` (sample j of one goes with sample j of every other):
    the positions of the ranges as the across numbers them (tests/across_model.py)"""
    off = across_model.offsets(counts, stride)
    idx = [int(b) + int(stride) * np.arange(across_model.outputs(c, stride), dtype=np.int64) for b, c in zip(begins, counts)]
    idx = np.concatenate(idx) if idx else np.empty(0, dtype=np.int64)
    x = np.stack([np.asarray(f, dtype=np.float64)[idx] for f in fulls])
    return rows(x, levels, method), off


def same(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))
