"""NumPy restatement of the windowed rolling quantiles' contract (include/atsc_hip.h, DESIGN.md "Windowed rolling
quantiles"), from the full decode's samples: the row of the position whose window is [lo, lo + w) is the windowed
quantiles' row of the listed window (lo, w) -- the window's non-NaN samples in the total order of the quantiles' key, the
levels by tests/quantile_model.py's level().

rows() sorts the keys of many windows at once (a sliding view over the stream's keys, sorted per window in blocks of
positions) and takes every level through quantile_model.level; literal() is the contract read literally, one listed
window at a time through quantile_model.windows.  tests/test_rolling_quantile_host.py holds the two together."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from tests import quantile_model as QM
from tests import rolling_model as R

LINEAR, LOWER, HIGHER, NEAREST = QM.LINEAR, QM.LOWER, QM.HIGHER, QM.NEAREST
METHODS = (LINEAR, LOWER, HIGHER, NEAREST)
MAX_WIDTH = 8192
KEY_NAN = np.uint64(0xFFFFFFFFFFFFFFFF)  # above every sample's key
BLOCK = 1 << 22                          # keys sorted at once
outputs = R.outputs


def span_keys(w):
    """the slots one task sorts (the P rule): the least power of two in [512, 8192] that holds two windows,
    8192 above that"""
    p = 512
    while p < 8192 and p < 2 * w:
        p *= 2
    return p


def task_positions(w, s):
    """B: the positions one task holds"""
    return (span_keys(w) - w) // s + 1


def offsets(counts, w, s):
    """the ranges' row offsets: range i's rows are [off[i], off[i + 1])"""
    return np.concatenate([[0], np.cumsum([outputs(int(c), w, s) for c in counts])]).astype(np.uint64)


def positions(begins, counts, w, s):
    """the first sample of every position's window, range after range"""
    lo = [int(b) + s * np.arange(outputs(int(c), w, s), dtype=np.int64) for b, c in zip(begins, counts)]
    return np.concatenate(lo) if lo else np.zeros(0, dtype=np.int64)


def stream_keys(x):
    """the total-order keys of the samples, KEY_NAN where the sample is NaN"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return np.where(np.isnan(x), KEY_NAN, QM.keys(x))


def unkey(k):
    """the samples of keys"""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63), k & np.uint64(0x7FFFFFFFFFFFFFFF), ~k).view(np.float64)


def rows(x, lo, w, levels, method=LINEAR, keys=None):
    """(len(lo), n_levels): the rows of the windows [lo[i], lo[i] + w) of the stream x (keys: stream_keys(x), kept by the
    caller across calls)"""
    lv = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    lo = np.asarray(lo, dtype=np.int64)
    out = np.empty((len(lo), len(lv)), dtype=np.float64)
    if len(lo) == 0:
        return out
    k = stream_keys(x) if keys is None else keys
    assert 1 <= w <= len(k) and int(lo.min()) >= 0 and int(lo.max()) + w <= len(k)
    view = sliding_window_view(k, w)
    step = max(1, BLOCK // w)
    for at in range(0, len(lo), step):
        srt = np.sort(view[lo[at:at + step]], axis=1)
        n = (srt != KEY_NAN).sum(axis=1)
        val = unkey(srt)
        for i in range(len(srt)):
            s = val[i, :n[i]]
            out[at + i] = [QM.level(s, q, method) for q in lv]
    return out


def literal(x, lo, w, levels, method=LINEAR):
    """the same rows, each window on its own: quantile_model.windows on the listed windows (lo[i], w)"""
    return QM.windows(np.asarray(x, dtype=np.float64), lo, [w] * len(lo), levels, method)


def rolling(x, begins, counts, w, s, levels, method=LINEAR, keys=None):
    """-> (rows, off) of a call over the ranges [begins[i], begins[i] + counts[i])"""
    return rows(x, positions(begins, counts, w, s), w, levels, method, keys), offsets(counts, w, s)
