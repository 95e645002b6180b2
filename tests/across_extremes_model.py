"""NumPy model of the windowed across extremes' contract (include/atsc_hip.h, DESIGN.md "Windowed across extremes"):
the record of a position is the windowed extremes' record of the column x_0 .. x_(N-1) of the N streams' samples there,
`at` being the stream's place in the list -- extremes_model.window_extremes(column, 0, N, k), which `column_record`
is.  `records` is the same thing for whole arrays at a time (a stable argsort along the stream axis: NumPy compares
-0.0 and +0.0 as equal and puts NaN last); tests/test_across_extremes_host.py holds it to the definition column by
column.  Ranges and record numbering are the across' (tests/across_model.py)."""
import numpy as np

from tests import across_model
from tests import extremes_model as E

NONE = E.NONE
MAX_K = E.MAX_K
dtype = E.dtype
words = E.words


def column_record(column, k):
    """the definition: the windowed extremes' record of the column as a window of N samples"""
    column = np.asarray(column, dtype=np.float64)
    return E.window_extremes(column, 0, len(column), k)


def records(x, k):
    """x: (N, P) samples, a column per position.  -> P records of dtype(k)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n_streams, p = x.shape
    out = np.zeros(p, dtype=dtype(k))
    nan = np.isnan(x)
    out["count"] = n_streams
    out["nans"] = nan.sum(axis=0)
    some = n_streams - nan.sum(axis=0)  # entries in use per position, before the cut at k
    for name, w in (("largest", -x), ("smallest", x)):
        out[name]["value"] = np.nan
        out[name]["at"] = NONE
        order = np.argsort(w, axis=0, kind="stable")[:k]  # (j, P): the stream of rank j; NaN behind the others
        j = len(order)
        used = (np.arange(j)[:, None] < some[None, :]).T  # (P, j)
        value = np.take_along_axis(x, order, axis=0).T
        out[name]["value"][:, :j] = np.where(used, value, np.nan)
        out[name]["at"][:, :j] = np.where(used, order.T.astype(np.uint64), np.uint64(NONE))
    return out


def positions(begins, counts, stride=1):
    """-> the sample index of every position of the ranges, range after range"""
    idx = [int(b) + int(stride) * np.arange(across_model.outputs(c, stride), dtype=np.int64) for b, c in zip(begins, counts)]
    return np.concatenate(idx) if idx else np.empty(0, dtype=np.int64)


def columns(fulls, begins, counts, stride=1):
    """-> (N, P): the decoded streams' samples at the positions of the ranges"""
    idx = positions(begins, counts, stride)
    return np.stack([np.asarray(f, dtype=np.float64)[idx] for f in fulls])


def across_extremes(fulls, begins, counts, k, stride=1):
    """-> (records, off) of the call over the decoded streams `fulls` (sample j of one goes with sample j of every
    other)"""
    return records(columns(fulls, begins, counts, stride), k), across_model.offsets(counts, stride)


def same(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return len(a) == 0 or bool(np.array_equal(words(a), words(b)))
