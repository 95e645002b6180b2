"""NumPy model of the windowed across value counts (include/atsc_hip.h, DESIGN.md "Windowed across value counts"): at
every position of ranges of the decoded streams, the windowed value counts' record (tests/values_model.py) of the column
of the N streams' samples there, as if the column were a window of N samples -- count = N, nans, below, and the k
smallest distinct values above `above` with the number of streams that hold each.  Offsets and positions are the
across' (tests/across_model.py).  No arithmetic touches a sample, so every field is the contract's bit for bit."""
import math

import numpy as np

from tests import across_model as AM
from tests import values_model as VM

MAX_K = VM.MAX_K
MAX_STREAMS = AM.MAX_STREAMS
dtype = VM.dtype
words = VM.words


def records(columns, k, above=math.nan):
    """columns: (N, M), stream j's samples at the M positions -> M records of dtype(k): a column is a window"""
    x = np.asarray(columns, dtype=np.float64)
    assert x.ndim == 2 and 1 <= x.shape[0] <= MAX_STREAMS
    out = np.zeros(x.shape[1], dtype=dtype(k))
    for p in range(x.shape[1]):
        out[p] = VM.window_values(np.ascontiguousarray(x[:, p]), 0, x.shape[0], k, above)
    return out


def across_values(fulls, begins, counts, k, stride=1, above=math.nan):
    """fulls: the full decode of every stream, in list order -> (records, off) of an across value-count call over the
    ranges"""
    off = AM.offsets(counts, stride)
    parts = []
    for b, c in zip(begins, counts):
        idx = int(b) + int(stride) * np.arange(AM.outputs(c, stride), dtype=np.int64)
        assert len(idx) == 0 or all(idx[-1] < len(f) for f in fulls)
        parts.append(records(np.array([np.asarray(f)[idx] for f in fulls]).reshape(len(fulls), len(idx)), k, above))
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=dtype(k))), off


def pages(column, k):
    """the records of one column paged with above = the last listed value until nothing is left: ceil(D / k) of them (one
    where D == 0)"""
    col = np.asarray(column, dtype=np.float64).reshape(-1, 1)
    out, above = [], math.nan
    while True:
        r = records(col, k, above)[0]
        out.append(r)
        if not int(r["more"]):
            return out
        above = float(r["entry"]["value"][int(r["distinct"]) - 1])
