"""NumPy model of the windowed across histograms (include/atsc_hip.h, DESIGN.md "Windowed across histograms") over already
decoded arrays: at every position of the across' ranges, how many of the N streams hold a sample in each value bin.  The
bin of a sample that is not NaN is numpy.searchsorted(edges, v, side="right") under LEFT_CLOSED and side="left" under
RIGHT_CLOSED (the windowed histograms' rule, tests/histogram_model.py); NaN samples go to the last counter.  Positions and
offsets are tests/across_model.py's."""
import numpy as np

from tests import across_model as AM

LEFT_CLOSED, RIGHT_CLOSED = 0, 1
MAX_EDGES = 1024


def rows(columns, edges, closed=LEFT_CLOSED):
    """columns: an (N, M) array, stream k's samples at the M positions -> (M, n_edges + 2) uint64 rows"""
    x = np.asarray(columns, dtype=np.float64)
    assert x.ndim == 2 and 1 <= x.shape[0] <= AM.MAX_STREAMS
    edges = np.asarray(edges, dtype=np.float64)
    assert 1 <= len(edges) <= MAX_EDGES and closed in (LEFT_CLOSED, RIGHT_CLOSED)
    n, m = x.shape
    out = np.zeros((m, len(edges) + 2), dtype=np.uint64)
    nan = np.isnan(x)
    bins = np.full(x.shape, len(edges) + 1, dtype=np.int64)
    bins[~nan] = np.searchsorted(edges, x[~nan], side="left" if closed == RIGHT_CLOSED else "right")
    np.add.at(out, (np.broadcast_to(np.arange(m), (n, m)), bins), 1)
    return out


def across_histogram(fulls, begins, counts, edges, stride=1, closed=LEFT_CLOSED):
    """fulls: the full decode of every stream, in list order -> (rows, off) of an across histogram call over the ranges"""
    off = AM.offsets(counts, stride)
    parts = []
    for b, c in zip(begins, counts):
        idx = int(b) + int(stride) * np.arange(AM.outputs(c, stride), dtype=np.int64)
        assert len(idx) == 0 or all(idx[-1] < len(f) for f in fulls)
        parts.append(rows(np.array([np.asarray(f, dtype=np.float64)[idx] for f in fulls]).reshape(len(fulls), len(idx)), edges, closed))
    return (np.concatenate(parts) if parts else np.zeros((0, len(edges) + 2), dtype=np.uint64)), off


# the kernel's passes (atsc_across_histogram.hip): a row's pitch in bytes and the rows a wavefront counts at a time
WAVE_LDS = 14336


def row_pitch(n_edges):
    return 4 * (((n_edges + 2 + 3) // 4) | 1)


def rows_a_pass(n_edges):
    return min(64, WAVE_LDS // row_pitch(n_edges))


def pass_boundaries():
    """every n_edges at which rows_a_pass differs from its value at n_edges - 1, with the n_edges in front of it"""
    out = []
    for e in range(2, MAX_EDGES + 1):
        if rows_a_pass(e) != rows_a_pass(e - 1):
            out += [e - 1, e]
    return sorted(set(out))
