"""NumPy model of the windowed histograms' contract (include/atsc_hip.h, atsc_histogram_windows): a row of
n_edges + 2 u64 counters per window -- bins 0 .. n_edges, then the number of NaN samples.  A non-NaN sample v goes to
bin numpy.searchsorted(edges, v, side="right") when the bins are left closed (the number of edges <= v) and
side="left" when they are right closed (the number of edges < v); samples and edges are compared as values."""
import numpy as np

LEFT_CLOSED, RIGHT_CLOSED = 0, 1
MAX_EDGES = 1024
SIDE = {LEFT_CLOSED: "right", RIGHT_CLOSED: "left"}


def bins(x, edges, closed=LEFT_CLOSED):
    """the counter every sample of x adds to: its bin, or n_edges + 1 for NaN"""
    x = np.asarray(x, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    nan = np.isnan(x)
    k = np.searchsorted(edges, np.where(nan, 0.0, x), side=SIDE[closed])
    return np.where(nan, len(edges) + 1, k).astype(np.int64)


def row(x, edges, closed=LEFT_CLOSED):
    """the counters of one window's samples x"""
    return np.bincount(bins(x, edges, closed), minlength=len(edges) + 2).astype(np.uint64)


def windows(full, begins, counts, edges, closed=LEFT_CLOSED, prefix=None):
    """-> (n_windows, n_edges + 2) uint64: row() of full[begins[i] : begins[i] + counts[i]].  The samples are binned
    once; a window's counters come from its stretch of the bins, or (prefix; the default above 4096 windows) from
    prefix sums per bin."""
    rows = len(edges) + 2
    bb = np.asarray(begins, dtype=np.int64).reshape(-1)
    cc = np.asarray(counts, dtype=np.int64).reshape(-1)
    out = np.zeros((len(bb), rows), dtype=np.uint64)
    live = np.flatnonzero(cc > 0)
    if not len(live):
        return out
    lo, hi = int(bb[live].min()), int((bb[live] + cc[live]).max())
    k = bins(np.asarray(full, dtype=np.float64)[lo:hi], edges, closed)
    if len(bb) > 4096 if prefix is None else prefix:
        for b in np.unique(k):
            cs = np.concatenate([[0], np.cumsum(k == b)]).astype(np.uint64)
            out[live, b] = cs[bb[live] - lo + cc[live]] - cs[bb[live] - lo]
        return out
    for i in live:
        out[i] = np.bincount(k[bb[i] - lo: bb[i] - lo + cc[i]], minlength=rows)
    return out
