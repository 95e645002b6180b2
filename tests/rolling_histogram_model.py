"""NumPy restatement of the windowed rolling histograms' contract (include/atsc_hip.h, DESIGN.md "Windowed rolling
histograms"), from the full decode's samples: the row of the position whose window is [lo, lo + w) is the windowed
histograms' row of the listed window (lo, w) -- n_edges + 2 u64 counters, bins 0 .. n_edges by tests/hist_model.py's
bins(), then the window's NaN samples.

rows() bins the stream once (numpy.searchsorted, the side by `closed`, NaN to the last counter), takes the prefix sums
of the one-hot bins and reads a window's counters as the difference of the sums at lo + w and at lo; literal() is the
contract read literally, hist_model.windows on the listed windows.  tests/test_rolling_histogram_host.py holds the two
together.  task_positions() states the rule that sizes a task (rh_task_positions in atsc_internal.h)."""
import numpy as np

from tests import hist_model as HM
from tests import rolling_model as R

LEFT_CLOSED, RIGHT_CLOSED = HM.LEFT_CLOSED, HM.RIGHT_CLOSED
MAX_EDGES = HM.MAX_EDGES
MAX_WIDTH = 1 << 20
TASK_MIN, TASK_MAX = 64, 2048
outputs = R.outputs


def task_positions(w, s):
    """B: the positions one task holds -- eight windows' worth of positions, at least 64 and at most 2048"""
    return min(max(8 * -(-w // s), TASK_MIN), TASK_MAX)


def offsets(counts, w, s):
    """the ranges' row offsets: range i's rows are [off[i], off[i + 1])"""
    return np.concatenate([[0], np.cumsum([outputs(int(c), w, s) for c in counts])]).astype(np.uint64)


def positions(begins, counts, w, s):
    """the first sample of every position's window, range after range"""
    lo = [int(b) + s * np.arange(outputs(int(c), w, s), dtype=np.int64) for b, c in zip(begins, counts)]
    return np.concatenate(lo) if lo else np.zeros(0, dtype=np.int64)


def stream_bins(x, edges, closed=LEFT_CLOSED):
    """the counter every sample of the stream adds to (kept by the caller across calls with the same edges and side)"""
    return HM.bins(x, edges, closed)


def rows(x, lo, w, edges, closed=LEFT_CLOSED, bins=None):
    """(len(lo), n_edges + 2) uint64: the rows of the windows [lo[i], lo[i] + w) of the stream x (bins:
    stream_bins(x, edges, closed)).  Prefix sums of the one-hot bins over the stretch the windows cover, a bin at a time."""
    n_rows = len(edges) + 2
    lo = np.asarray(lo, dtype=np.int64)
    out = np.zeros((len(lo), n_rows), dtype=np.uint64)
    if len(lo) == 0:
        return out
    k = stream_bins(x, edges, closed) if bins is None else bins
    a, z = int(lo.min()), int(lo.max()) + w
    assert 1 <= w and a >= 0 and z <= len(k)
    k = k[a:z]
    for b in np.unique(k):
        cs = np.concatenate([[0], np.cumsum(k == b)]).astype(np.uint64)
        out[:, b] = cs[lo - a + w] - cs[lo - a]
    return out


def literal(x, lo, w, edges, closed=LEFT_CLOSED):
    """the same rows, each window on its own: hist_model.windows on the listed windows (lo[i], w), no prefix sums"""
    return HM.windows(np.asarray(x, dtype=np.float64), lo, [w] * len(lo), edges, closed, prefix=False)


def rolling(x, begins, counts, w, s, edges, closed=LEFT_CLOSED, bins=None):
    """-> (rows, off) of a call over the ranges [begins[i], begins[i] + counts[i])"""
    return rows(x, positions(begins, counts, w, s), w, edges, closed, bins), offsets(counts, w, s)
