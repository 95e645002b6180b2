"""NumPy restatement of the windowed pair matrix' contract (include/atsc_hip.h, DESIGN.md "Windowed pair matrix"): record
(i, j), i <= j, of a window is the windowed pair moments' record (tests/pair_model.py) of stream i as x and stream j as y
over that window; a window's records lie in the order of the index formula."""
import numpy as np

from tests import pair_model as P

TILE = P.TILE
FIELDS = P.FIELDS
DTYPE = P.DTYPE


def records(n):
    """P: the records per window of n streams"""
    return n * (n + 1) // 2


def index(n, i, j):
    """p of pair (i, j), i <= j < n; None where there is no such pair"""
    if i > j or j >= n:
        return None
    return i * (2 * n - i + 1) // 2 + (j - i)


def pairs(n):
    """the pairs (i, j) in the records' order"""
    return [(i, j) for i in range(n) for j in range(i, n)]


def windows_pair_matrix(streams, wins, only=None):
    """-> (W, P) structured array of the windows (begin, count) of the list of sample arrays; only: the pairs to compute
    (the others' records stay zero)"""
    n = len(streams)
    out = np.zeros((len(wins), records(n)), dtype=DTYPE)
    for (i, j) in (pairs(n) if only is None else only):
        out[:, index(n, i, j)] = P.windows_pair(streams[i], streams[j], wins)
    return out
