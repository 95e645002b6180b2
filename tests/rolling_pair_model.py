"""NumPy restatement of the windowed rolling pair moments' contract (include/atsc_hip.h, DESIGN.md "Windowed rolling pair
moments"), from the two full decodes' samples: the windowed pair moments' node, leaf and Merge (tests/pair_model.py; the
merge is tests/moments_model.py's, with y where that has the position) over the rolling's aligned chunks and chunk walk
(tests/rolling_model.py, chunks), the chain merged left to right.  It is tests/rolling_moments_model.py with the pair's
leaf, and no field of the record is counted from the window's begin.

window_record() is the contract read literally, one window at a time.  Pyramid does the same for many windows at once
(the levels once per pair of streams, the walk over all positions together); tests/test_rolling_pair_host.py holds the
two together.  org: the stream index of x[0] and y[0] (the chunks' alignment counts in the stream's index)."""
import math

import numpy as np

from tests import moments_model as MM
from tests import pair_model as PM
from tests import rolling_model as R
from tests import rolling_moments_model as RM

U = R.U
FIELDS = PM.FIELDS
RECORD = PM.DTYPE
outputs = R.outputs
chunks = R.chunks
listed = RM.listed
depth = RM.depth


def leaves(x, y):
    """the leaf nodes of the samples x and y of the same stream indices: (1, x[j], 0, y[j], 0, 0), the empty node where
    x[j] or y[j] is NaN"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert len(x) == len(y)
    ok = ~(np.isnan(x) | np.isnan(y))
    z = np.zeros(len(x))
    return ok.astype(np.uint64), np.where(ok, x, 0.0), z, np.where(ok, y, 0.0), z.copy(), z.copy()


_halve = RM._halve


def N(x, y, org, a, l):
    """N(a, l) of the streams whose samples org + j are x[j] and y[j], a a multiple of 2^l in the stream index -> a node
    of one-element arrays"""
    assert a % (1 << l) == 0 and a >= org
    q = leaves(x[a - org:a - org + (1 << l)], y[a - org:a - org + (1 << l)])
    assert len(q[0]) == 1 << l
    while len(q[0]) > 1:
        q = _halve(q)
    return q


def _record(n, mx, m2x, my, m2y, c):
    """the record of the nodes (arrays)"""
    some = n > 0
    out = np.zeros(len(n), dtype=RECORD)
    out["count"] = n
    for k, v in zip(FIELDS[1:], (mx, m2x, my, m2y, c)):
        out[k] = np.where(some, v, np.nan)
    return out


def window_record(x, y, lo, w, org=0):
    """-> (count, mean_x, m2_x, mean_y, m2_y, c_xy) of the position whose window is x[lo:lo + w] and y[lo:lo + w], the
    samples org + lo .. of the streams"""
    acc = None
    for pos, l in chunks(org + lo, w):
        c = N(x, y, org, pos, l)
        acc = c if acc is None else MM.merge(acc, c)  # (Merge(empty, c) is c)
    r = _record(*acc)[0]
    return (int(r["count"]),) + tuple(float(r[k]) for k in FIELDS[1:])


def bounds(w, n, mean_x, m2_x, mean_y, m2_y):
    """the documented bounds (b_mean / mean|.|, b_m2_x, b_m2_y, b_c_xy) from the exact values of a window of w slots with
    n counted samples: (3 L + 2) u times (1, kappa_x m2_x, kappa_y m2_y, kappa_x kappa_y sqrt(m2_x m2_y)), L = max(1,
    ceil(log2 w)) -- tests/pair_model.py's bounds with 3 L + 2 for L + 2.  kappa^2 m2 = m2 + n mean^2 keeps the products
    finite where m2 == 0."""
    k = (3 * depth(w) + 2) * U
    ax = float(m2_x) + n * float(mean_x) ** 2
    ay = float(m2_y) + n * float(mean_y) ** 2
    return k, k * math.sqrt(float(m2_x) * ax), k * math.sqrt(float(m2_y) * ay), k * math.sqrt(ax * ay)


class Pyramid:
    """the chunk nodes of a pair of streams, level by level, and the records of many windows read off them"""

    def __init__(self, x, y, org=0):
        assert org % R.MAX_WIDTH == 0  # (so that x's own index is aligned as the stream's is)
        n = min(len(x), len(y))  # a window lies inside both streams
        self.x = np.asarray(x, dtype=np.float64)[:n]
        self.y = np.asarray(y, dtype=np.float64)[:n]
        self.org = org
        self.levels = [leaves(self.x, self.y)]

    def _level(self, l):
        while len(self.levels) <= l:
            self.levels.append(_halve(self.levels[-1]))

    def records(self, lo, w):
        """-> RECORD array: the windows x[lo[i]:lo[i] + w], y[lo[i]:lo[i] + w]"""
        lo = np.asarray(lo, dtype=np.int64)
        if len(lo) == 0:
            return np.zeros(0, dtype=RECORD)
        assert w >= 1 and lo.min() >= 0 and lo.max() + w <= len(self.x)
        self._level(max(int(math.floor(math.log2(w))), 0))
        pos, hi = lo.copy(), lo + w
        acc = [np.zeros(len(lo), dtype=np.uint64)] + [np.zeros(len(lo)) for _ in range(5)]
        while True:
            live = np.flatnonzero(pos < hi)
            if len(live) == 0:
                break
            p, room = pos[live], hi[live] - pos[live]
            up = np.where(p == 0, 62, np.log2(np.maximum(p & -p, 1).astype(np.float64)).astype(np.int64))
            fit = np.floor(np.log2(room.astype(np.float64))).astype(np.int64)
            lv = np.minimum(up, fit)
            for l in np.unique(lv):
                at = live[lv == l]
                j = pos[at] >> l
                m = MM.merge(tuple(f[at] for f in acc), tuple(f[j] for f in self.levels[l]))
                for f, v in zip(acc, m):
                    f[at] = v
                pos[at] += 1 << l
        return _record(*acc)

    def rolling(self, begins, counts, w, s):
        """-> (RECORD array, offsets): the records of the ranges, range after range, as the library stores them"""
        lo, off = [], [0]
        for b, c in zip(begins, counts):
            m = outputs(int(c), w, s)
            lo.append(int(b) + s * np.arange(m, dtype=np.int64))
            off.append(off[-1] + m)
        lo = np.concatenate(lo) if lo else np.zeros(0, dtype=np.int64)
        return self.records(lo, w), np.array(off, dtype=np.uint64)
