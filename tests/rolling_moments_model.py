"""NumPy restatement of the windowed rolling moments' contract (include/atsc_hip.h, DESIGN.md "Windowed rolling
moments"), from the full decode's samples: the windowed moments' node, leaf and Merge (tests/moments_model.py, merge) over
the rolling's aligned chunks and chunk walk (tests/rolling_model.py, chunks), the chain merged left to right.

window_record() is the contract read literally, one window at a time.  Pyramid does the same for many windows at once
(the levels once per stream, the walk over all positions together); tests/test_rolling_moments_host.py holds the two
together.  org: the stream index of x[0] (the leaves' positions and the chunks' alignment count in the stream's index)."""
import math

import numpy as np

from tests import moments_model as MM
from tests import rolling_model as R

U = R.U
FIELDS = MM.FIELDS
RECORD = np.dtype([("count", "<u8")] + [(k, "<f8") for k in FIELDS[1:]])
outputs = R.outputs
chunks = R.chunks


def leaves(x, org=0):
    """the leaf nodes of the samples x, x[j] at stream index org + j: (1, x[j], 0, (double)(org + j), 0, 0), a NaN slot
    the empty node"""
    x = np.asarray(x, dtype=np.float64)
    ok = ~np.isnan(x)
    z = np.zeros(len(x))
    t = (np.arange(len(x), dtype=np.uint64) + np.uint64(org)).astype(np.float64)
    return ok.astype(np.uint64), np.where(ok, x, 0.0), z, np.where(ok, t, 0.0), z.copy(), z.copy()


def _halve(q):
    """one level up: Merge(q[2 i], q[2 i + 1])"""
    n = len(q[0]) // 2 * 2
    return MM.merge(tuple(f[0:n:2] for f in q), tuple(f[1:n:2] for f in q))


def N(x, org, a, l):
    """N(a, l) of the stream whose sample org + j is x[j], a a multiple of 2^l in the stream index -> a node of
    one-element arrays"""
    assert a % (1 << l) == 0 and a >= org
    q = leaves(x[a - org:a - org + (1 << l)], a)
    assert len(q[0]) == 1 << l
    while len(q[0]) > 1:
        q = _halve(q)
    return q


def _record(n, mx, m2x, mt, m2t, c, lo):
    """the record of the node whose window begins at stream index lo (arrays)"""
    some = n > 0
    with np.errstate(all="ignore"):
        t_mean = mt - lo.astype(np.float64)
    out = np.zeros(len(n), dtype=RECORD)
    out["count"] = n
    for k, v in zip(FIELDS[1:], (mx, m2x, t_mean, m2t, c)):
        out[k] = np.where(some, v, np.nan)
    return out


def window_record(x, lo, w, org=0):
    """-> (count, mean, m2, t_mean, t_m2, c_tx) of the position whose window is x[lo:lo + w], the samples org + lo ..
    of the stream"""
    acc = None
    for pos, l in chunks(org + lo, w):
        c = N(x, org, pos, l)
        acc = c if acc is None else MM.merge(acc, c)  # (Merge(empty, c) is c)
    r = _record(*acc, np.array([org + lo], dtype=np.uint64))[0]
    return (int(r["count"]),) + tuple(float(r[k]) for k in FIELDS[1:])


def listed(begins, counts, w, s):
    """-> [(lo, w)]: the windows of a call's positions, range after range"""
    return [(int(b) + j * s, w) for b, c in zip(begins, counts) for j in range(outputs(int(c), w, s))]


def depth(w):
    """L = max(1, ceil(log2 w))"""
    return max(1, math.ceil(math.log2(w))) if w > 1 else 1


def bounds(w, n, mean, m2, t_m2):
    """the documented bounds (b_mean / mean|x|, b_m2, b_t_m2 / r, b_c_tx / r) from the exact values of a window of w
    slots with n samples: (3 L + 2) u times (1, kappa m2, t_m2, kappa sqrt(t_m2 m2)) -- tests/moments_model.py's bounds
    with 3 L for L"""
    k = (3 * depth(w) + 2) * U
    m2f, tf = float(m2), float(t_m2)
    spread = m2f + n * float(mean) ** 2
    return k, k * math.sqrt(m2f * spread), k * tf, k * math.sqrt(tf * spread)


class Pyramid:
    """the chunk nodes of a stream, level by level, and the records of many windows read off them"""

    def __init__(self, x, org=0):
        assert org % R.MAX_WIDTH == 0  # (so that x's own index is aligned as the stream's is)
        self.x = np.asarray(x, dtype=np.float64)
        self.org = org
        self.levels = [leaves(self.x, org)]

    def _level(self, l):
        while len(self.levels) <= l:
            self.levels.append(_halve(self.levels[-1]))

    def records(self, lo, w):
        """-> RECORD array: the windows x[lo[i]:lo[i] + w]"""
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
        return _record(*acc, lo.astype(np.uint64) + np.uint64(self.org))

    def rolling(self, begins, counts, w, s):
        """-> (RECORD array, offsets): the records of the ranges, range after range, as the library stores them"""
        lo, off = [], [0]
        for b, c in zip(begins, counts):
            m = outputs(int(c), w, s)
            lo.append(int(b) + s * np.arange(m, dtype=np.int64))
            off.append(off[-1] + m)
        lo = np.concatenate(lo) if lo else np.zeros(0, dtype=np.int64)
        return self.records(lo, w), np.array(off, dtype=np.uint64)
