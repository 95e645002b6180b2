"""NumPy restatement of the windowed rolling deltas' contract (include/atsc_hip.h, DESIGN.md "Windowed rolling deltas"),
from the full decode's samples: the deltas' pairs and terms (tests/delta_model.py) at the slot of the pair's second sample,
T level by level over those slots, and the chunk walk and left-to-right fold of the rolling (tests/rolling_model.py) over
the window's pair slots [lo + 1, lo + w).

window_record() is the contract read literally, one window at a time.  Pyramid does the same for many windows at once
(the levels once per stream, the walk over all positions together); tests/test_rolling_delta_host.py holds the two
together."""
import math

import numpy as np

from tests import delta_model as D
from tests import rolling_model as R

U = R.U
FIELDS = D.FIELDS
RECORD = D.DTYPE
outputs = R.outputs


def chunks(lo, w):
    """the chunks (pos, l) of the window's pair slots [lo + 1, lo + w), left to right"""
    return R.chunks(lo + 1, w - 1)


def slot_terms(x):
    """-> (up, down, after_falls, counted, rise, fall) per slot of the stream x: slot j holds the pair (x[j - 1], x[j]);
    slot 0 and the slots without a term hold -0.0"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    up, down, after = (np.full(n, -0.0) for _ in range(3))
    counted, rise, fall = (np.zeros(n, dtype=bool) for _ in range(3))
    if n > 1:
        a, b = x[:-1], x[1:]
        ok = ~np.isnan(a) & ~np.isnan(b)
        with np.errstate(invalid="ignore", over="ignore"):
            r, f = b - a, a - b  # one rounded subtract each
            rs, fl = ok & (b > a), ok & (b < a)
        counted[1:], rise[1:], fall[1:] = ok, rs, fl
        up[1:] = np.where(rs, r, -0.0)
        down[1:] = np.where(fl, f, -0.0)
        after[1:] = np.where(fl, b, -0.0)
    return up, down, after, counted, rise, fall


def _fold(t, lo, w):
    s = None
    with np.errstate(invalid="ignore", over="ignore"):
        for pos, l in chunks(lo, w):
            c = R.T(t, pos, l)
            s = c if s is None else s + c
    return float(s)


def window_record(x, lo, w):
    """-> (pairs, rises, falls, up, down, after_falls, max_rise, max_fall) of the position whose window is x[lo:lo + w]"""
    if w <= 1:
        return 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0
    up, down, after, counted, rise, fall = slot_terms(x)
    sl = slice(lo + 1, lo + w)
    n_r, n_f = int(rise[sl].sum()), int(fall[sl].sum())
    return (int(counted[sl].sum()), n_r, n_f, _fold(up, lo, w) if n_r else 0.0, _fold(down, lo, w) if n_f else 0.0,
            _fold(after, lo, w) if n_f else 0.0, float(np.max(up[sl][rise[sl]])) if n_r else 0.0,
            float(np.max(down[sl][fall[sl]])) if n_f else 0.0)


def listed(begins, counts, w, s):
    """-> [(lo, w)]: the windows of a call's positions, range after range"""
    return [(int(b) + j * s, w) for b, c in zip(begins, counts) for j in range(outputs(int(c), w, s))]


def bound_factor(w):
    """(3 L + 1) u with L = max(1, ceil(log2 w)): one rounding for the subtract, then the rolling's 3 L"""
    L = max(1, math.ceil(math.log2(w))) if w > 1 else 1
    return (3 * L + 1) * U


class Pyramid:
    """the chunk partials of a stream's pair slots, level by level, and the records of many windows read off them"""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float64)
        up, down, after, counted, rise, fall = slot_terms(self.x)
        self.sums = [[up], [down], [after]]
        # the maxima's leaves: the term of a rise or fall (> 0), else +0.0
        self.maxs = [[np.where(rise, up, 0.0)], [np.where(fall, down, 0.0)]]
        self.cnts = [[counted.astype(np.uint64)], [rise.astype(np.uint64)], [fall.astype(np.uint64)]]

    def _level(self, l):
        with np.errstate(invalid="ignore", over="ignore"):
            while len(self.sums[0]) <= l:
                n = len(self.sums[0][-1]) // 2 * 2
                for a in self.sums + self.cnts:
                    a.append(a[-1][0:n:2] + a[-1][1:n:2])
                for a in self.maxs:
                    a.append(np.maximum(a[-1][0:n:2], a[-1][1:n:2]))

    def records(self, lo, w):
        """-> RECORD array: the windows x[lo[i]:lo[i] + w]"""
        lo = np.asarray(lo, dtype=np.int64)
        out = np.zeros(len(lo), dtype=RECORD)
        if len(lo) == 0 or w <= 1:
            return out
        assert lo.min() >= 0 and lo.max() + w <= len(self.x)
        self._level(int(math.floor(math.log2(w - 1))))
        pos, hi = lo + 1, lo + w
        s = [np.full(len(lo), -0.0) for _ in range(3)]  # (-0.0 + t is t, bit for bit)
        m = [np.zeros(len(lo)) for _ in range(2)]
        c = [np.zeros(len(lo), dtype=np.uint64) for _ in range(3)]
        with np.errstate(invalid="ignore", over="ignore"):
            while True:
                live = np.flatnonzero(pos < hi)
                if len(live) == 0:
                    break
                p, room = pos[live], hi[live] - pos[live]
                up = np.log2((p & -p).astype(np.float64)).astype(np.int64)
                fit = np.floor(np.log2(room.astype(np.float64))).astype(np.int64)
                lv = np.minimum(up, fit)
                for l in np.unique(lv):
                    at = live[lv == l]
                    j = pos[at] >> l
                    for k in range(3):
                        s[k][at] = s[k][at] + self.sums[k][l][j]
                        c[k][at] += self.cnts[k][l][j]
                    for k in range(2):
                        m[k][at] = np.maximum(m[k][at], self.maxs[k][l][j])
                    pos[at] += 1 << l
        out["pairs"], out["rises"], out["falls"] = c
        out["up"] = np.where(c[1] > 0, s[0], 0.0)
        out["down"] = np.where(c[2] > 0, s[1], 0.0)
        out["after_falls"] = np.where(c[2] > 0, s[2], 0.0)
        out["max_rise"], out["max_fall"] = m
        return out

    def rolling(self, begins, counts, w, s):
        """-> (RECORD array, offsets): the records of the ranges, range after range, as the library stores them"""
        lo, off = [], [0]
        for b, c in zip(begins, counts):
            m = outputs(int(c), w, s)
            lo.append(int(b) + s * np.arange(m, dtype=np.int64))
            off.append(off[-1] + m)
        lo = np.concatenate(lo) if lo else np.zeros(0, dtype=np.int64)
        return self.records(lo, w), np.array(off, dtype=np.uint64)
