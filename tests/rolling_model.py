"""NumPy restatement of the windowed rolling's contract (include/atsc_hip.h, DESIGN.md "Windowed rolling"), from the full
decode's samples: the terms, T level by level, a window's chunk walk and the left-to-right fold of its sum; count, min and
max by the aggregates' rules (tests/agg_model.py), the sign of a zero extreme included.

window_record() is the contract read literally, one window at a time.  Pyramid does the same for many windows at once
(the levels once per stream, the walk over all positions together); tests/test_rolling_host.py holds the two together."""
import math

import numpy as np

from tests import agg_model

MAX_WIDTH = 1 << 20
U = 2.0 ** -53


def outputs(count, width, stride):
    """positions of a range of `count` samples"""
    return (count - width) // stride + 1 if width and stride and count >= width else 0


def terms(x):
    """term(j): x[j], or -0.0 where x[j] is NaN"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), -0.0, x)


def chunks(lo, w):
    """the window's chunks (pos, l), left to right"""
    out, pos, hi = [], lo, lo + w
    while pos < hi:
        l = 0
        while pos % (2 << l) == 0 and pos + (2 << l) <= hi:
            l += 1
        out.append((pos, l))
        pos += 1 << l
    return out


def T(t, a, l):
    """T(a, l) over the terms t, a a multiple of 2^l: T(a, l - 1) + T(a + 2^(l-1), l - 1)"""
    assert a % (1 << l) == 0
    v = np.array(t[a:a + (1 << l)], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):  # +Inf + -Inf is NaN, as on the GPU
        while len(v) > 1:
            v = v[0::2] + v[1::2]
    return v[0]


def window_sum(x, lo, w):
    """the sum of x[lo:lo + w] in the documented order (+0.0 when no sample counts)"""
    v = np.asarray(x[lo:lo + w], dtype=np.float64)
    if np.isnan(v).all():
        return 0.0
    t = terms(x)
    s = None
    with np.errstate(invalid="ignore", over="ignore"):
        for pos, l in chunks(lo, w):
            c = T(t, pos, l)
            s = c if s is None else s + c
    return float(s)


def _tile_key(at):
    """the place of stream index `at` in the order in which the aggregates' tile kernel visits its tile of 2048 (the first
    of equal values stays): real lane in bit-reversed order (the wave's halving tree), then virtual lane 0, 2, 1, 3, the
    quarter and the slot of the pair"""
    s = at % 2048
    v = (s % 512) // 2
    lane, k = v % 64, v // 64
    rev = int("{:06b}".format(lane)[::-1], 2)
    return (rev, (0, 2, 1, 3)[k], s // 512, s % 2)


def zero_sign(x, lo, w):
    """the sign bit of the zero that atsc_aggregate_windows reports as an extreme of x[lo:lo + w]: of the window's first
    tile with a zero in it, the zero that the tile kernel visits first (tiles merge left to right, the left operand
    staying where values are equal)"""
    v = np.asarray(x[lo:lo + w], dtype=np.float64)
    at = lo + np.flatnonzero(v == 0.0)
    at = at[at // 2048 == at[0] // 2048]
    best = min(at, key=lambda a: _tile_key(int(a)))
    return bool(np.signbit(x[best]))


def _fix_zero(value, x, lo, w):
    return (-0.0 if zero_sign(x, lo, w) else 0.0) if value == 0.0 else value


def window_record(x, lo, w):
    """-> (count, min, max, sum) of the position whose window is x[lo:lo + w]"""
    n, mn, mx, _, _, _ = agg_model.window_stats(x, lo, w)
    if n:
        mn, mx = _fix_zero(mn, x, lo, w), _fix_zero(mx, x, lo, w)
    return n, mn, mx, window_sum(x, lo, w)


def error_bound(v):
    """3 L 2^-53 sum|x| over the non-NaN samples of the window v, L = max(1, ceil(log2 w))"""
    v = np.asarray(v, dtype=np.float64)
    L = max(1, math.ceil(math.log2(len(v)))) if len(v) else 1
    return 3 * L * U * float(math.fsum(np.abs(v[~np.isnan(v)])))


RECORD = np.dtype([("count", "<u8"), ("min", "<f8"), ("max", "<f8"), ("sum", "<f8")])


class Pyramid:
    """the chunk partials of a stream, level by level, and the records of many windows read off them"""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=np.float64)
        nan = np.isnan(self.x)
        self.sum = [terms(self.x)]
        self.mn = [np.where(nan, np.inf, self.x)]
        self.mx = [np.where(nan, -np.inf, self.x)]
        self.cnt = [(~nan).astype(np.uint64)]
        zero = self.x == 0.0
        self.neg = [(zero & np.signbit(self.x)).astype(np.uint64)]
        self.pos = [(zero & ~np.signbit(self.x)).astype(np.uint64)]

    def _level(self, l):
        with np.errstate(invalid="ignore", over="ignore"):
            while len(self.sum) <= l:
                n = len(self.sum[-1]) // 2 * 2
                self.sum.append(self.sum[-1][0:n:2] + self.sum[-1][1:n:2])
                self.mn.append(np.minimum(self.mn[-1][0:n:2], self.mn[-1][1:n:2]))
                self.mx.append(np.maximum(self.mx[-1][0:n:2], self.mx[-1][1:n:2]))
                for a in (self.cnt, self.neg, self.pos):
                    a.append(a[-1][0:n:2] + a[-1][1:n:2])

    def records(self, lo, w):
        """-> RECORD array: the windows x[lo[i]:lo[i] + w]"""
        lo = np.asarray(lo, dtype=np.int64)
        out = np.zeros(len(lo), dtype=RECORD)
        if len(lo) == 0:
            return out
        assert w >= 1 and lo.min() >= 0 and lo.max() + w <= len(self.x)
        self._level(max(int(math.floor(math.log2(w))), 0))
        pos, hi = lo.copy(), lo + w
        s = np.full(len(lo), -0.0)  # (-0.0 + t is t, bit for bit)
        mn, mx = np.full(len(lo), np.inf), np.full(len(lo), -np.inf)
        cnt, neg, plus = (np.zeros(len(lo), dtype=np.uint64) for _ in range(3))
        with np.errstate(invalid="ignore", over="ignore"):
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
                    s[at] = s[at] + self.sum[l][j]
                    mn[at] = np.minimum(mn[at], self.mn[l][j])
                    mx[at] = np.maximum(mx[at], self.mx[l][j])
                    cnt[at] += self.cnt[l][j]
                    neg[at] += self.neg[l][j]
                    plus[at] += self.pos[l][j]
                    pos[at] += 1 << l
        some = cnt > 0
        out["count"] = cnt
        out["sum"] = np.where(some, s, 0.0)
        for name, v in (("min", mn), ("max", mx)):
            v = np.where(some, v, np.nan)
            z = some & (v == 0.0)
            v[z & (neg > 0) & (plus == 0)] = -0.0
            v[z & (neg == 0)] = 0.0
            for i in np.flatnonzero(z & (neg > 0) & (plus > 0)):
                v[i] = -0.0 if zero_sign(self.x, int(lo[i]), w) else 0.0
            out[name] = v
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
