"""NumPy restatement of the windowed runs' contract (include/atsc_hip.h, DESIGN.md "Windowed runs"): the samples of a
window that meet the condition, their maximal runs read off the inside mask by differences (not by the merge rule), and
`excess` in the aggregate sum's tree (tests/agg_model.py), from the full decode's samples; the merge rule of
atsc_runs_merge; the exact excess in rational arithmetic and the documented error bound."""
import math
from fractions import Fraction

import numpy as np

from tests import agg_model as G

TILE = G.TILE
U = 2.0 ** -53
NONE = 2 ** 64 - 1
GT, GE, LT, LE, EQ, NE = range(6)
OPS = (GT, GE, LT, LE, EQ, NE)

FIELDS = ("samples", "inside", "runs", "longest", "longest_at", "first_at", "last_at", "head", "tail", "excess")
DTYPE = np.dtype([(k, "<u8") for k in FIELDS[:9]] + [("excess", "<f8")])
EMPTY = (0, 0, 0, 0, NONE, NONE, NONE, 0, 0, 0.0)


def inside_mask(v, op, limit):
    """x OP limit compared as values; NaN is never inside, under NE too"""
    v = np.asarray(v, dtype=np.float64)
    limit = np.float64(limit)
    with np.errstate(invalid="ignore"):
        m = {GT: v > limit, GE: v >= limit, LT: v < limit, LE: v <= limit, EQ: v == limit, NE: v != limit}[op]
    return m & ~np.isnan(v)


def mask_record(m):
    """-> the nine integers of a window with the inside mask m: runs start where the mask steps up and end where it
    steps down"""
    m = np.asarray(m, dtype=bool)
    n = len(m)
    if n == 0:
        return EMPTY[:9]
    d = np.diff(np.concatenate(([0], m.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)  # run r is [starts[r], ends[r])
    if len(starts) == 0:
        return n, 0, 0, 0, NONE, NONE, NONE, 0, 0
    ln = ends - starts
    k = int(np.argmax(ln))  # the first of the largest
    return (n, int(m.sum()), len(starts), int(ln[k]), int(starts[k]), int(starts[0]), int(ends[-1]) - 1,
            int(ln[0]) if starts[0] == 0 else 0, int(ln[-1]) if ends[-1] == n else 0)


def window_excess(x, begin, count, m, limit):
    """the sum, in the aggregate's order, of fabs(x - limit) at the slots of the inside samples and -0.0 at every other
    slot of the window's tiles; +0.0 without an inside sample"""
    if not m.any():
        return 0.0
    v = np.asarray(x[begin:begin + count], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.where(m, np.abs(v - np.float64(limit)), -0.0)
    kb, ke = begin // TILE, (begin + count - 1) // TILE
    seg = np.full((ke - kb + 1) * TILE, -0.0)
    lo = begin - kb * TILE
    seg[lo:lo + count] = terms
    return float(G.pairwise(G.tile_sums(seg.reshape(-1, TILE))))


def window_runs(x, begin, count, op, limit):
    """-> the ten fields of atsc_window_runs of x[begin:begin + count] as the contract defines them"""
    if count == 0:
        return EMPTY
    m = inside_mask(x[begin:begin + count], op, limit)
    return mask_record(m) + (window_excess(x, begin, count, m, limit),)


def windows_runs(x, wins, op, limit):
    """-> structured array (the fields of atsc_window_runs) of the windows (begin, count) of x"""
    out = np.zeros(len(wins), dtype=DTYPE)
    for i, (b, c) in enumerate(wins):
        out[i] = window_runs(x, int(b), int(c), op, limit)
    return out


def merge(a, b):
    """the header's merge of record a followed by record b (tuples in FIELDS order); u64 arithmetic"""
    a = tuple(int(v) for v in a[:9]) + (float(a[9]),)
    b = tuple(int(v) for v in b[:9]) + (float(b[9]),)
    if b[0] == 0:
        return a
    if a[0] == 0:
        return b
    (sa, ia, ra, la, lat_a, fa, _, ha, ta, ea) = a
    (sb, ib, rb, lb, lat_b, fb, tb_at, hb, tb, eb) = b
    M = 2 ** 64
    o = sa
    join = ta != 0 and hb != 0
    lg, at = la, lat_a
    if join and (ta + hb) % M > lg:
        lg, at = (ta + hb) % M, (o - ta) % M
    if lb > lg:
        lg, at = lb, (lat_b + o) % M
    return ((sa + sb) % M, (ia + ib) % M, (ra + rb - (1 if join else 0)) % M, lg, at,
            fa if ia else ((fb + o) % M if ib else NONE), (tb_at + o) % M if ib else a[6],
            (sa + hb) % M if ha == sa else ha, (sb + ta) % M if tb == sb else tb,
            float(np.float64(ea) + np.float64(eb)))


def merge_all(recs):
    """atsc_runs_merge: left to right, empty records skipped"""
    acc = EMPTY
    for r in recs:
        acc = merge(acc, tuple(r))
    return acc


def _scaled_int(v):
    """v * 2^1074 as an integer (exact for every finite double)"""
    num, den = float(v).as_integer_ratio()
    return num * ((1 << 1074) // den)


def exact_excess(v, op, limit):
    """-> (inside, excess) of the window v with finite or NaN samples: the sum of the exact |x - limit| (not of the
    rounded ones) as a Fraction"""
    v = np.asarray(v, dtype=np.float64)
    m = inside_mask(v, op, limit)
    lim = _scaled_int(limit)
    tot = sum(abs(_scaled_int(q) - lim) for q in v[m])
    return int(m.sum()), tot * Fraction(1, 1 << 1074)


def bound_factor(inside):
    """(L + 3) u with L = max(1, ceil(log2 inside)): one rounding for the subtract, L + 2 for the tree"""
    L = max(1, math.ceil(math.log2(inside))) if inside > 1 else 1
    return (L + 3) * U
