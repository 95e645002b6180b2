"""NumPy restatement of the windowed deltas' contract (include/atsc_hip.h, DESIGN.md "Windowed deltas"): the pairs of
stream-adjacent samples of a window, their terms at the slot of the pair's second sample, and the three sums in the
aggregate sum's tree (tests/agg_model.py), from the full decode's samples; what atsc_delta_derive reads off a record;
exact sums in rational arithmetic and the documented error bound."""
import math
from fractions import Fraction

import numpy as np

from tests import agg_model as G

TILE = G.TILE
U = 2.0 ** -53

FIELDS = ("pairs", "rises", "falls", "up", "down", "after_falls", "max_rise", "max_fall")
DTYPE = np.dtype([(k, "<u8") for k in FIELDS[:3]] + [(k, "<f8") for k in FIELDS[3:]])
FIT_FIELDS = ("changes", "variation", "net", "increase", "mean_step")


def _pairs(x, begin, count):
    """-> (a, b, counted, rise, fall) of the pairs j = begin + 1 .. begin + count - 1 of x"""
    v = np.asarray(x[begin:begin + count], dtype=np.float64)
    a, b = v[:-1], v[1:]
    counted = ~np.isnan(a) & ~np.isnan(b)
    with np.errstate(invalid="ignore"):
        return a, b, counted, counted & (b > a), counted & (b < a)


def _tree(begin, count, terms):
    """the sum, in the aggregate's order, of terms[i] at slot begin + 1 + i and -0.0 at every other slot of the
    window's tiles"""
    kb, ke = begin // TILE, (begin + count - 1) // TILE
    seg = np.full((ke - kb + 1) * TILE, -0.0)
    lo = begin + 1 - kb * TILE
    seg[lo:lo + len(terms)] = terms
    return float(G.pairwise(G.tile_sums(seg.reshape(-1, TILE))))


def window_delta(x, begin, count):
    """-> (pairs, rises, falls, up, down, after_falls, max_rise, max_fall) of x[begin:begin + count] as the contract
    defines them"""
    if count <= 1:
        return 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0
    a, b, counted, rise, fall = _pairs(x, begin, count)
    with np.errstate(invalid="ignore", over="ignore"):
        r, f = b - a, a - b  # one rounded subtract each
    n_r, n_f = int(rise.sum()), int(fall.sum())
    up = _tree(begin, count, np.where(rise, r, -0.0)) if n_r else 0.0
    down = _tree(begin, count, np.where(fall, f, -0.0)) if n_f else 0.0
    after = _tree(begin, count, np.where(fall, b, -0.0)) if n_f else 0.0
    return (int(counted.sum()), n_r, n_f, up, down, after, float(np.max(r[rise])) if n_r else 0.0,
            float(np.max(f[fall])) if n_f else 0.0)


def windows_delta(x, wins):
    """-> structured array (the fields of atsc_window_delta) of the windows (begin, count) of x"""
    out = np.zeros(len(wins), dtype=DTYPE)
    for i, (b, c) in enumerate(wins):
        out[i] = window_delta(x, int(b), int(c))
    return out


def derive(pairs, rises, falls, up, down, after_falls, max_rise=0.0, max_fall=0.0):
    """atsc_delta_derive of one record -> (changes, variation, net, increase, mean_step)"""
    up, down, after_falls = np.float64(up), np.float64(down), np.float64(after_falls)
    with np.errstate(all="ignore"):
        variation = up + down
        mean_step = variation / np.float64(int(pairs)) if int(pairs) else np.float64("nan")
        return (int(rises) + int(falls)) % 2 ** 64, variation, up - down, up + after_falls, mean_step


def _scaled_int(v):
    """v * 2^1074 as an integer (exact for every finite double)"""
    num, den = float(v).as_integer_ratio()
    return num * ((1 << 1074) // den)


def exact_delta(v):
    """-> (pairs, up, down, after_falls) of the window v with finite or NaN samples: the sums of the exact differences
    (not of the rounded ones) as Fractions"""
    v = np.asarray(v, dtype=np.float64)
    s = [None if math.isnan(q) else _scaled_int(q) for q in v]
    pairs = up = down = after = 0
    for a, b in zip(s[:-1], s[1:]):
        if a is None or b is None:
            continue
        pairs += 1
        if b > a:
            up += b - a
        elif b < a:
            down += a - b
            after += b
    one = Fraction(1, 1 << 1074)
    return pairs, up * one, down * one, after * one


def bound_factor(pairs):
    """(L + 3) u with L = max(1, ceil(log2 pairs)): one rounding for the subtract, L + 2 for the tree"""
    L = max(1, math.ceil(math.log2(pairs))) if pairs > 1 else 1
    return (L + 3) * U
