"""NumPy restatement of the windowed rolling runs' contract (include/atsc_hip.h, DESIGN.md "Windowed rolling runs"), from
the full decode's samples: the runs' inside mask and terms (tests/runs_model.py), the nodes of the aligned chunks level by
level under the header's merge rule with positions counted from the chunk's first sample, T level by level over the
terms, and the chunk walk and left-to-right fold of the rolling (tests/rolling_model.py).

window_record() is the contract read literally, one window at a time: the nine integers off the window's inside mask
(runs_model.mask_record, no merge at all), excess by the chunk fold.  Pyramid does the same for many windows at once, the
integers by the merge rule over the chunks; tests/test_rolling_runs_host.py holds the two together."""
import math

import numpy as np

from tests import rolling_model as R
from tests import runs_model as M

U = R.U
NONE = M.NONE
FIELDS = M.FIELDS
RECORD = M.DTYPE
outputs = R.outputs
chunks = R.chunks

_INTS = ("inside", "runs", "longest", "head", "tail", "longest_at", "first_at", "last_at")


def slot_terms(x, op, limit):
    """-> (inside mask, term) per slot of the stream x: fabs(x - limit) (one rounded subtract) where x is inside, else
    -0.0"""
    x = np.asarray(x, dtype=np.float64)
    m = M.inside_mask(x, op, limit)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.where(m, np.abs(x - np.float64(limit)), -0.0)
    return m, t


def window_excess(t, any_inside, lo, w):
    """the fold of T over the window's chunks; +0.0 without an inside sample"""
    if not any_inside:
        return 0.0
    s = None
    with np.errstate(invalid="ignore", over="ignore"):
        for pos, l in chunks(lo, w):
            c = R.T(t, pos, l)
            s = c if s is None else s + c
    return float(s)


def window_record(x, lo, w, op, limit):
    """-> the ten fields of the position whose window is x[lo:lo + w]"""
    m, t = slot_terms(x, op, limit)
    mw = m[lo:lo + w]
    return M.mask_record(mw) + (window_excess(t, bool(mw.any()), lo, w),)


def listed(begins, counts, w, s):
    """-> [(lo, w)]: the windows of a call's positions, range after range"""
    return [(int(b) + j * s, w) for b, c in zip(begins, counts) for j in range(outputs(int(c), w, s))]


def bound_factor(w):
    """(3 L + 1) u with L = max(1, ceil(log2 w)): one rounding for the subtract, then the rolling's 3 L"""
    L = max(1, math.ceil(math.log2(w))) if w > 1 else 1
    return (3 * L + 1) * U


def merge_nodes(a, la, b, lb):
    """the header's merge rule on arrays of nodes: a (of la samples each) followed by b (of lb), b's positions moved
    behind a.  A node without an inside sample holds 0 in first_at and last_at, one without a run 0 in longest_at.
    Strict comparisons: of equal runs the earliest stays."""
    la, lb = np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64)
    join = (a["tail"] != 0) & (b["head"] != 0)
    r = {"inside": a["inside"] + b["inside"], "runs": a["runs"] + b["runs"] - join}
    r["head"] = np.where(a["head"] == la, la + b["head"], a["head"])
    r["tail"] = np.where(b["tail"] == lb, lb + a["tail"], b["tail"])
    r["first_at"] = np.where(a["inside"] > 0, a["first_at"], np.where(b["inside"] > 0, la + b["first_at"], 0))
    r["last_at"] = np.where(b["inside"] > 0, la + b["last_at"], a["last_at"])
    lg, at = a["longest"], a["longest_at"]
    jl = a["tail"] + b["head"]
    take = join & (jl > lg)
    lg, at = np.where(take, jl, lg), np.where(take, la - a["tail"], at)
    take = b["longest"] > lg
    lg, at = np.where(take, b["longest"], lg), np.where(take, la + b["longest_at"], at)
    r["longest"], r["longest_at"] = lg, at
    with np.errstate(invalid="ignore", over="ignore"):
        r["excess"] = a["excess"] + b["excess"]
    return r


class Pyramid:
    """the chunk partials of a stream under one condition, level by level, and the records of many windows read off them"""

    def __init__(self, x, op, limit):
        self.x = np.asarray(x, dtype=np.float64)
        m, t = slot_terms(self.x, op, limit)
        i = m.astype(np.int64)
        z = np.zeros(len(i), dtype=np.int64)
        self.levels = [{"inside": i, "runs": i, "longest": i, "head": i, "tail": i, "longest_at": z, "first_at": z,
                        "last_at": z, "excess": t}]

    def _level(self, l):
        while len(self.levels) <= l:
            p = self.levels[-1]
            n = len(p["inside"]) // 2 * 2
            half = 1 << (len(self.levels) - 1)
            self.levels.append(merge_nodes({k: v[0:n:2] for k, v in p.items()}, half, {k: v[1:n:2] for k, v in p.items()}, half))

    def records(self, lo, w):
        """-> RECORD array: the windows x[lo[i]:lo[i] + w]"""
        lo = np.asarray(lo, dtype=np.int64)
        out = np.zeros(len(lo), dtype=RECORD)
        if len(lo) == 0:
            return out
        assert w >= 1 and lo.min() >= 0 and lo.max() + w <= len(self.x)
        self._level(max(int(math.floor(math.log2(w))), 0))
        pos, hi = lo.copy(), lo + w
        acc = {k: np.zeros(len(lo), dtype=np.int64) for k in _INTS}
        acc["excess"] = np.full(len(lo), -0.0)  # (-0.0 + t is t, bit for bit)
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
                r = merge_nodes({k: v[at] for k, v in acc.items()}, pos[at] - lo[at], {k: v[j] for k, v in self.levels[l].items()},
                                1 << int(l))
                for k in acc:
                    acc[k][at] = r[k]
                pos[at] += 1 << l
        some, run = acc["inside"] > 0, acc["runs"] > 0
        out["samples"] = w
        for k in ("inside", "runs", "longest", "head", "tail"):
            out[k] = acc[k].astype(np.uint64)
        out["longest_at"] = np.where(run, acc["longest_at"], -1).astype(np.int64).view(np.uint64)
        out["first_at"] = np.where(some, acc["first_at"], -1).astype(np.int64).view(np.uint64)
        out["last_at"] = np.where(some, acc["last_at"], -1).astype(np.int64).view(np.uint64)
        out["excess"] = np.where(some, acc["excess"], 0.0)
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
