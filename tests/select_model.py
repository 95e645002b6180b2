"""NumPy restatement of the windowed select's contract (include/atsc_hip.h, DESIGN.md "Windowed select"): per window the
samples that meet the condition, in ascending position, as (value bits, offset from the window's begin), window after
window in the order given; the offsets are the true counts whatever `cap` is, the entries the first `cap`."""
import numpy as np

GT, GE, LT, LE, EQ, NE = range(6)
OPS = (GT, GE, LT, LE, EQ, NE)
DTYPE = np.dtype([("value", "<f8"), ("at", "<u8")])


def selected_mask(v, op, limit):
    """x OP limit compared as values; NaN is never selected, under NE too"""
    v = np.asarray(v, dtype=np.float64)
    limit = np.float64(limit)
    with np.errstate(invalid="ignore"):
        m = {GT: v > limit, GE: v >= limit, LT: v < limit, LE: v <= limit, EQ: v == limit, NE: v != limit}[op]
    return m & ~np.isnan(v)


def windows_select(full, wins, op, limit, cap):
    """-> (off, entries): off[0 .. len(wins)] as uint64, entries the first min(off[-1], cap) selected samples"""
    full = np.asarray(full, dtype=np.float64)
    off = np.zeros(len(wins) + 1, dtype=np.uint64)
    parts = []
    for i, (b, c) in enumerate(wins):
        v = full[int(b):int(b) + int(c)]
        at = np.flatnonzero(selected_mask(v, op, limit))
        e = np.zeros(len(at), dtype=DTYPE)
        e["value"] = v[at]  # a copy of the bits: -0.0 stays -0.0
        e["at"] = at
        parts.append(e)
        off[i + 1] = off[i] + np.uint64(len(at))
    entries = np.concatenate(parts) if parts else np.zeros(0, dtype=DTYPE)
    return off, entries[: min(int(off[-1]), int(cap))]
