"""NumPy restatement of the windowed value counts' contract (include/atsc_hip.h, DESIGN.md "Windowed value counts"): the
k smallest distinct values of a window above `above` with their multiplicities by numpy.unique over the full decode's
samples, the merge rule of atsc_values_merge on tuples, atsc_values_mode, and the two kernels' counting written as plain
functions over k_val_tiles' slot-to-lane mapping and k_val_combine's cursors, so that both can be checked against
numpy.unique without a GPU."""
import math

import numpy as np

TILE = 2048
MAX_K = 32
VALUE_COUNT = np.dtype([("value", "<f8"), ("n", "<u8")])
VALUE_MODE = np.dtype([("value", "<f8"), ("n", "<u8"), ("exact", "<u4"), ("pad", "<u4")])


def dtype(k):
    return np.dtype([("count", "<u8"), ("nans", "<u8"), ("below", "<u8"), ("distinct", "<u4"), ("more", "<u4"),
                     ("entry", VALUE_COUNT, (k,))])


def empty(k):
    r = np.zeros((), dtype=dtype(k))
    r["entry"]["value"] = np.nan
    return r


def _fill(r, k, values, counts):
    d = min(len(values), k)
    r["distinct"] = d
    r["more"] = int(len(values) > k)
    r["entry"]["value"][:d] = values[:d]
    r["entry"]["n"][:d] = counts[:d]


def window_values(x, begin, count, k, above=math.nan):
    """-> the record of the window [begin, begin + count) of x, a 0-d array of dtype(k)"""
    r = empty(k)
    v = np.asarray(x[begin:begin + count], dtype=np.float64)
    r["count"] = count
    r["nans"] = int(np.isnan(v).sum())
    w = v[~np.isnan(v)] + 0.0  # (-0.0 + 0.0 is +0.0: the zeros are one value, reported as +0.0; nothing else changes)
    if not math.isnan(above):
        listed = w > above
        r["below"] = int((~listed).sum())
        w = w[listed]
    u, c = np.unique(w, return_counts=True)
    _fill(r, k, u, c)
    return r


def windows_values(x, wins, k, above=math.nan):
    out = np.zeros(len(wins), dtype=dtype(k))
    for i, (b, c) in enumerate(wins):
        out[i] = window_values(x, b, c, k, above)
    return out


def head_of(records, j):
    """the records of a call with j <= k from those of a call with k (same above): the first j entries, distinct =
    min(distinct_k, j), more = distinct_k > j or more_k"""
    out = np.zeros(len(records), dtype=dtype(j))
    for name in ("count", "nans", "below"):
        out[name] = records[name]
    out["distinct"] = np.minimum(records["distinct"], j)
    out["more"] = (records["distinct"] > j) | (records["more"] != 0)
    out["entry"] = records["entry"][:, :j]
    return out


def words(records):
    """the records as rows of 4 + 2 k unsigned words, every NaN replaced by one NaN: equal rows are equal records"""
    r = np.ascontiguousarray(np.atleast_1d(records))
    w = r.view(np.uint64).reshape(len(r), -1).copy()
    f = w.view(np.float64)
    for c in range(4, w.shape[1], 2):
        w[np.isnan(f[:, c]), c] = 0x7FF8000000000000
    return w


def merge(records, k):
    """the header's rule on tuples: the heads add, the lists merge by value with the n of equal values added, the result
    is cut at k, more is set iff an entry was cut or a part had more; records with count == 0 are skipped"""
    out = empty(k)
    tally = {}
    more = False
    for r in np.atleast_1d(records):
        if int(r["count"]) == 0:
            continue
        for name in ("count", "nans", "below"):
            out[name] += r[name]
        more = more or int(r["more"]) != 0
        for e in r["entry"][: int(r["distinct"])]:
            tally[float(e["value"])] = tally.get(float(e["value"]), 0) + int(e["n"])
    values = sorted(tally)
    _fill(out, k, values, [tally[v] for v in values])
    out["more"] = int(more or len(values) > k)
    return out


def mode(records):
    """atsc_values_mode: of every record the listed entry with the largest n, the smallest value on ties"""
    rs = np.atleast_1d(records)
    out = np.zeros(len(rs), dtype=VALUE_MODE)
    for i, r in enumerate(rs):
        best = (math.nan, 0)
        for e in r["entry"][: int(r["distinct"])]:
            if int(e["n"]) > best[1]:
                best = (float(e["value"]), int(e["n"]))
        out[i] = (best[0], best[1], int(int(r["more"]) == 0), 0)
    return out


# ---- the kernels' counting as plain functions -------------------------------------------------
NO_KEY = 0xFFFFFFFFFFFFFFFF


def key(v):
    """sample_key (atsc_tile_reduce.h): unsigned order is value order, both zeros on +0.0's key; 0 for NaN"""
    if v != v:
        return 0
    b = 0 if v == 0.0 else int(np.float64(v).view(np.uint64))
    return b ^ (NO_KEY if b >> 63 else 0x8000000000000000)


def key_value(k):
    """val_bits: the value of a key, +0.0 for the zeros' key"""
    b = k ^ 0x8000000000000000 if k >> 63 else k ^ NO_KEY
    return float(np.uint64(b).view(np.float64))


def tile_count(x, lo, hi, k, above=math.nan):
    """k_val_tiles on the slots [lo, hi) of the 2048 samples x -> (the partial, a 0-d array of dtype(k), and the rounds
    it took): every lane's 32 keys by the kernel's slot-to-lane mapping, then rounds of wave minimum, count and knock-out"""
    akey = key(above)
    keys = [[NO_KEY] * 32 for _ in range(64)]
    nans = below = 0
    for lane in range(64):
        for kk in range(4):
            for q in range(4):
                for e in range(2):
                    p = 512 * q + 2 * (lane + 64 * kk) + e
                    ks = key(float(x[p])) if lo <= p < hi else 0
                    listed = ks > akey
                    nans += lo <= p < hi and x[p] != x[p]
                    below += ks != 0 and not listed
                    keys[lane][8 * kk + 2 * q + e] = ks if listed else NO_KEY
    r = empty(k)
    r["count"], r["nans"], r["below"] = hi - lo, nans, below
    rounds = distinct = 0
    for rnd in range(k + 1):
        m = min(min(l) for l in keys)
        rounds += 1
        if m == NO_KEY:
            break
        if rnd == k:
            r["more"] = 1
            break
        c = 0
        for l in keys:
            for j in range(32):
                if l[j] == m:
                    c += 1
                    l[j] = NO_KEY
        r["entry"][rnd] = (key_value(m), c)
        distinct = rnd + 1
    r["distinct"] = distinct
    return r, rounds


def combine(parts, k):
    """k_val_combine over up to 64 partials, one per lane -> the group's partial: cursors into the lists, the wave
    minimum of the heads' keys, the n of every lane that holds it added, those lanes' cursors advanced"""
    assert len(parts) <= 64
    out = empty(k)
    for name in ("count", "nans", "below"):
        out[name] = sum(int(p[name]) for p in parts)
    nd = [min(int(p["distinct"]), k) for p in parts]
    cur = [0] * len(parts)

    def head(i):
        return key(float(parts[i]["entry"]["value"][cur[i]])) if cur[i] < nd[i] else NO_KEY

    distinct = 0
    for rnd in range(k):
        hk = [head(i) for i in range(len(parts))]
        m = min(hk, default=NO_KEY)
        if m == NO_KEY:
            break
        s = 0
        for i in range(len(parts)):
            if hk[i] == m:
                s += int(parts[i]["entry"]["n"][cur[i]])
                cur[i] += 1
        out["entry"][rnd] = (key_value(m), s)
        distinct = rnd + 1
    out["distinct"] = distinct
    out["more"] = int(any(head(i) != NO_KEY or int(parts[i]["more"]) for i in range(len(parts))))
    return out
