"""NumPy restatement of the windowed extremes' contract (include/atsc_hip.h, DESIGN.md "Windowed extremes"): the k largest
and the k smallest non-NaN samples of a window by a stable sort of the full decode's samples, the merge rule of
atsc_extremes_merge, and the two kernels' selection written as plain functions over k_ext_tiles' slot-to-lane mapping
(lane-bests, the bitonic network, the threshold, the candidates in the order the ballots give them, the shifting insert)
and k_ext_combine's pop order, so that both can be checked against the sort without a GPU."""
import struct

import numpy as np

TILE = 2048
NONE = 2 ** 64 - 1
MAX_K = 16
EXTREME = np.dtype([("value", "<f8"), ("at", "<u8")])


def dtype(k):
    return np.dtype([("count", "<u8"), ("nans", "<u8"), ("largest", EXTREME, (k,)), ("smallest", EXTREME, (k,))])


def _first(w, k):
    """-> the positions of the k first of w ascending, equal values earliest first, NaN dropped: the head of
    np.argsort(w, kind="stable").  A long window is cut down to the values up to the k-th first."""
    idx = np.flatnonzero(~np.isnan(w))
    if len(idx) > 8 * k:
        thr = np.partition(w[idx], k - 1)[k - 1]
        idx = idx[w[idx] <= thr]
    return idx[np.argsort(w[idx], kind="stable")][:k]


def window_extremes(x, begin, count, k):
    """-> the record of the window [begin, begin + count) of x, a 0-d array of dtype(k)"""
    r = np.zeros((), dtype=dtype(k))
    for name in ("largest", "smallest"):
        r[name]["value"] = np.nan
        r[name]["at"] = NONE
    v = np.asarray(x[begin:begin + count], dtype=np.float64)
    r["count"] = count
    r["nans"] = int(np.isnan(v).sum())
    for name, w in (("largest", -v), ("smallest", v)):
        at = _first(w, k)
        r[name]["value"][: len(at)] = v[at]
        r[name]["at"][: len(at)] = at
    return r


def windows_extremes(x, wins, k):
    out = np.zeros(len(wins), dtype=dtype(k))
    for i, (b, c) in enumerate(wins):
        out[i] = window_extremes(x, b, c, k)
    return out


def head_of(records, j):
    """the records of a call with j <= k from those of a call with k: the first j entries of each list"""
    out = np.zeros(len(records), dtype=dtype(j))
    out["count"], out["nans"] = records["count"], records["nans"]
    out["largest"], out["smallest"] = records["largest"][:, :j], records["smallest"][:, :j]
    return out


def words(records):
    """the records as rows of 2 + 4 k unsigned words, every NaN replaced by one NaN: equal rows are equal records"""
    r = np.ascontiguousarray(np.atleast_1d(records))
    w = r.view(np.uint64).reshape(len(r), -1).copy()
    f = w.view(np.float64)
    k = (w.shape[1] - 2) // 4
    for c in range(2, 2 + 4 * k, 2):
        w[np.isnan(f[:, c]), c] = 0x7FF8000000000000
    return w


def merge(records, k):
    """the header's rule, left to right, on tuples: count and nans add, every `at` is shifted by the counts in front of
    it, a list is the first k of the parts' entries in the list's order (Python's sort is stable, and the parts come in
    stream order)"""
    out = np.zeros((), dtype=dtype(k))
    for name in ("largest", "smallest"):
        out[name]["value"] = np.nan
        out[name]["at"] = NONE
    base = 0
    ents = {"largest": [], "smallest": []}
    for r in records:
        if int(r["count"]) == 0:
            continue
        for name in ents:
            ents[name] += [(float(e["value"]), int(e["at"]) + base) for e in r[name] if int(e["at"]) != NONE]
        base += int(r["count"])
        out["nans"] += r["nans"]
    out["count"] = base
    for name, sign in (("largest", -1.0), ("smallest", 1.0)):
        best = sorted(ents[name], key=lambda e: (sign * e[0] + 0.0, e[1]))[:k]  # (-0.0 + 0.0 is +0.0: the zeros tie)
        for j, (v, at) in enumerate(best):
            out[name][j] = (v, at)
    return out


# ---- the kernels' selection as plain functions ------------------------------------------------
def key(v):
    """k_ext_tiles' key under the largest list's reading; 0 for NaN"""
    if v != v:
        return 0
    b = 0 if v == 0.0 else struct.unpack("<Q", struct.pack("<d", v))[0]
    return b ^ (0xFFFFFFFFFFFFFFFF if b >> 63 else 0x8000000000000000)


def _ahead(ka, pa, kb, pb):
    return ka > kb or (ka == kb and pa < pb)


def _sort(ent):
    """the bitonic network of ext_sort over 64 (key, pos) entries, one per lane"""
    ent = list(ent)
    size = 2
    while size <= 64:
        stride = size >> 1
        while stride:
            new = list(ent)
            for lane in range(64):
                ok, op = ent[lane ^ stride]
                k0, p0 = ent[lane]
                lower, desc = (lane & stride) == 0, (lane & size) == 0
                other = _ahead(ok, op, k0, p0)
                if other if lower == desc else not other:
                    new[lane] = (ok, op)
            ent = new
            stride >>= 1
        size <<= 1
    return ent


def _insert(lst, ck, cp):
    """ext_insert on the list's lanes"""
    new = list(lst)
    for lane in range(len(lst)):
        here = _ahead(ck, cp, *lst[lane])
        left = lane != 0 and _ahead(ck, cp, *lst[lane - 1])
        if here:
            new[lane] = lst[lane - 1] if left else (ck, cp)
    return new


def tile_select(x, lo, hi, k):
    """k_ext_tiles on the slots [lo, hi) of the 2048 samples x -> (nans, largest, smallest, candidates): the lists as
    slot numbers (None where empty), and the number of insertions per end"""
    NO = (0, 0xFFFFFFFF)
    keys = [[0] * TILE, [0] * TILE]
    nans = 0
    for p in range(lo, hi):
        kl = key(float(x[p]))
        nans += kl == 0
        keys[0][p] = kl
        keys[1][p] = (kl ^ 0xFFFFFFFFFFFFFFFF) if kl else 0
    lists, cands = [], []
    for end in range(2):
        kk_ = keys[end]
        best = [NO] * 64
        for lane in range(64):
            for kk in range(4):
                for q in range(4):
                    for e in range(2):
                        p = 512 * q + 2 * (lane + 64 * kk) + e
                        if kk_[p] and _ahead(kk_[p], p, *best[lane]):
                            best[lane] = (kk_[p], p)
        lst = _sort(best)
        thr = lst[k - 1]
        lst = lst[:k]
        n = 0
        if k > 1:
            for kk in range(4):
                for q in range(4):
                    for e in range(2):
                        for src in range(64):  # the ballot's bits from the lowest lane up
                            p = 512 * q + 128 * kk + 2 * src + e
                            if kk_[p] and p != best[src][1] and _ahead(kk_[p], p, *thr):
                                lst = _insert(lst, kk_[p], p)
                                n += 1
        lists.append([p if kq else None for kq, p in lst])
        cands.append(n)
    return nans, lists[0], lists[1], cands


def combine_pop(parts, k, end):
    """k_ext_combine's rounds over up to 64 lists in stream order, each a list of (value, at) without the empty
    entries: the wave maximum of the heads' keys, of equal keys the lowest lane, whose cursor advances"""
    cur = [0] * len(parts)
    out = []

    def head(i):
        if cur[i] >= min(k, len(parts[i])):
            return 0
        kl = key(parts[i][cur[i]][0])
        return (kl ^ 0xFFFFFFFFFFFFFFFF) if end else kl

    for _ in range(k):
        hk = [head(i) for i in range(len(parts))]
        mx = max(hk, default=0)
        if mx == 0:
            break
        w = hk.index(mx)
        out.append(parts[w][cur[w]])
        cur[w] += 1
    return out
