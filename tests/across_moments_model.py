"""NumPy model of the windowed across moments' contract (include/atsc_hip.h, DESIGN.md "Windowed across moments"): the
record of a position is the x half (n, mx, M2x) of Merge(.. Merge(Merge(leaf_0, leaf_1), leaf_2) .., leaf_(N-1)) over
the column x_0 .. x_(N-1) of the N streams' samples there, Merge being the windowed moments' rule
(moments_model.merge) and leaf_k = (1, x_k, 0), or the empty node where x_k is NaN.  `records` folds whole arrays of
positions at a time; tests/test_across_moments_host.py holds it to a scalar, line-by-line restatement of the rule.  Also
atsc_across_moments_merge (`merge_records`), atsc_across_moments_fit (`fit`), and exact values and the documented bounds
(moments_model.exact_moments).  Ranges and record numbering are the across' (tests/across_model.py)."""
import math

import numpy as np

from tests import across_extremes_model
from tests import across_model
from tests import moments_model as MM

U = MM.U
dtype = np.dtype([("count", "<u4"), ("nans", "<u4"), ("mean", "<f8"), ("m2", "<f8")])  # atsc_across_moments
fit_dtype = np.dtype([("mean", "<f8"), ("variance", "<f8"), ("stddev", "<f8"), ("sample_variance", "<f8"),
                      ("sample_stddev", "<f8")])  # atsc_across_fit
columns = across_extremes_model.columns


def _node(n, mx, m2):
    """(n, mx, M2x) as a node of moments_model.merge: the position half stays zero"""
    z = np.zeros(np.shape(n))
    return np.asarray(n, dtype=np.uint64), np.asarray(mx, dtype=np.float64), np.asarray(m2, dtype=np.float64), z, z, z


def _from_nodes(node, nans):
    n, mx, m2 = node[0], node[1], node[2]
    out = np.zeros(len(n), dtype=dtype)
    out["count"] = n
    out["nans"] = nans
    out["mean"] = np.where(n > 0, mx, np.nan)
    out["m2"] = np.where(n > 0, m2, np.nan)
    return out


def records(x):
    """x: (N, P) samples, a column per position.  -> P records: the left fold of the N leaves in list order"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n_streams, p = x.shape
    acc = _node(np.zeros(p), np.zeros(p), np.zeros(p))
    for k in range(n_streams):
        ok = ~np.isnan(x[k])
        acc = MM.merge(acc, _node(ok, np.where(ok, x[k], 0.0), np.zeros(p)))
    return _from_nodes(acc, np.isnan(x).sum(axis=0))


def across_moments(fulls, begins, counts, stride=1):
    """-> (records, off) of the call over the decoded streams `fulls` (sample j of one goes with sample j of every
    other)"""
    return records(columns(fulls, begins, counts, stride)), across_model.offsets(counts, stride)


def merge_records(parts):
    """parts: a list of arrays of P records each (one per sub-list, in list order).  -> the P records that
    atsc_across_moments_merge gives position by position: the left fold by the general Merge from the empty node, a
    record with count == 0 being the empty node; count and nans added"""
    p = len(parts[0]) if len(parts) else 1
    acc = _node(np.zeros(p), np.zeros(p), np.zeros(p))
    nans = np.zeros(p, dtype=np.uint64)
    for r in parts:
        r = np.atleast_1d(r)
        some = r["count"] > 0
        acc = MM.merge(acc, _node(r["count"], np.where(some, r["mean"], 0.0), np.where(some, r["m2"], 0.0)))
        nans = nans + r["nans"]
    return _from_nodes(acc, nans)


def fit(rec):
    """atsc_across_moments_fit of an array of records -> fit_dtype array: atsc_moments_fit's definitions, one rounded
    operation each"""
    rec = np.atleast_1d(rec)
    out = np.zeros(len(rec), dtype=fit_dtype)
    n = rec["count"].astype(np.float64)
    some = rec["count"] > 0
    with np.errstate(all="ignore"):
        var = np.where(some, rec["m2"] / n, np.nan)
        svar = np.where(rec["count"] >= 2, rec["m2"] / (n - 1.0), np.nan)
        out["mean"] = np.where(some, rec["mean"], np.nan)
        out["variance"], out["stddev"] = var, np.sqrt(var)
        out["sample_variance"], out["sample_stddev"] = svar, np.sqrt(svar)
    return out


def words(rec):
    """the records as 3 uint64 words each, every NaN as one NaN: bit for bit, any NaN equal to any NaN"""
    r = np.ascontiguousarray(np.atleast_1d(rec))
    f = r.view(np.float64).reshape(len(r), -1).copy()
    f[:, 1:][np.isnan(f[:, 1:])] = np.nan  # (word 0 is count and nans)
    return f.view(np.uint64)


def same(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return len(a) == 0 or bool(np.array_equal(words(a), words(b)))


def exact(column):
    """-> (n, mean, m2, mean|x|) of the column's finite samples as Fractions (None where n == 0)"""
    n, mean, m2, _, _, _, mabs = MM.exact_moments(np.asarray(column, dtype=np.float64))
    return n, mean, m2, mabs


def bounds(n, mean, m2, mabs):
    """the documented bounds (on mean, on m2) from the exact values: (n + 2) u mean|x| and (n + 2) u kappa m2, with
    kappa m2 = sqrt(m2 (m2 + n mean^2)) as moments_model.bounds writes it"""
    k = (n + 2) * U
    m2f = float(m2)
    return k * float(mabs), k * math.sqrt(m2f * (m2f + n * float(mean) ** 2))
