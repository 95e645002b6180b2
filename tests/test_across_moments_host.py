"""The windowed across moments without a GPU: the vectorised NumPy model (tests/across_moments_model.py) against a scalar,
line-by-line restatement of the contract's rule, hand values, and exact rational arithmetic within the documented
(n + 2) u bounds on the windowed moments' input families laid across streams; what the header says follows (m2 == 0.0
on equal values and at count == 1, NaN at count == 0, count and nans under a reordering); atsc_across_moments_merge and
atsc_across_moments_fit (the C functions) bit for bit against the model, the singleton property, sub-lists of 64 up to
N = 400 within the bounds, the empty merge and the errors; the new symbols, the public surfaces and the command line's
argument errors (exit 2 before any GPU work)."""
import ctypes as C
import inspect
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import across_model as AM
from tests import across_moments_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATSC = os.path.join(ROOT, "atsc_amd", "bin", "atsc")
NAN, INF = np.nan, np.inf
SIZES = [1, 2, 3, 5, 8, 17, 33, 63, 64]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _scalar(column):
    """the contract, line by line, on one column -> (count, nans, mean, m2)"""
    f8 = np.float64
    n, nans, mean, m2 = 0, 0, f8(NAN), f8(NAN)
    with np.errstate(all="ignore"):
        for x in column:
            x = f8(x)
            if np.isnan(x):  # the empty leaf: Merge(a, empty) is a
                nans += 1
                continue
            if n == 0:  # Merge(empty, leaf) is the leaf (1, x, 0)
                n, mean, m2 = 1, x, f8(0.0)
                continue
            na = n
            n = na + 1
            w = f8(1.0) / f8(n)
            f = f8(na) * w
            dx = x - mean
            mean = mean + dx * w
            m2 = (m2 + f8(0.0)) + (dx * dx) * f
    return n, nans, mean, m2


def _families(rng, n, p):
    """the input families the windowed moments' bounds were stated on (tests/test_moments_host.py), laid across streams:
    every column of the (n, p) arrays is one draw of n samples; and random decimal scalings"""
    holes = rng.normal(0, 1, (n, p))
    holes[rng.random((n, p)) < 0.2] = NAN
    holes30 = 1e6 + rng.normal(0, 1, (n, p))
    holes30[rng.random((n, p)) < 0.3] = NAN
    return {"normal": rng.normal(0, 1, (n, p)), "offset1e6": 1e6 + rng.normal(0, 1, (n, p)),
            "offset1e9": 1e9 + rng.normal(0, 1e-3, (n, p)),
            "ramp": 0.25 * np.arange(n)[:, None] + rng.normal(0, 3, (n, p)), "walk": np.cumsum(rng.normal(0, 1, (n, p)), axis=0),
            "constant": np.full((n, p), 1234.5678), "nan20": holes, "offset1e6_nan30": holes30,
            "decimal": rng.normal(0, 1, (n, p)) * 10.0 ** rng.integers(-3, 4, (n, p)),
            "decimal_columns": rng.normal(0, 1, (n, p)) * 10.0 ** rng.integers(-6, 7, (1, p))}


def _hand_columns(n):
    i = np.arange(n)
    cols = [np.full(n, NAN), np.r_[np.full(n - 1, NAN), 2.5], np.r_[-7.0, np.full(n - 1, NAN)], np.full(n, 3.0),
            np.full(n, -0.0), np.where(i % 2 == 0, -0.0, 0.0), np.where(i % 3 == 0, INF, 1.0), np.where(i % 3 == 0, -INF, 1.0),
            np.where(i % 2 == 0, INF, -INF), np.where(i % 4 == 1, NAN, i // 3 * 1.5), np.where(i % 2 == 0, 1e308, -1e308),
            np.where(i % 2 == 0, 5e-324, -5e-324), np.r_[np.full(n - 1, 1e9), 1e9 + 1e-3], i[::-1].astype(np.float64)]
    return np.array(cols).T.copy()


def _assert_same(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, got.shape, want.shape)
    if not M.same(got, want):
        bad = np.argwhere((M.words(got) != M.words(want)).any(axis=1))[:, 0]
        assert False, (label, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


def _by_rule(x):
    out = np.zeros(x.shape[1], dtype=M.dtype)
    for p in range(x.shape[1]):
        out[p] = _scalar(x[:, p])
    return out


@pytest.mark.parametrize("n", SIZES)
def test_model_equals_the_rule_line_by_line(n):
    rng = np.random.default_rng(100 + n)
    for name, x in list(_families(rng, n, 12).items()) + [("hand", _hand_columns(n))]:
        got = M.records(x)
        _assert_same(got, _by_rule(x), (n, name))
        assert np.all(got["count"] + got["nans"] == n)


def test_hand_values():
    r = M.records(np.array([[2.0, 4, 4, 4, 5, 5, 7, 9]]).T)[0]
    assert (r["count"], r["nans"], r["mean"], r["m2"]) == (8, 0, 5.0, 32.0)
    r = M.records(np.array([[NAN, 2.0, NAN, 4, 4, 4, 5, NAN, 5, 7, 9, NAN]]).T)[0]  # NaN leaves are skipped
    assert (r["count"], r["nans"], r["mean"], r["m2"]) == (8, 4, 5.0, 32.0)
    r = M.records(np.array([[1.0, 2.0, 3.0]]).T)[0]
    assert (r["count"], r["mean"], r["m2"]) == (3, 2.0, 2.0)
    f = M.fit(M.records(np.array([[2.0, 4, 4, 4, 5, 5, 7, 9]]).T))[0]
    assert (f["mean"], f["variance"], f["stddev"]) == (5.0, 4.0, 2.0) and f["sample_variance"] == 32.0 / 7.0
    # a fleet at 1e9 +- 1e-3 keeps its variance; sum(x^2) - sum(x)^2 / n would not
    x = 1e9 + np.array([1e-3, -1e-3, 1e-3, -1e-3])
    r = M.records(x[:, None])[0]
    en, emean, em2, eabs = M.exact(x)
    assert abs(Fraction(float(r["m2"])) - em2) <= M.bounds(en, emean, em2, eabs)[1] < 1e-3 * em2 and 3.9e-6 < r["m2"] < 4.1e-6
    naive = np.sum(x * x) - np.sum(x) ** 2 / 4
    assert abs(naive - float(em2)) >= float(em2)  # (the variance is lost whole)


def test_model_within_bounds_of_exact():
    worst = {"mean": 0.0, "m2": 0.0}
    rng = np.random.default_rng(163)
    for n in sorted(set(SIZES + [4, 16, 32, 48])):
        for name, x in _families(rng, n, 8).items():
            rec = M.records(x)
            for p in range(x.shape[1]):
                en, emean, em2, eabs = M.exact(x[:, p])
                assert rec["count"][p] == en and rec["nans"][p] == n - en, (n, name, p)
                if en == 0:
                    assert np.isnan(rec["mean"][p]) and np.isnan(rec["m2"][p])
                    continue
                b_mean, b_m2 = M.bounds(en, emean, em2, eabs)
                for what, got, ex, lim in (("mean", rec["mean"][p], emean, b_mean), ("m2", rec["m2"][p], em2, b_m2)):
                    e = float(abs(Fraction(float(got)) - ex))
                    assert e <= lim, (n, name, p, what, e, lim)
                    if lim > 0:
                        worst[what] = max(worst[what], e / lim)
                if em2 == 0:
                    assert rec["m2"][p] == 0.0, (n, name, p)
    print("largest error / bound:", worst)
    assert worst["mean"] > 0 and worst["m2"] > 0


def test_what_follows_from_the_rule():
    rng = np.random.default_rng(167)
    for n in SIZES:
        x = _families(rng, n, 10)
        # equal values: no spread, exactly; the mean is the value
        r = M.records(x["constant"])
        assert np.all(r["m2"] == 0.0) and np.all(r["mean"] == 1234.5678) and not np.signbit(r["m2"]).any()
        # count == 1, wherever the one sample stands
        one = np.full((n, n), NAN)
        one[np.arange(n), np.arange(n)] = rng.normal(0, 1e6, n)
        r = M.records(one)
        assert np.all(r["count"] == 1) and np.all(r["m2"] == 0.0) and r["mean"].tobytes() == one.diagonal().tobytes()
        # all NaN
        r = M.records(np.full((n, 3), NAN))
        assert np.all(r["count"] == 0) and np.all(r["nans"] == n) and np.isnan(r["mean"]).all() and np.isnan(r["m2"]).all()
        # a reordered list: count and nans as they were, mean and m2 within both bounds of each other's exact value
        a, b = M.records(x["nan20"]), M.records(x["nan20"][::-1])
        assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["nans"], b["nans"])
        for p in range(10):
            en, emean, em2, eabs = M.exact(x["nan20"][:, p])
            if en:
                b_mean, b_m2 = M.bounds(en, emean, em2, eabs)
                assert abs(a["mean"][p] - b["mean"][p]) <= 2 * b_mean and abs(a["m2"][p] - b["m2"][p]) <= 2 * b_m2
    # Inf: what NumPy gives under the same operations, compared by NaN-ness (and by value where it is not NaN)
    for n in (2, 3, 8, 64):
        x = _hand_columns(n)
        got, want = M.records(x), _by_rule(x)
        for fld in ("mean", "m2"):
            assert np.array_equal(np.isnan(got[fld]), np.isnan(want[fld])) and np.array_equal(got[fld], want[fld], equal_nan=True)
        assert not np.isfinite(got["mean"][[6, 7, 8]]).any() and not np.isfinite(got["m2"][[6, 7, 8]]).any()  # columns with Inf
        assert np.isnan(got["mean"][8]) and (n < 3 or np.isnan(got["m2"][8]))  # +Inf and -Inf


def test_model_ranges(A):
    fulls = [np.arange(30.0), np.arange(30.0)[::-1].copy(), np.full(30, NAN)]
    rec, off = M.across_moments(fulls, [3, 0, 29, 5], [10, 0, 1, 15], 4)
    assert off.tolist() == [0, 3, 3, 4, 8] and rec.shape == (8,)
    assert np.all(rec["count"] == 2) and np.all(rec["nans"] == 1) and np.all(rec["mean"] == 14.5)
    assert rec["m2"].tolist() == [(29 - 2 * i) ** 2 / 2 for i in (3, 7, 11, 29, 5, 9, 13, 17)]
    assert off.tolist() == A.across_offsets([10, 0, 1, 15], 4).tolist() == AM.offsets([10, 0, 1, 15], 4).tolist()


def _merged(A, parts):
    out = np.zeros(len(parts[0]), dtype=M.dtype)
    for p in range(len(out)):
        out[p] = A.across_moments_merge(np.array([part[p] for part in parts]))
    return out


def test_merge_bit_for_bit_against_the_model(A):
    assert A.ACROSS_MOMENTS == M.dtype and A.ACROSS_MOMENTS.itemsize == 24
    rng = np.random.default_rng(173)
    for name, x in _families(rng, 64, 20).items():
        for cuts in ([64], [1, 63], [23, 41], [8] * 8, [1] * 64, [5, 0, 17, 0, 42]):
            at = np.concatenate([[0], np.cumsum(cuts)])
            parts = [M.records(x[a:b]) if b > a else M.records(np.full((1, 20), NAN)) for a, b in zip(at[:-1], at[1:])]
            _assert_same(_merged(A, parts), M.merge_records(parts), (name, cuts))
    x = _hand_columns(9)
    parts = [M.records(x[:4]), M.records(x[4:])]
    _assert_same(_merged(A, parts), M.merge_records(parts), "hand")


def test_merge_with_singletons_is_the_longer_list(A):
    rng = np.random.default_rng(179)
    for name, x in _families(rng, 40, 16).items():
        for n0 in (0, 1, 2, 17, 39):
            parts = [M.records(x[:n0])] if n0 else []
            parts += [M.records(x[k: k + 1]) for k in range(n0, 40)]  # NaN singletons (0, 1, NaN, NaN) among them
            _assert_same(_merged(A, parts), M.records(x), (name, n0))


def test_merged_sub_lists_of_64_within_the_bounds(A):
    worst = {"mean": 0.0, "m2": 0.0}
    rng = np.random.default_rng(181)
    for n in (65, 128, 200, 400):
        for name, x in _families(rng, n, 4).items():
            parts = [M.records(x[a: a + 64]) for a in range(0, n, 64)]
            got = _merged(A, parts)
            for p in range(x.shape[1]):
                en, emean, em2, eabs = M.exact(x[:, p])
                assert got["count"][p] == en and got["nans"][p] == n - en
                b_mean, b_m2 = M.bounds(en, emean, em2, eabs)
                for what, v, ex, lim in (("mean", got["mean"][p], emean, b_mean), ("m2", got["m2"][p], em2, b_m2)):
                    e = float(abs(Fraction(float(v)) - ex))
                    assert e <= lim, (n, name, p, what, e, lim)
                    if lim > 0:
                        worst[what] = max(worst[what], e / lim)
    print("largest error / bound, merged:", worst)


def test_merge_empty_and_errors(A):
    lib, Ec = A.capi.lib(), A.capi
    e = A.across_moments_merge(np.zeros(0, dtype=M.dtype))
    assert (e["count"], e["nans"]) == (0, 0) and np.isnan(e["mean"]) and np.isnan(e["m2"])
    e = A.across_moments_merge(np.array([(0, 3, NAN, NAN), (0, 2, 1.0, 1.0)], dtype=M.dtype))  # empty records only
    assert (e["count"], e["nans"]) == (0, 5) and np.isnan(e["mean"]) and np.isnan(e["m2"])
    sent = np.array([(7, 7, 7.0, 7.0)], dtype=M.dtype)
    out = sent.copy()
    big = np.array([(2 ** 31, 0, 1.0, 1.0), (2 ** 31, 0, 2.0, 1.0)], dtype=M.dtype)
    assert lib.atsc_across_moments_merge(C.c_void_p(big.ctypes.data), 2, C.c_void_p(out.ctypes.data)) == Ec.E_INVALID
    big = np.array([(1, 2 ** 32 - 1, 1.0, 0.0), (1, 1, 2.0, 0.0)], dtype=M.dtype)
    assert lib.atsc_across_moments_merge(C.c_void_p(big.ctypes.data), 2, C.c_void_p(out.ctypes.data)) == Ec.E_INVALID
    assert lib.atsc_across_moments_merge(None, 1, C.c_void_p(out.ctypes.data)) == Ec.E_INVALID
    assert lib.atsc_across_moments_merge(C.c_void_p(big.ctypes.data), 1, None) == Ec.E_INVALID
    assert lib.atsc_across_moments_merge(None, 0, None) == Ec.E_INVALID
    assert out.tobytes() == sent.tobytes()  # an error leaves the result as it was
    fits = np.array([(2 ** 31, 5, 1.0, 1.0), (2 ** 31 - 1, 2 ** 32 - 6, 1.0, 1.0)], dtype=M.dtype)  # 2^32 - 1 of each: fits
    got = A.across_moments_merge(fits)
    assert (got["count"], got["nans"]) == (2 ** 32 - 1, 2 ** 32 - 1)
    _assert_same(np.atleast_1d(got), M.merge_records([fits[:1], fits[1:]]), "large counts")


def test_fit_bit_for_bit(A):
    assert A.ACROSS_FIT == M.fit_dtype and A.ACROSS_FIT.itemsize == 40
    rng = np.random.default_rng(191)
    rows = [(0, 4, 1.0, 2.0), (0, 0, NAN, NAN), (1, 0, 7.25, 0.0), (1, 63, -3.0, 0.0), (2, 0, -3.5, 0.5), (2, 1, 1e9, 2e-6),
            (9, 0, INF, NAN), (9, 0, 1.0, INF), (3, 0, -INF, NAN), (64, 0, 0.1, 0.3), (6, 0, 1e-300, 1e-320), (5, 0, 3.0, -0.0),
            (2 ** 32 - 1, 0, 1.0, 3.0)]
    rows += [(int(n), int(64 - n), rng.normal(0, 1e3), abs(rng.normal(0, 1e3)) * n) for n in rng.integers(1, 65, 300)]
    m = np.array(rows, dtype=M.dtype)
    got, want = A.across_moments_fit(m), M.fit(m)
    assert got.dtype == A.ACROSS_FIT and len(got) == len(rows)
    for name in M.fit_dtype.names:
        g, w = got[name].copy(), want[name].copy()
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        assert g[~np.isnan(g)].tobytes() == w[~np.isnan(w)].tobytes(), name
    assert all(np.isnan(got[i][k]) for i in (0, 1) for k in M.fit_dtype.names)  # count == 0: all NaN whatever else is there
    for i in (2, 3):  # count == 1
        assert got[i]["variance"] == 0.0 and got[i]["stddev"] == 0.0 and np.isnan(got[i]["sample_variance"])
        assert np.isnan(got[i]["sample_stddev"]) and got[i]["mean"] == m[i]["mean"]
    assert got[4]["variance"] == 0.25 and got[4]["stddev"] == 0.5 and got[4]["sample_variance"] == 0.5
    assert len(A.across_moments_fit(np.zeros(0, dtype=M.dtype))) == 0
    lib = A.capi.lib()
    out = np.zeros(1, dtype=M.fit_dtype)
    assert lib.atsc_across_moments_fit(None, 1, C.c_void_p(out.ctypes.data)) == A.capi.E_INVALID
    assert lib.atsc_across_moments_fit(C.c_void_p(m.ctypes.data), 1, None) == A.capi.E_INVALID
    assert lib.atsc_across_moments_fit(None, 0, None) == 0


def test_symbols_are_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_across_moments_windows_dev", "atsc_across_moments_windows", "atsc_stream_across_moments_windows",
                 "atsc_across_moments_merge", "atsc_across_moments_fit"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name


def test_public_surfaces(A):
    want = {(A.Context, "across_moments_windows_host"): "(self, records_list, begins, counts, stride=1, has_count=False)",
            (A.DPlan, "across_moments_windows"): "(self, d_body, others, other_bodies, begins, counts, d_out, stride=1, stream=0)",
            (A.CompressedStream, "across_moments_windows"): "(self, others, begins, counts, stride=1)",
            (A.stream, "across_moments_data_windows"): "(ctx, bros, begins, counts, stride=1)",
            (A.engine, "across_moments_merge"): "(records)", (A.engine, "across_moments_fit"): "(moments)"}
    for (owner, name), sig in want.items():
        f = getattr(owner, name)
        assert str(inspect.signature(f)) == sig, name
        assert f.__doc__ and f.__doc__.strip()
    assert A.across_moments_data_windows is A.stream.across_moments_data_windows
    assert A.across_moments_merge is A.engine.across_moments_merge and A.across_moments_fit is A.engine.across_moments_fit


def test_null_context_is_invalid(A):
    lib = A.capi.lib()
    assert lib.atsc_across_moments_windows(None, 1, None, None, None, 0, None, None, 1, None) == A.capi.E_INVALID
    assert lib.atsc_across_moments_windows_dev(None, 1, None, None, 0, None, None, 1, None, None) == A.capi.E_INVALID
    assert lib.atsc_stream_across_moments_windows(None, 1, 0, None, None, 1, None) == A.capi.E_INVALID


def _run(argv):
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = "-1"  # exit 2 must come before any GPU work
    return subprocess.run(argv, capture_output=True, text=True, env=env, timeout=60)


def test_atsc_cli_argument_errors(A, tmp_path):
    f, other = str(tmp_path / "missing.bro"), str(tmp_path / "other.bro")
    across = ["-u", "--samples", "0:10", "--across", other]
    r = _run([ATSC, "-u", "--samples", "0:10", "--across-moments", f])  # the option without --across
    assert r.returncode == 2 and "'--across-moments' needs '--across'" in r.stderr, r.stderr
    r = _run([ATSC, "-u", "--across-moments", f])
    assert r.returncode == 2 and "error:" in r.stderr, r.stderr
    # --moments keeps its meaning: it needs --buckets, and --across does not go with --buckets
    r = _run([ATSC, *across, "--moments", f])
    assert r.returncode == 2 and "--buckets" in r.stderr, r.stderr
    r = _run([ATSC, "--help"])
    assert "--across-moments" in r.stdout + r.stderr and "nonnan,avg,stdvar,stddev" in r.stdout + r.stderr
    # a well-formed command line gets past the arguments (and fails on the missing file, not with a usage error)
    r = _run([ATSC, *across, "--across-stride", "3", "--across-quantiles", "0.5", "--across-extremes", "2", "--across-moments", f])
    assert r.returncode != 2, r.stderr
