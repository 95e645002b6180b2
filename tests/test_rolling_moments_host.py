"""The windowed rolling moments without a GPU: the NumPy model of the contract (tests/rolling_moments_model.py) -- its two
forms against each other, its count and its doubles against the windowed moments' model, its stated error bound against
exact rational arithmetic, exact zeros on a constant window, the all-NaN window, its independence of range and stride --
and the new symbols of the library."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import moments_model as MM
from tests import rolling_moments_model as M

WIDTHS = [1, 2, 3, 7, 8, 9, 64, 65, 300, 2049]
N = 9000


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


@pytest.fixture(scope="module")
def data():
    """mixed magnitudes, 1e-3 .. 1e5, both signs, with NaN holes, a stretch of NaN and a flat stretch"""
    rng = np.random.default_rng(41)
    x = rng.normal(0, 1, N) * 10.0 ** rng.integers(-3, 6, N)
    x[rng.random(N) < 0.03] = np.nan
    x[5000:5100] = np.nan
    x[7000:7050] = 4.25
    return x


def _sets():
    """the inputs the bound is stated on -> (name, x, org)"""
    rng = np.random.default_rng(43)
    holes = 0.01 * np.arange(N) + rng.normal(0, 1, N)
    holes[rng.random(N) < 0.3] = np.nan
    ramp = 0.25 * np.arange(N) + rng.normal(0, 3, N)
    return [("noise", rng.normal(0, 1, N), 0), ("offset1e9", 1e9 + rng.normal(0, 1e-3, N), 0), ("ramp", ramp, 0),
            ("ramp@2^30", ramp, 1 << 30), ("nan30", holes, 0), ("nan30@2^30", holes, 1 << 30),
            ("counter", np.cumsum(rng.integers(0, 51, N)).astype(np.float64), 0)]


def _positions(n, w, extra=()):
    rng = np.random.default_rng(3)
    lo = {0, 1, 7, 8, 2040, 2046, 2047, 2048, 2049, 4095, 4096, 4998, 4999, 5000, 5050, 5099, 6990, n - w} | set(extra)
    lo |= {int(v) for v in rng.integers(0, max(n - w, 1), 25)}
    return sorted(v for v in lo if 0 <= v <= n - w)


def _same(a, b):
    """count exactly; every double bit for bit, any NaN equal to any NaN"""
    if int(a[0]) != int(b[0]):
        return False
    return all((math.isnan(p) and math.isnan(q)) or np.float64(p).view(np.uint64) == np.float64(q).view(np.uint64)
               for p, q in zip(list(a)[1:], list(b)[1:]))


def test_the_two_forms_of_the_model_agree(data):
    x = data.copy()
    x[310:314] = [np.inf, -np.inf, 1.0, np.inf]
    for org in (0, 1 << 30):
        P = M.Pyramid(x, org)
        for w in WIDTHS:
            for s in (1, 7):
                b, c = [2040, 4990, 300, 0], [w + 20, w + 115, w + 14, w - 1]
                got, off = P.rolling(b, c, w, s)
                at = [lo for lo, _ in M.listed(b, c, w, s)]
                assert off.tolist() == [0, 20 // s + 1, 20 // s + 115 // s + 2, len(at), len(at)]
                for i, lo in enumerate(at):
                    assert _same(got[i], M.window_record(x, lo, w, org)), (org, lo, w, s)
            if org == 0:
                at = _positions(len(x), w)
                got = P.records(at, w)
                for i, lo in enumerate(at):
                    assert _same(got[i], M.window_record(x, lo, w)), (lo, w)


def test_count_is_the_windowed_moments_and_the_doubles_lie_within_both_bounds(data):
    """the windowed moments reduce the same window through another tree: the counts are equal, and where its value is not
    NaN each double lies within the sum of the two stated bounds of it (both taken around the exact value)"""
    P = M.Pyramid(data)
    for w in WIDTHS:
        lo = _positions(len(data), w)
        got = P.records(lo, w)
        for i, b in enumerate(lo):
            ref = MM.window_moments(data, b, w)
            assert int(got[i]["count"]) == ref[0], (b, w)
            if ref[0] == 0:
                assert all(math.isnan(got[i][k]) for k in M.FIELDS[1:])
                continue
            en, emean, em2, _, et_m2, _, eabs = MM.exact_moments(data[b:b + w])
            r = (b + w) / w
            mine, theirs = M.bounds(w, en, emean, em2, et_m2), MM.bounds(en, emean, em2, et_m2)
            lims = {"mean": (mine[0] + theirs[0]) * float(eabs), "m2": mine[1] + theirs[1],
                    "t_mean": (mine[0] + theirs[0]) * (b + w), "t_m2": r * (mine[2] + theirs[2]),
                    "c_tx": r * (mine[3] + theirs[3])}
            for j, k in enumerate(M.FIELDS[1:]):
                assert abs(float(got[i][k]) - ref[1 + j]) <= lims[k], (b, w, k, got[i][k], ref[1 + j], lims[k])


def test_model_within_the_stated_bound_of_exact():
    """(3 L + 2) u times mean|x|, kappa m2, r t_m2, r kappa sqrt(t_m2 m2) and lo + w, against exact rational arithmetic:
    the check that pins the header's constant"""
    worst = {}
    for name, x, org in _sets():
        P = M.Pyramid(x, org)
        for w in (2, 3, 7, 8, 9, 64, 65, 300, 2049, 3600):
            lo = [v for v in (0, 1, 777, 2047, 4000, 4999, N - w) if 0 <= v <= N - w]
            got = P.records(lo, w)
            for i, b in enumerate(lo):
                en, emean, em2, et_mean, et_m2, ec_tx, eabs = MM.exact_moments(x[b:b + w])
                assert int(got[i]["count"]) == en, (name, b, w)
                if en == 0:
                    continue
                k, b_m2, b_tm2, b_c = M.bounds(w, en, emean, em2, et_m2)
                at = org + b
                r = (at + w) / w
                errs = {"mean": (abs(Fraction(float(got[i]["mean"])) - emean), k * float(eabs)),
                        "m2": (abs(Fraction(float(got[i]["m2"])) - em2), b_m2),
                        "t_mean": (abs(Fraction(float(got[i]["t_mean"])) - et_mean), k * (at + w)),
                        "t_m2": (abs(Fraction(float(got[i]["t_m2"])) - et_m2), r * b_tm2),
                        "c_tx": (abs(Fraction(float(got[i]["c_tx"])) - ec_tx), r * b_c)}
                for what, (e, lim) in errs.items():
                    assert float(e) <= lim, (name, b, w, what, float(e), lim)
                    if lim > 0:
                        worst[what] = max(worst.get(what, 0.0), float(e) / lim)
                if name == "offset1e9" and w >= 300:  # the variance keeps its digits: sigma^2 = 1e-6, as sampled
                    assert abs(float(got[i]["m2"]) / en - 1e-6) < 0.5e-6, (b, w, got[i]["m2"] / en)
    print("largest error / bound:", worst)
    assert 0.0 < max(worst.values()) < 1.0


def test_constant_window_has_no_spread_and_no_trend_exactly(data):
    P = M.Pyramid(data)
    for w in (1, 2, 3, 7, 8, 9, 50):
        for lo in sorted({7000, min(7001, 7050 - w), 7050 - w}):
            r = P.records([lo], w)[0]
            assert r["count"] == w and r["mean"] == 4.25 and r["m2"] == 0.0 and r["c_tx"] == 0.0, (lo, w)
            assert _same(r, M.window_record(data, lo, w))
    x = np.full(5000, 1234.5678)
    got = M.Pyramid(x).records([0, 1, 1023, 2047], 2049)
    assert np.all(got["m2"] == 0.0) and np.all(got["c_tx"] == 0.0) and np.all(got["mean"] == 1234.5678)
    assert np.all(got["t_m2"] > 0.0)


def test_all_nan_window_is_count_zero_and_five_nans(data):
    P = M.Pyramid(data)
    for lo, w in ((5000, 100), (5001, 64), (5010, 7), (5099, 1)):
        r = P.records([lo], w)[0]
        assert r["count"] == 0 and all(math.isnan(r[k]) for k in M.FIELDS[1:]), (lo, w)
        lit = M.window_record(data, lo, w)
        assert lit[0] == 0 and all(math.isnan(v) for v in lit[1:])


def test_a_position_does_not_depend_on_range_or_stride(data):
    P = M.Pyramid(data)
    for w in (2, 3, 64, 65, 300, 2049):
        a, off_a = P.rolling([0], [len(data)], w, 1)
        assert int(off_a[1]) == len(data) - w + 1
        for begin, stride in ((1, 7), (5, w), (12, 2 * w + 1), (2048, 3)):
            b, off_b = P.rolling([begin, 100], [len(data) - begin, 50 + w], w, stride)
            lo = begin + stride * np.arange(int(off_b[1]))
            assert a[lo].tobytes() == b[: len(lo)].tobytes(), (w, begin, stride)
            lo2 = 100 + stride * np.arange(int(off_b[2] - off_b[1]))
            assert a[lo2].tobytes() == b[len(lo):].tobytes(), (w, begin, stride)


def test_symbols_and_surfaces(A):
    lib = A.capi.lib()
    for name in ("atsc_rolling_moments_windows_dev", "atsc_rolling_moments_windows", "atsc_stream_rolling_moments_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert A.WINDOW_MOMENTS.itemsize == 48 and A.WINDOW_MOMENTS.names == M.FIELDS and M.RECORD == A.WINDOW_MOMENTS
    for owner, name in ((A.Context, "rolling_moments_windows_host"), (A.DPlan, "rolling_moments_windows"),
                        (A.CompressedStream, "rolling_moments_windows"), (A, "rolling_moments_data_windows")):
        assert getattr(owner, name).__doc__.strip()
