"""The windowed rolling pair moments without a GPU: the NumPy model of the contract (tests/rolling_pair_model.py) -- its
two forms against each other, its count and its doubles against the windowed pair moments' model, its stated error bound
against exact rational arithmetic, the swap of x and y, y = x against the rolling moments' model, exact zeros on a constant
x, the window without a counted slot, its independence of range and stride -- and the new symbols of the library."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import pair_model as PM
from tests import rolling_moments_model as RM
from tests import rolling_pair_model as M

WIDTHS = [1, 2, 3, 7, 8, 9, 64, 65, 300, 2049]
BOUND_WIDTHS = [2, 3, 7, 8, 9, 64, 65, 300, 2049, 3600]
N = 9000
SWAP = ("count", "mean_y", "m2_y", "mean_x", "m2_x", "c_xy")


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


@pytest.fixture(scope="module")
def data():
    """two series of mixed magnitudes, 1e-3 .. 1e5, both signs, with NaN holes in different places, a stretch of NaN in
    x, one in y that overlaps it in part, interleaved holes (every slot NaN in one stream or the other) and a flat
    stretch of x"""
    rng = np.random.default_rng(47)
    x = rng.normal(0, 1, N) * 10.0 ** rng.integers(-3, 6, N)
    y = 0.5 * x + rng.normal(0, 1, N) * 10.0 ** rng.integers(-3, 6, N)
    x[rng.random(N) < 0.03] = np.nan
    y[rng.random(N) < 0.03] = np.nan
    x[5000:5100] = np.nan
    y[5060:5160] = np.nan
    x[6000:6100:2] = np.nan
    y[6001:6100:2] = np.nan
    x[7000:7050] = 4.25
    y[7000:7050] = rng.normal(0, 1, 50)
    return x, y


def _sets():
    """the inputs the bound is stated on -> (name, x, y)"""
    rng = np.random.default_rng(53)
    ramp = 0.25 * np.arange(N) + rng.normal(0, 3, N)
    holes = 0.01 * np.arange(N) + rng.normal(0, 1, N)
    holes[rng.random(N) < 0.3] = np.nan

    def mixed():
        return np.round(rng.normal(0, 1, N) * 10.0 ** rng.integers(3, 18, N))

    return [("noise/noise", rng.normal(0, 1, N), rng.normal(0, 1, N)),
            ("offset1e9/offset1e9", 1e9 + rng.normal(0, 1e-3, N), 1e9 + rng.normal(0, 1e-3, N)),
            ("ramp/noise", ramp, rng.normal(0, 1, N)),
            ("ramp/-2ramp+noise", ramp, -2.0 * ramp + rng.normal(0, 1, N)),
            ("nan30/ramp", holes, ramp),
            ("counter/noise", np.cumsum(rng.integers(0, 51, N)).astype(np.float64), rng.normal(0, 1, N)),
            ("mixed/mixed", mixed(), mixed())]


def _positions(n, w, extra=()):
    rng = np.random.default_rng(3)
    lo = {0, 1, 7, 8, 2040, 2046, 2047, 2048, 2049, 4095, 4096, 4998, 4999, 5000, 5050, 5099, 5999, 6990, n - w} | set(extra)
    lo |= {int(v) for v in rng.integers(0, max(n - w, 1), 25)}
    return sorted(v for v in lo if 0 <= v <= n - w)


def _same(a, b):
    """count exactly; every double bit for bit, any NaN equal to any NaN"""
    if int(a[0]) != int(b[0]):
        return False
    return all((math.isnan(p) and math.isnan(q)) or np.float64(p).view(np.uint64) == np.float64(q).view(np.uint64)
               for p, q in zip(list(a)[1:], list(b)[1:]))


def test_the_two_forms_of_the_model_agree(data):
    x, y = data[0].copy(), data[1].copy()
    x[310:314] = [np.inf, -np.inf, 1.0, np.inf]
    y[312:316] = [np.inf, 2.0, -np.inf, 3.0]
    for org in (0, 1 << 30):
        P = M.Pyramid(x, y, org)
        for w in WIDTHS:
            for s in (1, 7):
                b, c = [2040, 4990, 300, 0], [w + 20, w + 115, w + 14, w - 1]
                got, off = P.rolling(b, c, w, s)
                at = [lo for lo, _ in M.listed(b, c, w, s)]
                assert off.tolist() == [0, 20 // s + 1, 20 // s + 115 // s + 2, len(at), len(at)]
                for i, lo in enumerate(at):
                    assert _same(got[i], M.window_record(x, y, lo, w, org)), (org, lo, w, s)
            if org == 0:
                at = _positions(len(x), w)
                got = P.records(at, w)
                for i, lo in enumerate(at):
                    assert _same(got[i], M.window_record(x, y, lo, w)), (lo, w)


def test_count_is_the_windowed_pair_and_the_doubles_lie_within_both_bounds(data):
    """the windowed pair moments reduce the same window through another tree: the counts are equal, and each double lies
    within the sum of the two stated bounds of it (both taken around the exact value)"""
    x, y = data
    P = M.Pyramid(x, y)
    for w in WIDTHS:
        lo = _positions(N, w)
        got = P.records(lo, w)
        for i, b in enumerate(lo):
            ref = PM.window_pair(x, y, b, w)
            assert int(got[i]["count"]) == ref[0], (b, w)
            if ref[0] == 0:
                assert all(math.isnan(got[i][k]) for k in M.FIELDS[1:])
                continue
            en, emx, em2x, emy, em2y, _, eax, eay = PM.exact_pair(x[b:b + w], y[b:b + w])
            mine, theirs = M.bounds(w, en, emx, em2x, emy, em2y), PM.bounds(en, emx, em2x, emy, em2y)
            lims = {"mean_x": (mine[0] + theirs[0]) * float(eax), "m2_x": mine[1] + theirs[1],
                    "mean_y": (mine[0] + theirs[0]) * float(eay), "m2_y": mine[2] + theirs[2], "c_xy": mine[3] + theirs[3]}
            for j, k in enumerate(M.FIELDS[1:]):
                assert abs(float(got[i][k]) - ref[1 + j]) <= lims[k], (b, w, k, got[i][k], ref[1 + j], lims[k])


def test_model_within_the_stated_bound_of_exact():
    """(3 L + 2) u times mean|x|, kappa_x m2_x (and for y) and kappa_x kappa_y sqrt(m2_x m2_y), against exact rational
    arithmetic: the check that pins the header's constant"""
    worst = {}
    for name, x, y in _sets():
        P = M.Pyramid(x, y)
        for w in BOUND_WIDTHS:
            lo = [v for v in (0, 1, 777, 2047, 4000, 4999, N - w) if 0 <= v <= N - w]
            got = P.records(lo, w)
            for i, b in enumerate(lo):
                en, emx, em2x, emy, em2y, ec, eax, eay = PM.exact_pair(x[b:b + w], y[b:b + w])
                assert int(got[i]["count"]) == en, (name, b, w)
                if en == 0:
                    continue
                k, b_m2x, b_m2y, b_c = M.bounds(w, en, emx, em2x, emy, em2y)
                errs = {"mean_x": (abs(Fraction(float(got[i]["mean_x"])) - emx), k * float(eax)),
                        "m2_x": (abs(Fraction(float(got[i]["m2_x"])) - em2x), b_m2x),
                        "mean_y": (abs(Fraction(float(got[i]["mean_y"])) - emy), k * float(eay)),
                        "m2_y": (abs(Fraction(float(got[i]["m2_y"])) - em2y), b_m2y),
                        "c_xy": (abs(Fraction(float(got[i]["c_xy"])) - ec), b_c)}
                for what, (e, lim) in errs.items():
                    assert float(e) <= lim, (name, b, w, what, float(e), lim)
                    if lim > 0:
                        worst[what] = max(worst.get(what, 0.0), float(e) / lim)
                if name.startswith("offset1e9") and w >= 300:
                    # the variances and the covariance keep their digits: sigma_x = sigma_y = 1e-3, as sampled, so both
                    # variances are 1e-6 and the covariance is some fraction of sigma_x sigma_y = 1e-6; a sum of raw
                    # products at 1e9 would be wrong by some 1e18 u = 1e2.  As the rolling moments' check of the same
                    # set: each within half of sigma^2
                    assert abs(float(got[i]["m2_x"]) / en - 1e-6) < 0.5e-6 and abs(float(got[i]["m2_y"]) / en - 1e-6) < 0.5e-6
                    assert abs(float(got[i]["c_xy"]) / en - float(ec) / en) < 0.5e-6, (b, w, got[i]["c_xy"] / en)
    print("largest error / bound:", worst)
    assert set(worst) == set(M.FIELDS[1:])
    assert 0.0 < max(worst.values()) < 1.0


def test_swapping_x_and_y_swaps_the_fields_bit_for_bit(data):
    x, y = data
    P, Q = M.Pyramid(x, y), M.Pyramid(y, x)
    for w in WIDTHS:
        lo = _positions(N, w)
        a, b = P.records(lo, w), Q.records(lo, w)
        for i in range(len(lo)):
            assert _same(tuple(a[i][k] for k in M.FIELDS), tuple(b[i][k] for k in SWAP)), (lo[i], w)


def test_y_equal_to_x_is_the_rolling_moments_count_mean_and_m2(data):
    x = data[0]
    P, Q = M.Pyramid(x, x), RM.Pyramid(x)
    for w in WIDTHS:
        lo = _positions(N, w)
        a, b = P.records(lo, w), Q.records(lo, w)
        for i in range(len(lo)):
            assert _same((a[i]["count"], a[i]["mean_x"], a[i]["m2_x"]), (b[i]["count"], b[i]["mean"], b[i]["m2"])), (lo[i], w)
            assert _same((a[i]["count"], a[i]["mean_y"], a[i]["m2_y"], a[i]["c_xy"]),
                         (a[i]["count"], a[i]["mean_x"], a[i]["m2_x"], a[i]["m2_x"])), (lo[i], w)


def test_constant_x_has_no_spread_and_no_co_moment_exactly(data):
    x, y = data
    P = M.Pyramid(x, y)
    for w in (1, 2, 3, 7, 8, 9, 50):
        for lo in sorted({7000, min(7001, 7050 - w), 7050 - w}):
            r = P.records([lo], w)[0]
            assert r["count"] == w and r["mean_x"] == 4.25 and r["m2_x"] == 0.0 and r["c_xy"] == 0.0, (lo, w)
            assert w == 1 or r["m2_y"] > 0.0
            assert _same(r, M.window_record(x, y, lo, w))
    rng = np.random.default_rng(5)
    got = M.Pyramid(np.full(5000, 1234.5678), rng.normal(0, 1, 5000)).records([0, 1, 1023, 2047], 2049)
    assert np.all(got["m2_x"] == 0.0) and np.all(got["c_xy"] == 0.0) and np.all(got["mean_x"] == 1234.5678)
    assert np.all(got["m2_y"] > 0.0)


def test_window_without_a_counted_slot_is_count_zero_and_five_nans(data):
    """NaN in x alone, in both, and interleaved so that every slot has a NaN in one stream or the other"""
    x, y = data
    assert not np.all(np.isnan(x[6000:6100])) and not np.all(np.isnan(y[6000:6100]))
    P = M.Pyramid(x, y)
    for lo, w in ((5000, 100), (5001, 64), (5010, 7), (5099, 1), (5060, 40), (5100, 60), (6000, 100), (6001, 64), (6003, 7)):
        r = P.records([lo], w)[0]
        assert r["count"] == 0 and all(math.isnan(r[k]) for k in M.FIELDS[1:]), (lo, w)
        lit = M.window_record(x, y, lo, w)
        assert lit[0] == 0 and all(math.isnan(v) for v in lit[1:])


def test_a_position_does_not_depend_on_range_or_stride(data):
    x, y = data
    P = M.Pyramid(x, y)
    for w in (2, 3, 64, 65, 300, 2049):
        a, off_a = P.rolling([0], [N], w, 1)
        assert int(off_a[1]) == N - w + 1
        for begin, stride in ((1, 7), (5, w), (12, 2 * w + 1), (2048, 3)):
            b, off_b = P.rolling([begin, 100], [N - begin, 50 + w], w, stride)
            lo = begin + stride * np.arange(int(off_b[1]))
            assert a[lo].tobytes() == b[: len(lo)].tobytes(), (w, begin, stride)
            lo2 = 100 + stride * np.arange(int(off_b[2] - off_b[1]))
            assert a[lo2].tobytes() == b[len(lo):].tobytes(), (w, begin, stride)


def test_symbols_and_surfaces(A):
    lib = A.capi.lib()
    for name in ("atsc_rolling_pair_windows_dev", "atsc_rolling_pair_windows", "atsc_stream_rolling_pair_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert A.WINDOW_PAIR.itemsize == 48 and A.WINDOW_PAIR.names == M.FIELDS and M.RECORD == A.WINDOW_PAIR
    for owner, name in ((A.Context, "rolling_pair_windows_host"), (A.DPlan, "rolling_pair_windows"),
                        (A.CompressedStream, "rolling_pair_windows"), (A, "rolling_pair_data_windows")):
        assert getattr(owner, name).__doc__.strip()
