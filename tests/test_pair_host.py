"""CPU-only tests of the windowed pair moments' host half: the NumPy model of the documented merge tree
(tests/pair_model.py) against exact rational arithmetic and against numpy.cov / numpy.corrcoef / numpy.polyfit within the
documented (L + 2) bounds, atsc_pair_fit bit for bit against its Python restatement, the new symbols and dtypes, and the
command line's usage errors."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import pair_model as P

LENGTHS = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 2047, 2048, 2049, 4096, 5000, 12289, 40000]
BEGINS = [1, 1000, 2047, 2048, 12345, 3 * 2048 - 1, 1000003]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _inputs(rng, n):
    """(x, y) pairs: independent N(0, 1); y a noisy line of x; both at 1e6 + N(0, 1), correlated; both at 1e9 +- 1e-3,
    correlated; a ramp against a random walk; a constant against noise; anticorrelated; 20 % NaN in each, independently"""
    x = rng.normal(0, 1, n)
    e = rng.normal(0, 1, n)
    hx, hy = rng.normal(0, 1, n), rng.normal(3, 2, n)
    hx[rng.random(n) < 0.2] = np.nan
    hy[rng.random(n) < 0.2] = np.nan
    s = rng.normal(0, 1e-3, n)
    return {"independent": (x, e), "line": (x, 2.5 * x - 7.0 + 0.1 * e),
            "offset1e6": (1e6 + x, 1e6 + 0.5 * x + 0.5 * e),
            "offset1e9": (1e9 + s, 1e9 + 0.7 * s + 0.3 * rng.normal(0, 1e-3, n)),
            "ramp_walk": (0.25 * np.arange(n) + 3 * x, np.cumsum(e)), "constant": (np.full(n, 1234.5678), e),
            "anti": (x, -x), "nan20": (hx, hy)}


def _cases():
    """every length and input with the window at the stream's start and at a begin further in"""
    rng = np.random.default_rng(161)
    for k, n in enumerate(LENGTHS):
        for begin in (0, BEGINS[k % len(BEGINS)]):
            for name, (vx, vy) in _inputs(rng, n).items():
                # the outside must not matter
                x = np.concatenate([np.full(begin, 1e300), vx, rng.normal(-5, 100, 7)])
                y = np.concatenate([np.full(begin, -1e300), vy, rng.normal(5, 100, 7)])
                yield name, begin, n, x, y


def _bits(x):
    return np.float64(x).view(np.uint64)


def _F(v):
    return Fraction(float(v))


def test_model_within_bounds_of_exact():
    worst = {}
    for name, begin, count, x, y in _cases():
        n, mx, m2x, my, m2y, c = P.window_pair(x, y, begin, count)
        en, emx, em2x, emy, em2y, ec, eax, eay = P.exact_pair(x[begin:begin + count], y[begin:begin + count])
        assert n == en, (name, begin, count)
        if en == 0:
            assert all(math.isnan(q) for q in (mx, m2x, my, m2y, c))
            continue
        k, b_m2x, b_m2y, b_c = P.bounds(en, emx, em2x, emy, em2y)
        errs = (abs(_F(mx) - emx), abs(_F(my) - emy), abs(_F(m2x) - em2x), abs(_F(m2y) - em2y), abs(_F(c) - ec))
        lims = (k * float(eax), k * float(eay), b_m2x, b_m2y, b_c)
        for what, e, lim in zip(("mean_x", "mean_y", "m2_x", "m2_y", "c_xy"), errs, lims):
            assert float(e) <= lim, (name, begin, count, what, float(e), lim)
            if lim > 0:
                worst[what] = max(worst.get(what, 0.0), float(e) / lim)
        if em2x == 0:  # x constant over the counted samples: no spread and no co-moment, exactly
            assert m2x == 0.0 and c == 0.0, (name, begin, count)
        if em2y == 0:
            assert m2y == 0.0 and c == 0.0, (name, begin, count)
    print("largest error / bound:", worst)


def test_model_against_numpy_cov_corrcoef_polyfit():
    """numpy's two-pass forms carry rounding of their own, of the same order: both sides are held to the documented
    bounds around each other, propagated through the fit -- covariance: b_c / n; correlation = c / sqrt(m2_x m2_y):
    b_c / sqrt(m2_x m2_y) + |corr| (b_m2x / m2_x + b_m2y / m2_y) / 2; slope = c / m2_x: b_c / m2_x + |slope| b_m2x / m2_x;
    intercept = mean_y - slope mean_x: b_mean_y + (slope's bound) |mean_x| + |slope| b_mean_x -- each doubled for NumPy's
    share, which centres on its own rounded means: (b_mean_x)(b_mean_y) more on the covariance."""
    for name, begin, count, x, y in _cases():
        vx, vy = x[begin:begin + count], y[begin:begin + count]
        if count < 2 or np.isnan(vx).any() or np.isnan(vy).any():
            continue
        rec = P.window_pair(x, y, begin, count)
        cov, scov, corr, slope, icpt, r2, _ = P.fit(*rec)
        en, emx, em2x, emy, em2y, ec, eax, eay = P.exact_pair(vx, vy)
        k, b_m2x, b_m2y, b_c = P.bounds(en, emx, em2x, emy, em2y)
        fx, fy = float(em2x), float(em2y)
        want = np.cov(vx, vy, bias=True)[0, 1]
        assert abs(cov - want) <= 2 * b_c / en + (k * float(eax)) * (k * float(eay)) + 4 * P.U * abs(cov), (name, begin, count)
        assert abs(scov - np.cov(vx, vy)[0, 1]) <= (2 * b_c + 4 * P.U * abs(rec[5])) / (en - 1) + (k * float(eax)) * (
            k * float(eay)), (name, begin, count)
        if fx == 0 or fy == 0:
            assert math.isnan(corr) and (fx > 0 or math.isnan(slope)), (name, begin, count)
            continue
        b_corr = b_c / math.sqrt(fx * fy) + abs(corr) * (b_m2x / fx + b_m2y / fy) / 2
        assert abs(corr - np.corrcoef(vx, vy)[0, 1]) <= 2 * b_corr + 8 * P.U, (name, begin, count, corr)
        assert -1.0 <= corr <= 1.0 and _bits(r2) == _bits(corr * corr)
        if name.startswith("offset"):  # polyfit does not centre x: at kappa_x of 1e6 and more it keeps no digit to compare
            continue
        p1, p0 = np.polyfit(vx, vy, 1)
        b_slope = b_c / fx + abs(slope) * b_m2x / fx
        # polyfit solves a scaled least-squares system: its own error grows with the condition of x, kappa_x^2
        kx2 = 1.0 + en * float(emx) ** 2 / fx
        ulp = 64 * P.U * kx2
        assert abs(slope - p1) <= 2 * b_slope + ulp * max(abs(slope), math.sqrt(fy / fx)), (name, begin, count, slope, p1)
        b_icpt = k * float(eay) + b_slope * abs(float(emx)) + abs(slope) * k * float(eax)
        assert abs(icpt - p0) <= 2 * b_icpt + ulp * (abs(icpt) + max(abs(slope), math.sqrt(fy / fx)) * abs(float(emx))), (
            name, begin, count, icpt, p0)


def test_model_keeps_the_covariance_at_1e9():
    """two series at 1e9 +- 1e-3: sums of products would lose every digit (1e18 against 1e-6 per term); the centred
    merge keeps the covariance to the documented bound, far inside 1e-3 of its size"""
    rng = np.random.default_rng(167)
    n = 30000
    s = rng.normal(0, 1e-3, n)
    x, y = 1e9 + s, 1e9 + 0.8 * s + 0.6 * rng.normal(0, 1e-3, n)
    rec = P.window_pair(x, y, 0, n)
    en, emx, em2x, emy, em2y, ec, _, _ = P.exact_pair(x, y)
    _, _, _, b_c = P.bounds(en, emx, em2x, emy, em2y)
    assert abs(_F(rec[5]) - ec) <= b_c
    assert abs(float(_F(rec[5]) - ec)) <= 1e-3 * abs(float(ec))
    cov, _, corr, slope, _, _, _ = P.fit(*rec)
    assert abs(cov - float(ec) / n) <= 1e-3 * abs(float(ec) / n)
    assert abs(corr - float(ec) / math.sqrt(float(em2x) * float(em2y))) < 1e-3
    naive = float(np.sum(x * y) / n - np.mean(x) * np.mean(y))  # what the centred form is there to avoid
    assert abs(naive - float(ec) / n) > 100 * abs(cov - float(ec) / n)


def test_model_ignores_what_lies_outside_the_window():
    rng = np.random.default_rng(173)
    x, y = rng.normal(0, 1, 9000), rng.normal(0, 1, 9000)
    x2, y2 = x.copy(), y.copy()
    x2[:1000] = 1e300
    y2[3000:] = np.nan
    a, b = P.window_pair(x, y, 1000, 2000), P.window_pair(x2, y2, 1000, 2000)
    assert [_bits(q) for q in a[1:]] == [_bits(q) for q in b[1:]] and a[0] == b[0] == 2000
    e = P.window_pair(x, y, 5, 0)
    assert e[0] == 0 and all(math.isnan(q) for q in e[1:])


def test_model_nan_in_either_input_drops_the_sample():
    rng = np.random.default_rng(179)
    n = 5000
    x, y = rng.normal(0, 1, n), rng.normal(0, 1, n)
    nx, ny = rng.random(n) < 0.1, rng.random(n) < 0.1
    xh, yh = np.where(nx, np.nan, x), np.where(ny, np.nan, y)
    rec = P.window_pair(xh, yh, 100, 4500)
    drop = (nx | ny)[100:4600]
    assert rec[0] == int((~drop).sum()) < 4500 - int(nx[100:4600].sum())
    # the same record as with NaN in both inputs wherever either has one: only the counted slots' values are read
    both = P.window_pair(np.where(nx | ny, np.nan, x), np.where(nx | ny, np.nan, y), 100, 4500)
    assert rec[0] == both[0] and [_bits(q) for q in rec[1:]] == [_bits(q) for q in both[1:]]
    en, emx, em2x, emy, em2y, ec, _, _ = P.exact_pair(xh[100:4600], yh[100:4600])
    k, b_m2x, b_m2y, b_c = P.bounds(en, emx, em2x, emy, em2y)
    assert en == rec[0] and abs(_F(rec[5]) - ec) <= b_c and abs(_F(rec[2]) - em2x) <= b_m2x
    allnan = P.window_pair(np.full(n, np.nan), y, 0, n)
    assert allnan[0] == 0 and all(math.isnan(q) for q in allnan[1:])
    # swapped inputs: swapped fields; the same input twice: the moments' mean and m2
    s = P.window_pair(yh, xh, 100, 4500)
    assert s[0] == rec[0] and [_bits(q) for q in s[1:]] == [_bits(rec[i]) for i in (3, 4, 1, 2, 5)]
    from tests import moments_model as M

    xx, mm = P.window_pair(xh, xh, 100, 4500), M.window_moments(xh, 100, 4500)
    assert xx[0] == mm[0] and _bits(xx[1]) == _bits(xx[3]) == _bits(mm[1])
    assert _bits(xx[2]) == _bits(xx[4]) == _bits(xx[5]) == _bits(mm[2])


def test_pair_dtypes(A):
    assert A.WINDOW_PAIR.itemsize == 48
    assert A.WINDOW_PAIR.names == P.FIELDS
    assert A.WINDOW_PAIR_FIT.itemsize == 56
    assert A.WINDOW_PAIR_FIT.names == P.FIT_FIELDS


def test_symbols_exported_and_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_pair_windows_dev", "atsc_pair_windows", "atsc_stream_pair_windows", "atsc_pair_fit"):
        assert name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert callable(A.Context.pair_windows_host) and callable(A.DPlan.pair_windows)
    assert callable(A.CompressedStream.pair_windows) and callable(A.pair_fit)


def test_pair_fit_bit_for_bit(A):
    rng = np.random.default_rng(181)
    inf, nan = float("inf"), float("nan")
    above = np.nextafter(1.0, 2.0)
    rows = [(0, 1.0, 2.0, 3.0, 4.0, 5.0), (0, nan, nan, nan, nan, nan), (1, 7.25, 0.0, -3.0, 0.0, 0.0),
            (2, -3.5, 0.5, 2.0, 2.0, -1.0), (2, 1e9, 2e-6, 1e9, 2e-6, 2e-6), (5, 3.0, 0.0, 2.0, 10.0, 0.0),
            (5, 3.0, 10.0, 2.0, 0.0, 0.0), (5, 3.0, 0.0, 2.0, 0.0, 0.0), (5, 3.0, -0.0, 2.0, 4.0, 1.0),
            # correlations that would round above 1 or below -1: c_xy a hair past sqrt(m2_x m2_y)
            (9, 1.0, 4.0, 2.0, 9.0, 6.0 * above), (9, 1.0, 4.0, 2.0, 9.0, -6.0 * above), (9, 1.0, 3.0, 2.0, 3.0, 3.0 * above),
            (7, 0.1, 0.3, 0.7, 0.3, 0.3), (7, 0.1, 0.3, 0.7, 0.3, 0.30000000000000004), (7, 0.1, 0.3, 0.7, 0.3, -0.31),
            (9, inf, nan, 4.0, 60.0, nan), (9, 1.0, inf, 4.0, 60.0, inf), (9, 1.0, 2.0, -inf, nan, -inf),
            (3, 1.0, 2.0, 1.0, 2.0, inf), (4, 0.1, 0.3, 1.5, 5.0, 0.7), (2 ** 53 + 2, 0.1, 0.3, 1.5, 5.0, 0.7),
            (7, 1.0, 2.0, 3.0, nan, 1.0), (6, 1e-300, 1e-320, 2.5, 17.5, 1e-310), (6, 1e300, 1e300, 1e300, 1e300, 1e300)]
    for _ in range(300):
        n = int(rng.integers(1, 100000))
        m2x, m2y = abs(rng.normal(0, 1e3)) * n, abs(rng.normal(0, 1e3)) * n
        rows.append((n, rng.normal(0, 1e3), m2x, rng.normal(0, 1e3), m2y, float(np.sqrt(m2x * m2y)) * rng.uniform(-1.0, 1.0)))
    m = np.zeros(len(rows), dtype=A.WINDOW_PAIR)
    for i, r in enumerate(rows):
        m[i] = r
    got = A.pair_fit(m)
    assert got.dtype == A.WINDOW_PAIR_FIT and len(got) == len(rows)
    for r, g in zip(rows, got):
        want = P.fit(*r)
        for name, w in zip(A.WINDOW_PAIR_FIT.names, want):
            assert (np.isnan(w) and np.isnan(g[name])) or _bits(w) == _bits(g[name]), (r, name, w, g[name])
    assert all(np.isnan(got[0][k]) for k in A.WINDOW_PAIR_FIT.names)  # count == 0: all NaN whatever the other fields hold
    assert all(np.isnan(got[1][k]) for k in A.WINDOW_PAIR_FIT.names)
    g = got[2]  # count == 1
    assert g["covariance"] == 0.0 and np.isnan(g["sample_covariance"]) and np.isnan(g["correlation"]) and np.isnan(g["slope"])
    assert np.isnan(g["intercept"]) and np.isnan(g["r2"]) and g["mean_diff"] == 10.25
    g = got[3]  # count == 2
    assert g["covariance"] == -0.5 and g["sample_covariance"] == -1.0 and g["slope"] == -2.0
    assert abs(g["correlation"] + 1.0) <= 2 * P.U and g["intercept"] == -5.0 and g["mean_diff"] == -5.5
    # zero variance: in x -- no correlation, no slope, no intercept; in y only -- slope 0 and the mean as intercept
    assert np.isnan(got[5]["correlation"]) and np.isnan(got[5]["slope"]) and np.isnan(got[5]["intercept"])
    assert np.isnan(got[6]["correlation"]) and got[6]["slope"] == 0.0 and got[6]["intercept"] == 2.0 and np.isnan(got[6]["r2"])
    assert np.isnan(got[7]["correlation"]) and np.isnan(got[7]["slope"]) and got[7]["covariance"] == 0.0
    assert np.isnan(got[8]["correlation"]) and np.isnan(got[8]["slope"])  # m2_x == -0.0 is not > 0
    # the clamp
    assert got[9]["correlation"] == 1.0 and got[10]["correlation"] == -1.0 and got[11]["correlation"] == 1.0
    assert got[9]["r2"] == 1.0 and (6.0 * above / 2.0) / 3.0 > 1.0
    assert got[14]["correlation"] == -1.0
    assert len(A.pair_fit(np.zeros(0, dtype=A.WINDOW_PAIR))) == 0
    lib = A.capi.lib()
    out = np.zeros(1, dtype=A.WINDOW_PAIR_FIT)
    assert lib.atsc_pair_fit(None, 1, C.c_void_p(out.ctypes.data)) == A.capi.E_INVALID
    assert lib.atsc_pair_fit(C.c_void_p(m.ctypes.data), 1, None) == A.capi.E_INVALID
    assert lib.atsc_pair_fit(None, 0, None) == 0


def test_command_line_usage_errors(A, tmp_path):
    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    f = tmp_path / "x.bro"
    f.write_bytes(b"")
    g = tmp_path / "y.bro"
    g.write_bytes(b"")
    for cmd in ([atsc, "-u", "--pair", str(g), str(f)], [atsc, "--pair", str(g), str(f)],
                [atsc, "-u", "--samples", "0:10", "--pair", str(g), str(f)], [atsc, "--buckets", "5", "--pair", str(g), str(f)],
                [atsc, "-u", "--buckets", "5", "--pair=", str(f)],
                # csv-compressor does not take the option
                [csvc, "-u", "--from", "0", "--to", "10", "--step", "5", "--pair", str(g), str(f)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (cmd, r.stderr)
        assert "error:" in r.stderr, cmd
    r = subprocess.run([atsc, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--pair" in r.stderr and "pair_count" in r.stderr
    r = subprocess.run([csvc, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--pair" not in r.stderr
