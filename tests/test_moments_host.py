"""CPU-only tests of the windowed moments' host half: the NumPy model of the documented merge tree
(tests/moments_model.py) against exact rational arithmetic and against numpy.var / numpy.polyfit within the documented
(L + 2) bounds, atsc_moments_fit bit for bit against its Python restatement, the new symbols, and the command lines'
usage errors."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import moments_model as M

LENGTHS = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 2047, 2048, 2049, 4096, 5000, 12289, 40000]
BEGINS = [1, 1000, 2047, 2048, 12345, 3 * 2048 - 1, 1000003]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _inputs(rng, n):
    """the inputs the bounds were stated on: N(0, 1); 1e6 + N(0, 1); 1e9 + N(0, 1e-3); a noisy ramp; a random walk; a
    constant; 20 % NaN"""
    holes = rng.normal(0, 1, n)
    holes[rng.random(n) < 0.2] = np.nan
    return {"normal": rng.normal(0, 1, n), "offset1e6": 1e6 + rng.normal(0, 1, n),
            "offset1e9": 1e9 + rng.normal(0, 1e-3, n), "ramp": 0.25 * np.arange(n) + rng.normal(0, 3, n),
            "walk": np.cumsum(rng.normal(0, 1, n)), "constant": np.full(n, 1234.5678), "nan20": holes}


def _cases():
    """every length and input at the stream's start, where the bounds were stated, and at a begin further in"""
    rng = np.random.default_rng(61)
    for k, n in enumerate(LENGTHS):
        for begin in (0, BEGINS[k % len(BEGINS)]):
            for name, v in _inputs(rng, n).items():
                x = np.concatenate([np.full(begin, 1e300), v, rng.normal(-5, 100, 7)])  # the outside must not matter
                yield name, begin, n, x


def _position_factor(begin, count):
    """Node positions are the stream's, so that a tile shared by several windows is reduced once.  Wherever a merge joins
    unequal counts (a window's edges, NaN holes) a node's mean position rounds, by up to L u times the absolute position
    begin + count instead of the window's own extent count, and that error enters dt linearly: the bounds on t_m2 and
    c_tx, stated for windows at the stream's start, grow by (begin + count) / count.  1 at begin == 0."""
    return (begin + count) / count


def _bits(x):
    return np.float64(x).view(np.uint64)


def Fraction_(v):
    return Fraction(float(v))


def test_model_within_bounds_of_exact():
    worst = {}
    for name, begin, count, x in _cases():
        n, mean, m2, t_mean, t_m2, c_tx = M.window_moments(x, begin, count)
        v = x[begin:begin + count]
        en, emean, em2, et_mean, et_m2, ec_tx, eabs = M.exact_moments(v)
        assert n == en, (name, begin, count)
        if en == 0:
            assert all(math.isnan(q) for q in (mean, m2, t_mean, t_m2, c_tx))
            continue
        k, b_m2, b_tm2, b_c = M.bounds(en, emean, em2, et_m2)
        errs = (abs(Fraction_(mean) - emean), abs(Fraction_(m2) - em2), abs(Fraction_(t_m2) - et_m2),
                abs(Fraction_(c_tx) - ec_tx))
        r = _position_factor(begin, count)
        lims = (k * float(eabs), b_m2, r * b_tm2, r * b_c)
        for what, e, lim in zip(("mean", "m2", "t_m2", "c_tx"), errs, lims):
            assert float(e) <= lim, (name, begin, count, what, float(e), lim)
            if lim > 0:
                worst[what] = max(worst.get(what, 0.0), float(e) / lim)
        if em2 == 0:  # a constant window (or a single sample): no spread and no trend, exactly
            assert m2 == 0.0 and c_tx == 0.0, (name, begin, count)
        if en == count and begin == 0:  # at the stream's start, without NaN, the mean position is exact
            assert Fraction_(t_mean) == et_mean, (name, begin, count)
        else:  # the mean of absolute positions, as `mean` of the values
            assert abs(Fraction_(t_mean) - et_mean) <= k * (begin + count), (name, begin, count)
    print("largest error / bound:", worst)


def test_model_against_numpy_var_and_polyfit():
    """numpy.var and numpy.polyfit(deg=1) carry rounding of their own, of the same order: both sides are held to the
    documented bounds around each other, propagated through the fit -- variance: b_m2 / n; slope = c_tx / t_m2:
    r b_c / t_m2 + |slope| r b_tm2 / t_m2; intercept = mean - slope t_mean: b_mean + (slope's bound) t_mean + |slope|
    (t_mean's bound) -- each doubled
    for NumPy's share.  numpy.var centres on its own rounded mean: (b_mean)^2 more."""
    for name, begin, count, x in _cases():
        v = x[begin:begin + count]
        if count < 2 or np.isnan(v).any():
            continue
        n, mean, m2, t_mean, t_m2, c_tx = M.window_moments(x, begin, count)
        _, var, _, _, _, slope, intercept = M.fit(n, mean, m2, t_mean, t_m2, c_tx)
        en, emean, em2, _, et_m2, _, eabs = M.exact_moments(v)
        k, b_m2, b_tm2, b_c = M.bounds(en, emean, em2, et_m2)
        assert abs(var - np.var(v)) <= 2 * b_m2 / n + (k * float(eabs)) ** 2 + 4 * M.U * var, (name, begin, count)
        assert abs(mean - np.mean(v)) <= 2 * k * float(eabs), (name, begin, count)
        p1, p0 = np.polyfit(np.arange(count, dtype=np.float64), v, 1)
        r = _position_factor(begin, count)
        b_slope = r * b_c / float(et_m2) + abs(slope) * r * b_tm2 / float(et_m2)
        assert abs(slope - p1) <= 2 * b_slope + 4 * M.U * abs(slope), (name, begin, count, slope, p1)
        b_icpt = k * float(eabs) + b_slope * t_mean + abs(slope) * k * (begin + count)
        assert abs(intercept - p0) <= 2 * b_icpt + 4 * M.U * abs(intercept), (name, begin, count, intercept, p0)


def test_model_ignores_what_lies_outside_the_window():
    rng = np.random.default_rng(67)
    x = rng.normal(0, 1, 9000)
    y = x.copy()
    y[:1000] = 1e300
    y[3000:] = np.nan
    a, b = M.window_moments(x, 1000, 2000), M.window_moments(y, 1000, 2000)
    assert [_bits(q) for q in a[1:]] == [_bits(q) for q in b[1:]] and a[0] == b[0] == 2000
    assert M.window_moments(x, 5, 0)[0] == 0 and math.isnan(M.window_moments(x, 5, 0)[1])
    y[1000:3000] = np.nan
    assert M.window_moments(y, 1000, 2000)[0] == 0 and math.isnan(M.window_moments(y, 1000, 2000)[3])


def test_moments_dtypes(A):
    assert A.WINDOW_MOMENTS.itemsize == 48
    assert A.WINDOW_MOMENTS.names == ("count", "mean", "m2", "t_mean", "t_m2", "c_tx")
    assert A.WINDOW_FIT.itemsize == 56
    assert A.WINDOW_FIT.names == ("mean", "variance", "stddev", "sample_variance", "sample_stddev", "slope", "intercept")


def test_symbols_exported_and_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_moments_windows_dev", "atsc_moments_windows", "atsc_stream_moments_windows", "atsc_moments_fit"):
        assert name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert callable(A.Context.moments_windows_host) and callable(A.DPlan.moments_windows)
    assert callable(A.CompressedStream.moments_windows) and callable(A.moments_data_windows) and callable(A.moments_fit)


def test_moments_fit_bit_for_bit(A):
    rng = np.random.default_rng(71)
    inf, nan = float("inf"), float("nan")
    rows = [(0, 1.0, 2.0, 3.0, 4.0, 5.0), (0, nan, nan, nan, nan, nan), (1, 7.25, 0.0, 0.0, 0.0, 0.0),
            (2, -3.5, 0.5, 0.5, 0.5, -0.5), (2, 1e9, 2e-6, 0.5, 0.5, 1e-3), (5, 3.0, 10.0, 2.0, 0.0, 0.0),
            (5, 3.0, 10.0, 2.0, -0.0, 1.0), (9, inf, nan, 4.0, 60.0, nan), (9, 1.0, inf, 4.0, 60.0, inf),
            (9, -inf, nan, 4.0, 60.0, -inf), (3, 1.0, 2.0, 1.0, 2.0, inf), (4, 0.1, 0.3, 1.5, 5.0, 0.7),
            (2 ** 53 + 2, 0.1, 0.3, 1.5, 5.0, 0.7), (7, 1.0, 2.0, 3.0, nan, 1.0), (6, 1e-300, 1e-320, 2.5, 17.5, 1e-310)]
    for _ in range(300):
        n = int(rng.integers(1, 100000))
        rows.append((n, rng.normal(0, 1e3), abs(rng.normal(0, 1e3)) * n, (n - 1) / 2 * rng.random(),
                     float(n) * (n * n - 1) / 12 * rng.random(), rng.normal(0, 1e4)))
    m = np.zeros(len(rows), dtype=A.WINDOW_MOMENTS)
    for i, r in enumerate(rows):
        m[i] = r
    got = A.moments_fit(m)
    assert got.dtype == A.WINDOW_FIT and len(got) == len(rows)
    for r, g in zip(rows, got):
        want = M.fit(*r)
        for name, w in zip(A.WINDOW_FIT.names, want):
            assert (np.isnan(w) and np.isnan(g[name])) or _bits(w) == _bits(g[name]), (r, name, w, g[name])
    assert all(np.isnan(got[0][k]) for k in A.WINDOW_FIT.names)  # count == 0: all NaN whatever the other fields hold
    assert np.isnan(got[2]["sample_variance"]) and got[2]["variance"] == 0.0 and np.isnan(got[2]["slope"])  # count == 1
    assert got[3]["sample_variance"] == 0.5 and got[3]["slope"] == -1.0 and got[3]["intercept"] == -3.0  # count == 2
    assert np.isnan(got[5]["slope"]) and np.isnan(got[6]["slope"]) and np.isnan(got[5]["intercept"])  # t_m2 == 0
    assert len(A.moments_fit(np.zeros(0, dtype=A.WINDOW_MOMENTS))) == 0
    lib = A.capi.lib()
    out = np.zeros(1, dtype=A.WINDOW_FIT)
    assert lib.atsc_moments_fit(None, 1, C.c_void_p(out.ctypes.data)) == A.capi.E_INVALID
    assert lib.atsc_moments_fit(C.c_void_p(m.ctypes.data), 1, None) == A.capi.E_INVALID
    assert lib.atsc_moments_fit(None, 0, None) == 0


def test_command_line_usage_errors(A, tmp_path):
    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    f = tmp_path / "x.bro"
    f.write_bytes(b"")
    for cmd in ([atsc, "-u", "--moments", str(f)], [atsc, "--moments", str(f)], [atsc, "--buckets", "5", "--moments", str(f)],
                [csvc, "-u", "--moments", str(f)], [csvc, "-u", "--from", "0", "--to", "10", "--moments", str(f)],
                [csvc, "--moments", str(f)]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (cmd, r.stderr)
        assert "error:" in r.stderr, cmd
    for exe in (atsc, csvc):
        r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--moments" in r.stderr and "per sample" in r.stderr.lower(), exe
