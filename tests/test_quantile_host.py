"""CPU-only tests of the windowed quantiles: the NumPy model of the contract against numpy.nanquantile, the documented
infinity cases, the command lines' argument errors (exit 2 before any GPU work) and the C functions' null-context
checks."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import quantile_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATSC = os.path.join(ROOT, "atsc_amd", "bin", "atsc")
CSV = os.path.join(ROOT, "atsc_amd", "bin", "csv-compressor")


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _same(a, b):
    """equal as values, and bit for bit unless the value is zero (NumPy's sign of a zero result may differ)"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if a != b:
        return False
    return a == 0.0 or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def _windows(rng, n_windows):
    for it in range(n_windows):
        n = int(rng.integers(1, 5001))
        kind = it % 4
        if kind == 0:
            x = rng.normal(0, 1, n) * 10.0 ** int(rng.integers(-6, 7))
        elif kind == 1:  # duplicate-heavy
            x = rng.integers(-3, 4, n).astype(np.float64) * 0.25
        elif kind == 2:
            x = np.round(rng.normal(100, 5, n), 1)
        else:
            x = rng.uniform(-1e300, 1e300, n)
        if it % 3 == 0:
            x[rng.integers(0, n, n // 5 + 1)] = np.nan
        yield x


@pytest.mark.parametrize("method", [M.LINEAR, M.LOWER, M.HIGHER, M.NEAREST])
def test_model_matches_nanquantile(method):
    rng = np.random.default_rng(100 + method)
    fixed = [0.0, 1.0, 0.5, 1.0 / 3.0, 0.99, 0.999]
    checked = 0
    for x in _windows(rng, 160):
        levels = fixed + list(rng.random(3))
        s = M.sort_total(x)
        if len(s) == 0:
            assert all(math.isnan(M.level(s, q, method)) for q in levels)
            continue
        want = np.nanquantile(x, levels, method=M.METHOD_NAMES[method])
        for q, w in zip(levels, want):
            got = M.level(s, q, method)
            assert _same(got, float(w)), (len(x), q, method, got, float(w))
            checked += 1
    assert checked > 1000


def test_model_all_nan_and_empty():
    for x in (np.array([]), np.full(7, np.nan)):
        for method in (M.LINEAR, M.LOWER, M.HIGHER, M.NEAREST):
            assert np.all(np.isnan(M.quantiles(x, [0.0, 0.5, 1.0], method)))


def test_model_total_order_and_ties():
    x = np.array([0.0, -0.0, 1.0, -1.0, np.nan, -np.inf, np.inf, 5e-324, -5e-324])
    s = M.sort_total(x)
    bits = s.view(np.uint64)
    assert list(bits) == list(np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf]).view(np.uint64))
    # nearest rounds v = 0.5, 1.5, 2.5 to even ranks
    y = np.arange(6.0)
    assert M.quantiles(y[:2], [0.5], M.NEAREST)[0] == 0.0
    assert M.quantiles(y[:4], [0.5], M.NEAREST)[0] == 2.0
    assert M.quantiles(y[:6], [0.5], M.NEAREST)[0] == 2.0


def test_documented_infinity_cases():
    # NumPy's _lerp meets Inf - Inf (or Inf * 0) and gives NaN; the contract returns the sample at the exact rank
    with np.errstate(invalid="ignore"):
        assert math.isnan(float(np.quantile([1.0, np.inf], 1.0)))
        assert math.isnan(float(np.quantile([-np.inf, 1.0], 0.0)))
    assert M.quantiles([1.0, np.inf], [1.0])[0] == np.inf
    assert M.quantiles([-np.inf, 1.0], [0.0])[0] == -np.inf
    # where the interpolation itself spans both infinities both give NaN
    with np.errstate(invalid="ignore"):
        assert math.isnan(float(np.quantile([-np.inf, np.inf], 0.5)))
    assert math.isnan(M.quantiles([-np.inf, np.inf], [0.5])[0])


def _run(argv):
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = "-1"  # exit 2 must come before any GPU work
    return subprocess.run(argv, capture_output=True, text=True, env=env, timeout=60)


BAD_LEVELS = ["", "0.5,", ",0.5", "x", "0.5,abc", "1.5", "-0.1", "nan", "inf", " 0.5", ",".join(["0.5"] * 65)]


def test_atsc_cli_quantile_argument_errors(A, tmp_path):
    f = str(tmp_path / "missing.bro")
    r = _run([ATSC, "-u", "--quantiles", "0.5", f])
    assert r.returncode == 2 and "--buckets" in r.stderr, r.stderr
    for bad in BAD_LEVELS:
        r = _run([ATSC, "-u", "--buckets", "60", "--quantiles", bad, f])
        assert r.returncode == 2 and "--quantiles" in r.stderr, (bad, r.returncode, r.stderr)
    r = _run([ATSC, "-u", "--buckets", "60", "--quantiles", "0.5", "--quantile-method", "median", f])
    assert r.returncode == 2 and "--quantile-method" in r.stderr, r.stderr
    r = _run([ATSC, "-u", "--buckets", "60", "--quantile-method", "lower", f])
    assert r.returncode == 2, r.stderr


def test_csv_compressor_quantile_argument_errors(A, tmp_path):
    f = str(tmp_path / "missing.csv")
    r = _run([CSV, "-u", "--from", "0", "--to", "100", "--quantiles", "0.5", f])
    assert r.returncode == 2 and "--step" in r.stderr, r.stderr
    for bad in BAD_LEVELS:
        r = _run([CSV, "-u", "--from", "0", "--to", "100", "--step", "10", "--quantiles", bad, f])
        assert r.returncode == 2 and "--quantiles" in r.stderr, (bad, r.returncode, r.stderr)
    r = _run([CSV, "-u", "--from", "0", "--to", "100", "--step", "10", "--quantiles", "0.5", "--quantile-method", "mid",
              f])
    assert r.returncode == 2 and "--quantile-method" in r.stderr, r.stderr


def test_null_context_is_invalid(A):
    L = A.capi.lib()
    one = (C.c_uint64 * 1)(0)
    q = (C.c_double * 1)(0.5)
    out = (C.c_double * 1)(7.0)
    body = (C.c_uint8 * 16)()
    rc = L.atsc_quantile_windows_dev(None, None, None, 1, one, one, 1, q, 0, C.cast(out, C.c_void_p), None)
    assert rc == A.capi.E_INVALID
    rc = L.atsc_quantile_windows(None, body, 16, 0, 1, one, one, 1, q, 0, out)
    assert rc == A.capi.E_INVALID
    rc = L.atsc_stream_quantile_windows(None, 1, one, one, 1, q, 0, out)
    assert rc == A.capi.E_INVALID
    assert out[0] == 7.0


def test_quantile_constants(A):
    assert (A.QUANTILE_LINEAR, A.QUANTILE_LOWER, A.QUANTILE_HIGHER, A.QUANTILE_NEAREST) == (0, 1, 2, 3)
    assert (M.LINEAR, M.LOWER, M.HIGHER, M.NEAREST) == (0, 1, 2, 3)
