"""The windowed across quantiles without a GPU: the vectorised NumPy model (tests/across_quantile_model.py) against
tests/quantile_model.py's definition column by column -- hand-written and random columns, every N that takes another
padded size, the four methods, levels whose (n - 1) q is an exact integer for some n only --, the order of the list, the
new symbols, the four public surfaces and the command line's argument errors (exit 2 before any GPU work)."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import across_quantile_model as M
from tests import quantile_model as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATSC = os.path.join(ROOT, "atsc_amd", "bin", "atsc")
NAN, INF = np.nan, np.inf
METHODS = [M.LINEAR, M.LOWER, M.HIGHER, M.NEAREST]
LEVELS = [0.0, 1.0, 0.5, 1.0 / 3.0, 0.25, 0.999]
# (n - 1) q is an exact integer for some n and not for others: q = j / 4 at n = 5, 9, 33; 1 / 8 at 9 and 33; 3 / 32 at 33
# only; 0.2 and 0.7 only through rounding (0.2 * 5 == 1.0, 0.7 * 10 == 7.000000000000001 is not)
EXACT = [0.25, 0.75, 0.125, 3.0 / 32.0, 0.2, 0.7, 1.0 / 7.0, 62.0 / 63.0]
SIZES = [1, 2, 3, 5, 8, 9, 33, 64]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _by_definition(x, levels, method):
    """quantile_model.quantiles of every column of x: (P, n_q)"""
    return np.array([Q.quantiles(x[:, p], levels, method) for p in range(x.shape[1])]).reshape(x.shape[1], len(levels))


def _hand_columns(n):
    """columns of n samples each, as an (n, P) array: all NaN, one value, ties, zeros of both signs in both orders, +-Inf"""
    cols = [np.full(n, NAN), np.r_[np.full(n - 1, NAN), 2.5], np.r_[-7.0, np.full(n - 1, NAN)], np.full(n, 3.0),
            np.arange(n, dtype=np.float64)[::-1].copy(), np.where(np.arange(n) % 2 == 0, -0.0, 0.0),
            np.where(np.arange(n) % 2 == 0, 0.0, -0.0), np.where(np.arange(n) % 3 == 0, INF, 1.0),
            np.where(np.arange(n) % 3 == 0, -INF, 1.0), np.where(np.arange(n) % 2 == 0, INF, -INF),
            np.where(np.arange(n) % 4 == 1, NAN, np.arange(n) // 3 * 1.5), np.r_[np.full(n - 1, 1e308), -1e308],
            np.where(np.arange(n) % 2 == 0, 5e-324, -5e-324)]
    return np.array(cols).T.copy()


def _random_columns(rng, n, p):
    x = rng.normal(0, 1, (n, p)) * 10.0 ** rng.integers(-3, 4, (n, p))
    x[:, p // 4: p // 2] = np.round(x[:, p // 4: p // 2])  # ties
    x[rng.random((n, p)) < 0.15] = NAN
    x[rng.random((n, p)) < 0.03] = INF
    x[rng.random((n, p)) < 0.03] = -INF
    x[rng.random((n, p)) < 0.03] = -0.0
    x[rng.random((n, p)) < 0.03] = 0.0
    return x


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", SIZES)
def test_model_equals_the_definition(n, method):
    rng = np.random.default_rng(1000 * n + method)
    levels = LEVELS + EXACT
    for x in (_hand_columns(n), _random_columns(rng, n, 120)):
        got = M.rows(x, levels, method)
        want = _by_definition(x, levels, method)
        assert got.shape == want.shape == (x.shape[1], len(levels))
        assert M.same(got, want), (n, method, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:3])
        # the order of the list changes no byte
        assert M.same(M.rows(x[::-1], levels, method), got)
        assert M.same(M.rows(x[rng.permutation(n)], levels, method), got)


def test_model_hand_values():
    x = np.array([[NAN, 4.0, -0.0, INF, NAN], [NAN, 1.0, 0.0, 1.0, 2.0], [NAN, 3.0, -0.0, -INF, NAN]])
    r = M.rows(x, [0.0, 0.5, 1.0])
    assert np.isnan(r[0]).all()
    assert r[1].tolist() == [1.0, 3.0, 4.0]
    assert np.signbit(r[2]).tolist() == [True, True, False]  # -0.0, -0.0, +0.0 in total order
    assert r[3][0] == -INF and r[3][1] == 1.0 and r[3][2] == INF
    assert r[4].tolist() == [2.0, 2.0, 2.0]
    assert M.rows(x, [0.5], M.LOWER)[:, 0].tolist()[1:] == [3.0, -0.0, 1.0, 2.0]
    # LINEAR between two ranks: n = 2, q = 0.25 -> x0 + (x1 - x0) * 0.25
    assert M.rows(np.array([[8.0], [4.0]]), [0.25, 0.75])[0].tolist() == [5.0, 7.0]


def test_model_exact_integer_ranks():
    for q in EXACT:
        hit = [n for n in SIZES if (float(n - 1) * q) == np.floor(float(n - 1) * q)]
        miss = [n for n in SIZES if n not in hit]
        assert len(hit) >= 1 and (len(miss) >= 1 or q in (0.0, 1.0)), (q, hit, miss)


def test_model_ranges(A):
    fulls = [np.arange(30.0), np.arange(30.0)[::-1].copy(), np.full(30, NAN)]
    rows, off = M.across_quantiles(fulls, [3, 0, 29, 5], [10, 0, 1, 15], [0.0, 0.5, 1.0], 4)
    assert off.tolist() == [0, 3, 3, 4, 8] and rows.shape == (8, 3)
    assert rows[:, 0].tolist() == [3.0, 7.0, 11.0, 0.0, 5.0, 9.0, 13.0, 12.0]
    assert rows[:, 1].tolist() == [14.5] * 8
    assert off.tolist() == A.across_offsets([10, 0, 1, 15], 4).tolist()


def test_symbols_are_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_across_quantile_windows_dev", "atsc_across_quantile_windows", "atsc_stream_across_quantile_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES, name


def test_public_surfaces(A):
    want = {(A.Context, "across_quantile_windows_host"):
            "(self, records_list, begins, counts, levels, stride=1, method=0, has_count=False)",
            (A.DPlan, "across_quantile_windows"):
            "(self, d_body, others, other_bodies, begins, counts, levels, d_out, stride=1, method=0, stream=0)",
            (A.CompressedStream, "across_quantile_windows"): "(self, others, begins, counts, levels, stride=1, method=0)",
            (A.stream, "across_quantile_data_windows"): "(ctx, bros, begins, counts, levels, stride=1, method=0)"}
    assert A.QUANTILE_LINEAR == 0
    for (owner, name), sig in want.items():
        f = getattr(owner, name)
        assert str(inspect.signature(f)) == sig, name
        assert f.__doc__ and f.__doc__.strip()
    assert A.across_quantile_data_windows is A.stream.across_quantile_data_windows


def test_null_context_is_invalid(A):
    lib = A.capi.lib()
    assert lib.atsc_across_quantile_windows(None, 1, None, None, None, 0, None, None, 1, 1, None, 0, None) == A.capi.E_INVALID
    assert lib.atsc_across_quantile_windows_dev(None, 1, None, None, 0, None, None, 1, 1, None, 0, None, None) == A.capi.E_INVALID
    assert lib.atsc_stream_across_quantile_windows(None, 1, 0, None, None, 1, 1, None, 0, None) == A.capi.E_INVALID


def _run(argv):
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = "-1"  # exit 2 must come before any GPU work
    return subprocess.run(argv, capture_output=True, text=True, env=env, timeout=60)


BAD_LEVELS = ["", "0.5,", ",0.5", "x", "0.5,abc", "1.5", "-0.1", "nan", "inf", " 0.5", ",".join(["0.5"] * 65)]


def test_atsc_cli_argument_errors(A, tmp_path):
    f, other = str(tmp_path / "missing.bro"), str(tmp_path / "other.bro")
    across = ["-u", "--samples", "0:10", "--across", other]
    r = _run([ATSC, "-u", "--samples", "0:10", "--across-quantiles", "0.5", f])
    assert r.returncode == 2 and "--across-quantiles" in r.stderr and "--across'" in r.stderr, r.stderr
    r = _run([ATSC, "-u", "--samples", "0:10", "--across-quantile-method", "lower", f])
    assert r.returncode == 2 and "--across-quantile-method" in r.stderr, r.stderr
    r = _run([ATSC, *across, "--across-quantile-method", "lower", f])  # the method without the levels
    assert r.returncode == 2 and "--across-quantile-method" in r.stderr and "--across-quantiles" in r.stderr, r.stderr
    for bad in BAD_LEVELS:
        r = _run([ATSC, *across, "--across-quantiles", bad, f])
        assert r.returncode == 2 and "--across-quantiles" in r.stderr, (bad, r.returncode, r.stderr)
    r = _run([ATSC, *across, "--across-quantiles", "0.5", "--across-quantile-method", "median", f])
    assert r.returncode == 2 and "--across-quantile-method" in r.stderr, r.stderr
    # --quantiles keeps its meaning: it needs --buckets, and --across does not go with --buckets
    r = _run([ATSC, *across, "--quantiles", "0.5", f])
    assert r.returncode == 2 and "--buckets" in r.stderr, r.stderr
    # a well-formed command line gets past the arguments (and fails on the missing file, not with a usage error)
    r = _run([ATSC, *across, "--across-quantiles", "0.5,0.9", "--across-quantile-method", "nearest", f])
    assert r.returncode != 2, r.stderr
