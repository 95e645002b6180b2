"""The windowed across extremes without a GPU: the vectorised NumPy model (tests/across_extremes_model.py) against the
definition -- extremes_model.window_extremes of every column -- on hand-written and random columns with ties, every N
around a padded size and every k around one, k > N included; the consequences the header states (the prefix property,
largest[0] / smallest[0] against the across' max / min, count - nans against its count, the listed values under a
reordering of the list); atsc_extremes_merge over the records of consecutive sub-lists against the record of the whole
list; the new symbols, the four public surfaces and the command line's argument errors (exit 2 before any GPU work)."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import across_extremes_model as M
from tests import across_model as AM
from tests import extremes_model as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATSC = os.path.join(ROOT, "atsc_amd", "bin", "atsc")
NAN, INF = np.nan, np.inf
SIZES = [1, 2, 3, 5, 8, 9, 16, 17, 33, 63, 64]
KS = [1, 2, 3, 5, 8, 9, 16]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _hand_columns(n):
    """columns of n samples each, as an (n, P) array: all NaN, one value, all equal, zeros of both signs in both orders,
    +-Inf, +-1e308, +-5e-324, NaN in every fourth place"""
    i = np.arange(n)
    cols = [np.full(n, NAN), np.r_[np.full(n - 1, NAN), 2.5], np.r_[-7.0, np.full(n - 1, NAN)], np.full(n, 3.0),
            i[::-1].astype(np.float64), np.where(i % 2 == 0, -0.0, 0.0), np.where(i % 2 == 0, 0.0, -0.0),
            np.where(i % 3 == 0, INF, 1.0), np.where(i % 3 == 0, -INF, 1.0), np.where(i % 2 == 0, INF, -INF),
            np.where(i % 4 == 1, NAN, i // 3 * 1.5), np.r_[np.full(n - 1, 1e308), -1e308], np.where(i % 2 == 0, 1e308, -1e308),
            np.where(i % 2 == 0, 5e-324, -5e-324), np.where(i % 3 == 0, -0.0, np.where(i % 3 == 1, 5e-324, 0.0))]
    return np.array(cols).T.copy()


def _random_columns(rng, n, p):
    x = rng.normal(0, 1, (n, p)) * 10.0 ** rng.integers(-3, 4, (n, p))
    x[:, p // 4: p // 2] = np.round(x[:, p // 4: p // 2])  # ties
    x[:, p // 2: 5 * p // 8] = rng.integers(-2, 3, (n, 5 * p // 8 - p // 2))  # many ties
    x[rng.random((n, p)) < 0.15] = NAN
    x[rng.random((n, p)) < 0.03] = INF
    x[rng.random((n, p)) < 0.03] = -INF
    x[rng.random((n, p)) < 0.03] = -0.0
    x[rng.random((n, p)) < 0.03] = 0.0
    return x


def _by_definition(x, k):
    out = np.zeros(x.shape[1], dtype=M.dtype(k))
    for p in range(x.shape[1]):
        out[p] = M.column_record(x[:, p], k)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_model_equals_the_definition(n):
    rng = np.random.default_rng(7000 + n)
    for x in (_hand_columns(n), _random_columns(rng, n, 96)):
        for k in KS:
            got = M.records(x, k)
            assert M.same(got, _by_definition(x, k)), (n, k)
            assert np.all(got["count"] == n)
            used = got["largest"]["at"] != M.NONE
            assert np.array_equal(used.sum(axis=1), np.minimum(k, n - got["nans"]))  # k > N: nothing beyond N
            assert np.array_equal(used, got["smallest"]["at"] != M.NONE)


def test_model_hand_values():
    x = np.array([[NAN, 4.0, -0.0, INF, NAN, 1.0], [NAN, 1.0, 0.0, 1.0, 2.0, 1.0], [NAN, 4.0, -0.0, -INF, NAN, 1.0]])
    r = M.records(x, 2)
    assert r["count"].tolist() == [3] * 6 and r["nans"].tolist() == [3, 0, 0, 0, 2, 0]
    assert np.isnan(r[0]["largest"]["value"]).all() and (r[0]["largest"]["at"] == M.NONE).all()
    assert r[1]["largest"].tolist() == [(4.0, 0), (4.0, 2)] and r[1]["smallest"].tolist() == [(1.0, 1), (4.0, 0)]
    # zeros of either sign are equal: the lowest index first in both lists, each with its own sign
    assert r[2]["largest"]["at"].tolist() == [0, 1] and np.signbit(r[2]["largest"]["value"]).tolist() == [True, False]
    assert r[2]["smallest"]["at"].tolist() == [0, 1] and np.signbit(r[2]["smallest"]["value"]).tolist() == [True, False]
    assert r[3]["largest"].tolist() == [(INF, 0), (1.0, 1)] and r[3]["smallest"].tolist() == [(-INF, 2), (1.0, 1)]
    assert r[4]["largest"]["at"].tolist() == [1, M.NONE] and r[4]["smallest"]["at"].tolist() == [1, M.NONE]
    assert r[5]["largest"]["at"].tolist() == [0, 1] and r[5]["smallest"]["at"].tolist() == [0, 1]  # one stream in both lists


@pytest.mark.parametrize("n", SIZES)
def test_contract_properties(n):
    rng = np.random.default_rng(7100 + n)
    x = np.concatenate([_hand_columns(n), _random_columns(rng, n, 96)], axis=1)
    full = M.records(x, 16)
    for j in KS:
        assert M.same(E.head_of(full, j), M.records(x, j)), (n, j)  # the prefix property
    with np.errstate(over="ignore"):  # (the sum of the +-1e308 columns, which nothing here reads)
        acr = AM.fold(list(x))
    some = acr["count"] > 0
    assert some.any() and (~some).any()
    assert np.array_equal(full["count"] - full["nans"], acr["count"])
    for name, fld in (("largest", "max"), ("smallest", "min")):
        e = full[name][:, 0]
        assert e["value"][some].tobytes() == acr[fld][some].tobytes()  # bit for bit, the sign of a zero included
        assert np.array_equal(e["at"][some], acr[fld + "_at"][some].astype(np.uint64))
        assert np.isnan(e["value"][~some]).all() and np.all(e["at"][~some] == M.NONE)
    # under a reordering of the list the listed values are the same as values; `at` maps through it where no value ties
    perm = rng.permutation(n)
    moved = M.records(x[perm], 16)
    for name in ("largest", "smallest"):
        a, b = full[name], moved[name]
        assert np.array_equal(a["value"], b["value"], equal_nan=True)
        for p in range(x.shape[1]):
            col = x[:, p][~np.isnan(x[:, p])]
            if len(np.unique(col)) == len(col):
                used = a["at"][p] != M.NONE
                assert np.array_equal(perm[b["at"][p][used].astype(np.int64)], a["at"][p][used].astype(np.int64))


def _merged(A, parts, k):
    """extremes_merge per position over the records of the sub-lists"""
    out = np.zeros(len(parts[0]), dtype=M.dtype(k))
    for p in range(len(out)):
        out[p] = A.extremes_merge(np.array([part[p] for part in parts]), k)
    return out


def test_merge_of_sub_lists_is_the_whole_list(A):
    rng = np.random.default_rng(7200)
    x = np.concatenate([_hand_columns(9), _random_columns(rng, 9, 64)], axis=1)
    for k in (1, 3, 16):
        whole = M.records(x, k)
        for cut in range(1, 9):
            assert M.same(_merged(A, [M.records(x[:cut], k), M.records(x[cut:], k)], k), whole), (k, cut)
        assert M.same(_merged(A, [M.records(x[:2], k), M.records(x[2:3], k), M.records(x[3:], k)], k), whole), k
    x = np.concatenate([_hand_columns(128), _random_columns(rng, 128, 64)], axis=1)
    for k in (1, 5, 16):
        got = _merged(A, [M.records(x[:64], k), M.records(x[64:], k)], k)
        assert M.same(got, M.records(x, k)), k
        assert np.all(got["count"] == 128) and got["largest"]["at"][got["largest"]["at"] != M.NONE].max() >= 64


def test_model_ranges(A):
    fulls = [np.arange(30.0), np.arange(30.0)[::-1].copy(), np.full(30, NAN)]
    rec, off = M.across_extremes(fulls, [3, 0, 29, 5], [10, 0, 1, 15], 2, 4)
    assert off.tolist() == [0, 3, 3, 4, 8] and rec.shape == (8,)
    assert rec["largest"]["value"][:, 0].tolist() == [26.0, 22.0, 18.0, 29.0, 24.0, 20.0, 16.0, 17.0]
    assert rec["largest"]["at"][:, 0].tolist() == [1, 1, 1, 0, 1, 1, 1, 0]
    assert rec["smallest"]["at"][:, 0].tolist() == [0, 0, 0, 1, 0, 0, 0, 1]
    assert np.all(rec["nans"] == 1) and np.all(rec["largest"]["at"][:, 1] == rec["smallest"]["at"][:, 0])
    assert off.tolist() == A.across_offsets([10, 0, 1, 15], 4).tolist()


def test_symbols_are_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_across_extremes_windows_dev", "atsc_across_extremes_windows", "atsc_stream_across_extremes_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES, name


def test_public_surfaces(A):
    want = {(A.Context, "across_extremes_windows_host"): "(self, records_list, begins, counts, k, stride=1, has_count=False)",
            (A.DPlan, "across_extremes_windows"): "(self, d_body, others, other_bodies, begins, counts, k, d_out, stride=1, stream=0)",
            (A.CompressedStream, "across_extremes_windows"): "(self, others, begins, counts, k, stride=1)",
            (A.stream, "across_extremes_data_windows"): "(ctx, bros, begins, counts, k, stride=1)"}
    for (owner, name), sig in want.items():
        f = getattr(owner, name)
        assert str(inspect.signature(f)) == sig, name
        assert f.__doc__ and f.__doc__.strip()
    assert A.across_extremes_data_windows is A.stream.across_extremes_data_windows
    assert A.window_extremes_dtype(3) == M.dtype(3) and A.EXTREMES_NONE == M.NONE and A.EXTREMES_MAX_K == M.MAX_K


def test_null_context_is_invalid(A):
    lib = A.capi.lib()
    assert lib.atsc_across_extremes_windows(None, 1, None, None, None, 0, None, None, 1, 1, None) == A.capi.E_INVALID
    assert lib.atsc_across_extremes_windows_dev(None, 1, None, None, 0, None, None, 1, 1, None, None) == A.capi.E_INVALID
    assert lib.atsc_stream_across_extremes_windows(None, 1, 0, None, None, 1, 1, None) == A.capi.E_INVALID


def _run(argv):
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = "-1"  # exit 2 must come before any GPU work
    return subprocess.run(argv, capture_output=True, text=True, env=env, timeout=60)


BAD_K = ["", "0", "17", "-1", "x", "3x", "1.5", "1,2", "99999999999999999999"]


def test_atsc_cli_argument_errors(A, tmp_path):
    f, other = str(tmp_path / "missing.bro"), str(tmp_path / "other.bro")
    across = ["-u", "--samples", "0:10", "--across", other]
    r = _run([ATSC, "-u", "--samples", "0:10", "--across-extremes", "3", f])  # the option without --across
    assert r.returncode == 2 and "--across-extremes" in r.stderr and "--across'" in r.stderr, r.stderr
    for bad in BAD_K:
        r = _run([ATSC, *across, "--across-extremes", bad, f])
        assert r.returncode == 2 and "--across-extremes" in r.stderr, (bad, r.returncode, r.stderr)
    # --extremes keeps its meaning: it needs --buckets, and --across does not go with --buckets
    r = _run([ATSC, *across, "--extremes", "3", f])
    assert r.returncode == 2 and "--buckets" in r.stderr, r.stderr
    r = _run([ATSC, "--help"])
    assert "--across-extremes" in r.stdout + r.stderr
    # a well-formed command line gets past the arguments (and fails on the missing file, not with a usage error)
    for k in ("1", "16"):
        r = _run([ATSC, *across, "--across-stride", "3", "--across-quantiles", "0.5", "--across-extremes", k, f])
        assert r.returncode != 2, r.stderr
