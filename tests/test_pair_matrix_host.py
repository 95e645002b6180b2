"""CPU-only tests of the windowed pair matrix' host half: the index helpers against the Python formula for every n and
every (i, j), the NumPy model's identities (the swap against tests/pair_model.py, the diagonal against
tests/moments_model.py) on synthetic data with NaN holes, pair_matrix_correlation's shape and symmetry, and the new
symbols."""
import numpy as np
import pytest

from tests import moments_model as M
from tests import pair_matrix_model as PM
from tests import pair_model as P

SYMBOLS = ("atsc_pair_matrix_windows_dev", "atsc_pair_matrix_windows", "atsc_stream_pair_matrix_windows",
           "atsc_pair_matrix_records", "atsc_pair_matrix_index")


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def test_helpers_against_the_formula(A):
    lib = A.capi.lib()
    none = 2 ** 64 - 1
    assert lib.atsc_pair_matrix_records(0) == 0
    for n in range(1, 65):
        assert lib.atsc_pair_matrix_records(n) == PM.records(n) == A.pair_matrix_records(n)
        seen = []
        for i in range(n + 2):
            for j in range(n + 2):
                want = PM.index(n, i, j)
                assert lib.atsc_pair_matrix_index(n, i, j) == (none if want is None else want), (n, i, j)
                if want is not None:
                    seen.append(want)
        assert seen == list(range(PM.records(n))), n  # row after row, every place once
        assert [PM.index(n, i, j) for i, j in PM.pairs(n)] == list(range(PM.records(n)))
    assert A.pair_matrix_index(64, 63, 63) == 2079 and A.pair_matrix_index(64, 0, 63) == 63
    for bad in ((3, 2, 1), (3, 0, 3), (1, 1, 1)):
        with pytest.raises(ValueError):
            A.pair_matrix_index(*bad)
    assert lib.atsc_pair_matrix_index(0, 0, 0) == none
    assert lib.atsc_pair_matrix_records(2 ** 32 - 1) == (2 ** 32 - 1) * 2 ** 31  # no overflow in 64 bits


@pytest.fixture(scope="module")
def synthetic():
    """four streams of 3 tiles + 100 samples with NaN holes at different slots, one of them a noisy line of another, and
    windows inside a tile, across tiles, whole, of lengths 0 .. 2"""
    rng = np.random.default_rng(3101)
    n = 3 * PM.TILE + 100
    s = [rng.normal(0, 1, n), rng.normal(1e6, 3, n), np.cumsum(rng.normal(0, 1, n)), None]
    s[3] = 2.5 * s[0] - 7 + 0.1 * rng.normal(0, 1, n)
    for k, v in enumerate(s):
        v[rng.random(n) < 0.05 * (k + 1)] = np.nan
    s[2][PM.TILE + 64:PM.TILE + 192] = np.nan
    wins = [(0, n), (0, 0), (5, 1), (5, 2), (100, 700), (PM.TILE - 3, 6), (PM.TILE, PM.TILE), (PM.TILE + 64, 128), (17, 2 * PM.TILE + 9)]
    return s, wins, PM.windows_pair_matrix(s, wins)


def test_model_swap_identity(synthetic):
    s, wins, rec = synthetic
    n = len(s)
    assert rec.shape == (len(wins), PM.records(n))
    swapped = ("count", "mean_y", "m2_y", "mean_x", "m2_x", "c_xy")
    for i, j in PM.pairs(n):
        got = rec[:, PM.index(n, i, j)]
        fwd, rev = P.windows_pair(s[i], s[j], wins), P.windows_pair(s[j], s[i], wins)
        assert np.array_equal(got["count"], fwd["count"]) and np.array_equal(got["count"], rev["count"])
        for k, kr in zip(P.FIELDS[1:], swapped[1:]):
            assert _same(got[k], fwd[k]) and _same(got[k], rev[kr]), (i, j, k)
    # pairwise complete: the holes of the streams outside a pair do not count
    w = 0
    ok = ~(np.isnan(s[0]) | np.isnan(s[1]))
    assert int(rec[w, PM.index(n, 0, 1)]["count"]) == int(ok.sum()) > int((ok & ~np.isnan(s[2])).sum())
    assert int(rec[7, PM.index(n, 2, 3)]["count"]) == 0 and np.isnan(rec[7, PM.index(n, 2, 3)]["c_xy"])  # stream 2 all NaN there
    assert int(rec[7, PM.index(n, 0, 1)]["count"]) > 0


def test_model_diagonal_is_the_moments(synthetic):
    s, wins, rec = synthetic
    n = len(s)
    for i in range(n):
        d = rec[:, PM.index(n, i, i)]
        mom = M.windows_moments(s[i], wins)
        assert np.array_equal(d["count"], mom["count"])
        for k, km in (("mean_x", "mean"), ("mean_y", "mean"), ("m2_x", "m2"), ("m2_y", "m2"), ("c_xy", "m2")):
            assert _same(d[k], mom[km]), (i, k)


def test_correlation_matrix(A, synthetic):
    s, wins, rec = synthetic
    n = len(s)
    r = rec.astype(A.WINDOW_PAIR)
    corr = A.pair_matrix_correlation(r, n)
    assert corr.shape == (len(wins), n, n) and corr.dtype == np.float64
    assert _same(corr, np.swapaxes(corr, 1, 2))
    fit = A.pair_fit(r.reshape(-1)).reshape(r.shape)
    for i, j in PM.pairs(n):
        assert _same(corr[:, i, j], fit["correlation"][:, PM.index(n, i, j)])
    for w in range(len(wins)):
        for i in range(n):
            d = r[w, PM.index(n, i, i)]
            if d["count"] and d["m2_x"] > 0:
                # (m / sqrt(m)) / sqrt(m): two square roots (one value, used twice) and two divides, each within
                # u = 2^-53 relative, so 1 within 4 u + O(u^2), clamped above
                assert abs(corr[w, i, i] - 1.0) <= 2.0 ** -51 and corr[w, i, i] <= 1.0, (w, i)
            else:
                assert np.isnan(corr[w, i, i]), (w, i)
    assert corr[0, 0, 3] > 0.99 and abs(corr[0, 0, 1]) < 0.1  # the line and the independent pair
    assert A.pair_matrix_correlation(np.zeros((0, 3), dtype=A.WINDOW_PAIR), 2).shape == (0, 2, 2)
    with pytest.raises(ValueError):
        A.pair_matrix_correlation(r, n + 2)  # 9 x 10 records are no rows of 21


def test_symbols_exported_and_bound(A):
    lib = A.capi.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in A.capi.SIGNATURES, name
    assert hasattr(A.Context, "pair_matrix_windows_host")
    assert hasattr(A.DPlan, "pair_matrix_windows") and hasattr(A.CompressedStream, "pair_matrix_windows")
    assert callable(A.pair_matrix_data_windows)
