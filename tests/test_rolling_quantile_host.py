"""The windowed rolling quantiles' contract, without a GPU: the two forms of the NumPy model (tests/rolling_quantile_model.py:
the sliding view sorted in blocks, and the listed windows one at a time) agree bit for bit; the model equals
numpy.nanquantile as a value on finite data for all four methods; all-NaN and part-NaN windows; -0.0 before +0.0; a
position's row depends on the stream and the window alone; the rule that sizes a task; and the new symbols and Python
surfaces exist."""
import math
import warnings

import numpy as np
import pytest

from tests import quantile_model as QM
from tests import rolling_quantile_model as M

N = 9000
LEVELS = [0.5, 0.0, 1.0, 0.99, 0.5, 0.123, 1.0 / 3.0]  # unsorted, a duplicate, both ends


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


@pytest.fixture(scope="module")
def data():
    """mixed magnitudes, both signs, NaN holes, a stretch of NaN, a flat stretch, zeros of both signs and +-Inf"""
    rng = np.random.default_rng(47)
    x = rng.normal(0, 1, N) * 10.0 ** rng.integers(-3, 6, N)
    x[rng.random(N) < 0.03] = np.nan
    x[5000:5100] = np.nan
    x[7000:7050] = 4.25
    x[7100:7110:2] = 0.0
    x[7101:7110:2] = -0.0
    x[100], x[200] = np.inf, -np.inf
    return x


def _same(a, b):
    """bit for bit, any NaN where the other is NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("method", M.METHODS)
def test_the_two_forms_of_the_model_agree(data, method):
    rng = np.random.default_rng(method)
    for w in (1, 2, 3, 64, 65, 300, 2049, 8192):
        lo = np.unique(np.concatenate([[0, N - w], rng.integers(0, N - w + 1, 40),
                                       np.clip([5000 - w // 2, 5100 - w, 7100 - w + 3], 0, N - w)]))
        assert _same(M.rows(data, lo, w, LEVELS, method), M.literal(data, lo, w, LEVELS, method)), (w, method)


def test_rolling_is_rows_at_the_positions(data):
    b, c, w, s = [3, 100, 50, 8000], [4000, 299, 300, 1000], 300, 7
    got, off = M.rolling(data, b, c, w, s, LEVELS)
    assert off.tolist() == [0, M.outputs(4000, w, s), M.outputs(4000, w, s), M.outputs(4000, w, s) + 1,
                            M.outputs(4000, w, s) + 1 + 101]
    lo = M.positions(b, c, w, s)
    assert len(lo) == len(got) == int(off[-1]) and lo[0] == 3 and lo[int(off[2])] == 50 and lo[-1] == 8000 + 700
    assert _same(got, M.literal(data, lo, w, LEVELS))


@pytest.mark.parametrize("method", M.METHODS)
def test_model_is_nanquantile_on_finite_data(method):
    rng = np.random.default_rng(53)
    x = rng.normal(0, 1000, 3000)
    x[rng.random(3000) < 0.1] = np.nan
    lv = [0.0, 0.25, 0.5, 0.9, 0.99, 1.0]
    for w in (1, 5, 64, 301):
        lo = np.arange(0, 3000 - w + 1, 37)
        got = M.rows(x, lo, w, lv, method)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (an all-NaN window: NaN, and NumPy says so)
            want = np.array([np.nanquantile(x[a:a + w], lv, method=QM.METHOD_NAMES[method]) for a in lo])
        both_nan = np.isnan(got) & np.isnan(want)
        assert np.all(both_nan | (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))), (w, method)
        assert np.all(both_nan | (got == want)) or method == M.LINEAR  # selection is exact: only the lerp may round apart


def test_all_nan_and_part_nan_windows(data):
    for lo, w in ((5000, 100), (5001, 64), (5010, 7), (5099, 1)):
        r = M.rows(data, [lo], w, LEVELS)[0]
        assert all(math.isnan(v) for v in r), (lo, w)
    # a window half inside the stretch of NaN: the levels of its samples alone
    lo, w = 4950, 100
    r = M.rows(data, [lo], w, [0.0, 0.5, 1.0])[0]
    live = data[lo:5000]
    live = live[~np.isnan(live)]
    assert 0 < len(live) <= 50 and r[0] == live.min() and r[2] == live.max() and r[1] == np.median(live)


def test_negative_zero_sorts_before_positive_zero(data):
    lo, w = 7100, 10  # five +0.0 and five -0.0, alternating
    assert np.all(data[lo:lo + w] == 0.0)
    r = M.rows(data, [lo], w, [0.0, 4.0 / 9.0, 5.0 / 9.0, 1.0], M.LOWER)[0]
    assert np.signbit(r).tolist() == [True, True, False, False]
    r = M.rows(data, [lo + 1], w - 2, [0.0, 1.0], M.HIGHER)[0]  # four of each
    assert np.signbit(r).tolist() == [True, False]


def test_a_position_does_not_depend_on_range_or_stride(data):
    keys = M.stream_keys(data)
    for w in (2, 65, 300, 2049):
        a, off_a = M.rolling(data, [0], [N], w, 1, LEVELS, keys=keys)
        assert int(off_a[1]) == N - w + 1
        for begin, stride in ((1, 7), (5, w), (12, 2 * w + 1), (2048, 3)):
            b, off_b = M.rolling(data, [begin, 100], [N - begin, 50 + w], w, stride, LEVELS, keys=keys)
            lo = begin + stride * np.arange(int(off_b[1]))
            assert _same(a[lo], b[: len(lo)]), (w, begin, stride)
            lo2 = 100 + stride * np.arange(int(off_b[2] - off_b[1]))
            assert _same(a[lo2], b[len(lo):]), (w, begin, stride)


def test_the_rule_that_sizes_a_task():
    """P by the width alone: the least power of two in [512, 8192] that holds two windows, 8192 above w = 4096; a task
    holds B = (P - w) / s + 1 positions, whose windows cover (B - 1) s + w <= P samples"""
    assert [M.span_keys(w) for w in (1, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8191, 8192)] == \
        [512, 512, 1024, 1024, 2048, 2048, 4096, 4096, 8192, 8192, 8192, 8192, 8192]
    for w in (1, 20, 256, 257, 300, 3600, 4096, 4097, 8192):
        for s in (1, 2, 7, 64, w + 1, 8193):
            b = M.task_positions(w, s)
            assert b >= 1 and (b - 1) * s + w <= M.span_keys(w) < b * s + w
    assert M.task_positions(8192, 1) == 1 and M.task_positions(20, 1) == 493 and M.task_positions(3600, 1) == 4593


def test_symbols_and_surfaces(A):
    lib = A.capi.lib()
    for name in ("atsc_rolling_quantile_windows_dev", "atsc_rolling_quantile_windows", "atsc_stream_rolling_quantile_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert A.ROLLING_QUANTILE_MAX_WIDTH == M.MAX_WIDTH == 8192
    for owner, name in ((A.Context, "rolling_quantile_windows_host"), (A.DPlan, "rolling_quantile_windows"),
                        (A.CompressedStream, "rolling_quantile_windows"), (A, "rolling_quantile_data_windows")):
        assert getattr(owner, name).__doc__.strip()
