"""The windowed rolling deltas without a GPU: the NumPy model of the contract (tests/rolling_delta_model.py) -- its chunk
walk, its two forms against each other, its counts and maxima against the windowed deltas' model, its error bound, its
independence of range and stride, exactness on an integer counter -- and the new symbols of the library."""
import math

import numpy as np
import pytest

from tests import delta_model as D
from tests import rolling_delta_model as M
from tests import rolling_model as R

WIDTHS = [1, 2, 3, 4, 5, 9, 64, 65, 66, 300, 2048, 2049, 2050, 4097, 4098]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


@pytest.fixture(scope="module")
def data():
    """20000 samples of mixed magnitudes, 1e-3 .. 1e5, both signs, with NaN holes, a stretch of NaN and flat stretches"""
    rng = np.random.default_rng(17)
    x = rng.normal(0, 1, 20000) * 10.0 ** rng.integers(-3, 6, 20000)
    x[rng.random(20000) < 0.03] = np.nan
    x[5000:5100] = np.nan
    x[7000:7050] = 4.25
    x[300:306] = [0.0, -0.0, 0.0, 5.0, 5.0, -0.0]
    return x


@pytest.fixture(scope="module")
def counter():
    """an integer counter: steps of 0 .. 50, a reset to a small value now and then, NaN holes"""
    rng = np.random.default_rng(23)
    n = 12000
    x = np.empty(n)
    v = 1000
    for i in range(n):
        v = int(rng.integers(0, 20)) if rng.random() < 0.004 else v + int(rng.integers(0, 51))
        x[i] = v
    x[rng.random(n) < 0.01] = np.nan
    x[4000:4003] = np.nan
    return x


def test_chunk_walk_covers_the_pair_slots_once_aligned_and_short():
    rng = np.random.default_rng(5)
    for w in WIDTHS + [70001, (1 << 18) + 2, R.MAX_WIDTH]:
        for lo in [0, 1, 2046, 2047, 2048, 65535, 65536, (1 << 20) - 1, 1 << 20] + [int(v) for v in rng.integers(0, 1 << 22, 12)]:
            c = M.chunks(lo, w)
            pos = lo + 1
            for p, l in c:
                assert p == pos and p % (1 << l) == 0 and p + (1 << l) <= lo + w, (lo, w, p, l)
                pos += 1 << l
            assert pos == max(lo + w, lo + 1) and (w > 1 or c == [])
            assert len(c) <= (2 * math.ceil(math.log2(w)) if w > 1 else 0), (lo, w, len(c))
            if w > 1:  # the highest level is floor(log2(w - 1)) at the most, and some position reaches it
                assert max(l for _, l in c) <= math.floor(math.log2(w - 1))
    for w in (2, 3, 5, 9, 65, 2049, 70001, (1 << 18) + 2):
        top = math.floor(math.log2(w - 1))
        assert max(l for _, l in M.chunks((1 << 20) - 1, w)) == top  # the slots begin at a multiple of 2^20


def _same(a, b):
    """the eight fields bit for bit"""
    return np.array([tuple(a)], dtype=M.RECORD).tobytes() == np.array([tuple(b)], dtype=M.RECORD).tobytes()


def _positions(n, w, extra=()):
    rng = np.random.default_rng(3)
    lo = {0, 1, 298, 299, 300, 301, 305, 2030, 2046, 2047, 2048, 2049, 4998, 4999, 5000, 5050, 5099, 6990, n - w} | set(extra)
    lo |= {int(v) for v in rng.integers(0, max(n - w, 1), 40)}
    return sorted(v for v in lo if 0 <= v <= n - w)


def test_the_two_forms_of_the_model_agree(data):
    x = data.copy()
    x[310:314] = [np.inf, -np.inf, 1.0, np.inf]
    P = M.Pyramid(x)
    for w in WIDTHS:
        lo = _positions(len(x), w)
        got = P.records(lo, w)
        for i, b in enumerate(lo):
            assert _same(got[i], M.window_record(x, b, w)), (b, w)


def test_counts_and_maxima_are_the_windowed_deltas(data):
    P = M.Pyramid(data)
    for w in WIDTHS:
        lo = _positions(len(data), w)
        got = P.records(lo, w)
        want = D.windows_delta(data, [(b, w) for b in lo])
        for k in ("pairs", "rises", "falls", "max_rise", "max_fall"):
            assert got[k].tobytes() == want[k].tobytes(), (w, k)


def test_sums_within_the_bound_of_fsum(data):
    """|up - exact| <= (3 L + 1) u up_exact and the same for down, exact being math.fsum over the pairs' samples (b and
    -a of every rise: the exact differences' sum correctly rounded, not the rounded differences')"""
    worst = 0.0
    for w in WIDTHS:
        for lo in (0, 1, 777, 4000, 4999, 5000, 5050, 6990, len(data) - w):
            if lo < 0 or lo + w > len(data) or w < 2:
                continue
            v = data[lo:lo + w]
            a, b = v[:-1], v[1:]
            ok = ~np.isnan(a) & ~np.isnan(b)
            with np.errstate(invalid="ignore"):
                rise, fall = ok & (b > a), ok & (b < a)
            rec = M.window_record(data, lo, w)
            up_exact = math.fsum(list(b[rise]) + list(-a[rise]))
            down_exact = math.fsum(list(a[fall]) + list(-b[fall]))
            for got, exact in ((rec[3], up_exact), (rec[4], down_exact)):
                bound = M.bound_factor(w) * exact
                assert exact >= 0.0 and abs(got - exact) <= bound, (lo, w, got, exact, bound)
                if bound:
                    worst = max(worst, abs(got - exact) / bound)
    assert 0.0 < worst < 1.0
    only_nan = M.window_record(data, 5000, 100)
    assert only_nan == (0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0) and not any(np.signbit(v) for v in only_nan[3:])
    flat = M.window_record(data, 7000, 50)  # counted pairs, no rise and no fall: the sums are +0.0
    assert flat[:3] == (49, 0, 0) and flat[3:] == (0.0,) * 5 and not any(np.signbit(v) for v in flat[3:])


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


def test_integer_counter_is_exact_and_equals_the_windowed_deltas(counter):
    x = counter
    P = M.Pyramid(x)
    for w in (2, 3, 9, 65, 300, 2049, 4098):
        lo = _positions(len(x), w, extra=(3990, 3999, 4000, 4001, 4002, 4003))
        got = P.records(lo, w)
        want = D.windows_delta(x, [(b, w) for b in lo])
        assert got.tobytes() == want.tobytes(), w
        for i, b in enumerate(lo):
            true = 0
            for p, q in zip(x[b:b + w - 1], x[b + 1:b + w]):
                if not (math.isnan(p) or math.isnan(q)):
                    true += int(q - p) if q > p else int(q) if q < p else 0
            increase = D.derive(*(got[i][k] for k in D.FIELDS))[3]
            assert float(increase) == float(true), (b, w)


def test_width_one_is_the_all_zero_record(data):
    P = M.Pyramid(data)
    rec, off = P.rolling([0, 5000], [100, 7], 1, 1)
    assert list(off) == [0, 100, 107] and rec.tobytes() == bytes(64 * 107)
    assert M.window_record(data, 3, 1) == (0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert M.chunks(3, 1) == []


def test_symbols_and_surfaces(A):
    lib = A.capi.lib()
    for name in ("atsc_rolling_delta_windows_dev", "atsc_rolling_delta_windows", "atsc_stream_rolling_delta_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES
    assert A.WINDOW_DELTA.itemsize == 64 and A.WINDOW_DELTA.names == D.FIELDS
    for owner, name in ((A.Context, "rolling_delta_windows_host"), (A.DPlan, "rolling_delta_windows"),
                        (A.CompressedStream, "rolling_delta_windows"), (A, "rolling_delta_data_windows")):
        assert getattr(owner, name).__doc__.strip()
