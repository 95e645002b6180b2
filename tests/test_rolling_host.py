"""The windowed rolling without a GPU: the NumPy model of the contract (tests/rolling_model.py) -- its chunk walk, its
error bound, its independence of range and stride, its two forms against each other -- and the host-only parts of the
library: atsc_rolling_outputs and the new symbols."""
import math

import numpy as np
import pytest

from tests import rolling_model as M

WIDTHS = [1, 2, 3, 5, 8, 63, 64, 65, 300, 1000, 2047, 2048, 2049, 4097, 16384]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


@pytest.fixture(scope="module")
def data():
    """20000 samples of mixed magnitudes, 1e-3 .. 1e5, both signs, with NaN holes and a stretch of NaN"""
    rng = np.random.default_rng(11)
    x = rng.normal(0, 1, 20000) * 10.0 ** rng.integers(-3, 6, 20000)
    x[rng.random(20000) < 0.03] = np.nan
    x[5000:5100] = np.nan
    return x


def test_chunk_walk_covers_each_window_once_aligned_and_short():
    rng = np.random.default_rng(5)
    for w in WIDTHS + [70001, M.MAX_WIDTH]:
        for lo in [0, 1, 2047, 2048, 65535, 65536, (1 << 20) - 1, 1 << 20] + [int(v) for v in rng.integers(0, 1 << 22, 12)]:
            c = M.chunks(lo, w)
            pos = lo
            for p, l in c:
                assert p == pos and p % (1 << l) == 0 and p + (1 << l) <= lo + w, (lo, w, p, l)
                pos += 1 << l
            assert pos == lo + w
            assert len(c) <= (2 * math.ceil(math.log2(w)) if w > 1 else 1), (lo, w, len(c))
            # left to right, the levels rise and then fall: each chunk is the largest that fits
            lv = [l for _, l in c]
            top = lv.index(max(lv))
            assert lv[:top + 1] == sorted(lv[:top + 1]) and lv[top:] == sorted(lv[top:], reverse=True)


def test_sum_within_the_bound_of_fsum(data):
    worst = 0.0
    for w in WIDTHS:
        for lo in (0, 1, 777, 4000, 4999, 5000, 5050, len(data) - w):
            if lo < 0 or lo + w > len(data):
                continue
            v = data[lo:lo + w]
            got, exact = M.window_sum(data, lo, w), math.fsum(v[~np.isnan(v)])
            bound = M.error_bound(v)
            assert abs(got - exact) <= bound, (lo, w, got, exact, bound)
            if bound:
                worst = max(worst, abs(got - exact) / bound)
    assert worst < 1.0
    assert M.window_sum(data, 5000, 100) == 0.0 and not np.signbit(M.window_sum(data, 5000, 100))  # only NaN: +0.0


def test_sum_does_not_depend_on_range_or_stride(data):
    P = M.Pyramid(data)
    for w in (3, 64, 300, 2049):
        a, off_a = P.rolling([0], [len(data)], w, 1)
        for begin, stride in ((1, 7), (5, w), (12, 2 * w + 1), (2048, 3)):
            b, off_b = P.rolling([begin, 100], [len(data) - begin, 50 + w], w, stride)
            lo = begin + stride * np.arange(int(off_b[1]))
            assert a[lo].tobytes() == b[: len(lo)].tobytes(), (w, begin, stride)
            lo2 = 100 + stride * np.arange(int(off_b[2] - off_b[1]))
            assert a[lo2].tobytes() == b[len(lo):].tobytes(), (w, begin, stride)


def _same_record(a, b):
    return all(x == y or (x != x and y != y) for x, y in zip(a, b)) and np.signbit(a[1]) == np.signbit(b[1]) and \
        np.signbit(a[2]) == np.signbit(b[2]) and np.signbit(a[3]) == np.signbit(b[3])


def test_the_two_forms_of_the_model_agree(data):
    x = data.copy()
    x[300:310] = [0.0, -0.0, 5.0, -0.0, 0.0, np.inf, -np.inf, 1.0, -0.0, 0.0]
    x[2040:2060] = np.tile([-0.0, 0.0], 10)  # zeros of both signs on both sides of a tile boundary
    x[2040:2048] = 3.0
    x[9000:9003] = [-0.0, -0.0, -0.0]
    P = M.Pyramid(x)
    rng = np.random.default_rng(3)
    for w in (1, 2, 3, 7, 64, 65, 300, 2049):
        lo = sorted({0, 1, 299, 300, 301, 305, 2030, 2047, 2048, 2049, 8999, 9000, 5000, len(x) - w} |
                    {int(v) for v in rng.integers(0, len(x) - w, 40)})
        lo = [v for v in lo if 0 <= v <= len(x) - w]
        got = P.records(lo, w)
        for i, b in enumerate(lo):
            want = M.window_record(x, b, w)
            assert _same_record((int(got[i]["count"]), float(got[i]["min"]), float(got[i]["max"]), float(got[i]["sum"])), want), (b, w)


def test_zero_sign_follows_the_visiting_order():
    x = np.ones(8192)
    x[[2, 512]] = [0.0, -0.0]  # slot 512 is virtual lane 0, slot 2 virtual lane 1: lane 0 is visited first
    assert M.zero_sign(x, 0, 2048) is True and M.zero_sign(x, 1, 511) is False
    x[[2050, 4100]] = [0.0, -0.0]  # the first tile with a zero decides
    assert M.zero_sign(x, 2048, 4096) is False and M.zero_sign(x, 2051, 4000) is True
    x[[4101]] = [0.0]  # one pair: the even slot first
    assert M.zero_sign(x, 4096, 100) is True


def test_rolling_outputs(A):
    f = A.rolling_outputs
    for w in (1, 2, 300, 1 << 20):
        assert f(w - 1, w, 1) == 0 and f(0, w, 3) == 0
        assert f(w, w, 1) == 1 and f(w, w, 1000) == 1
    assert f(10, 0, 1) == 0 and f(10, 1, 0) == 0 and f(0, 0, 0) == 0
    rng = np.random.default_rng(2)
    for _ in range(200):
        c, w, s = (int(v) for v in rng.integers(1, 5000, 3))
        assert f(c, w, s) == M.outputs(c, w, s) == ((c - w) // s + 1 if c >= w else 0)
    assert f(2 ** 64 - 1, 1, 1) == 2 ** 64 - 1
    assert list(A.rolling_offsets([10, 2, 3, 0], 3, 2)) == [0, 4, 4, 5, 5]


def test_symbols_and_surfaces(A):
    lib = A.capi.lib()
    for name in ("atsc_rolling_outputs", "atsc_rolling_windows_dev", "atsc_rolling_windows", "atsc_stream_rolling_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES
    assert A.WINDOW_ROLLING.itemsize == 32 and A.WINDOW_ROLLING.names == ("count", "min", "max", "sum")
    assert A.ROLLING_MAX_WIDTH == 1 << 20
    for owner, name in ((A.Context, "rolling_windows_host"), (A.DPlan, "rolling_windows"),
                        (A.CompressedStream, "rolling_windows"), (A, "rolling_data_windows")):
        assert getattr(owner, name).__doc__.strip()
