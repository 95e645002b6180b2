"""The windowed rolling histograms' contract, without a GPU: the two forms of the NumPy model
(tests/rolling_histogram_model.py: prefix sums of the one-hot bins, and the listed windows one at a time) agree exactly;
the rows equal numpy.histogram on finite data that avoids the last edge; every row sums to w; a position's row depends
on the stream and the window alone; the rule that sizes a task at its clamps; and the new symbols and Python surfaces
exist."""
import numpy as np
import pytest

from tests import rolling_histogram_model as M

N = 9000
EDGES = [-1000.0, -1.0, 0.0, 0.5, 4.25, 100.0, 1e5]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


@pytest.fixture(scope="module")
def data():
    """mixed magnitudes, both signs, NaN holes, a stretch of NaN, a flat stretch on an edge, zeros of both signs on an
    edge and +-Inf"""
    rng = np.random.default_rng(47)
    x = rng.normal(0, 1, N) * 10.0 ** rng.integers(-3, 6, N)
    x[rng.random(N) < 0.03] = np.nan
    x[5000:5100] = np.nan
    x[7000:7050] = 4.25
    x[7100:7110:2] = 0.0
    x[7101:7110:2] = -0.0
    x[100], x[200] = np.inf, -np.inf
    return x


@pytest.mark.parametrize("closed", (M.LEFT_CLOSED, M.RIGHT_CLOSED))
def test_the_two_forms_of_the_model_agree(data, closed):
    rng = np.random.default_rng(closed)
    for edges in (EDGES, [0.0], [-np.inf, 0.0, np.inf], np.linspace(-50.0, 50.0, 1024)):
        for w in (1, 2, 63, 64, 65, 300, 4096):
            lo = np.unique(np.concatenate([[0, N - w], rng.integers(0, N - w + 1, 40),
                                           np.clip([5000 - w // 2, 5100 - w, 7100 - w + 3, 7000], 0, N - w)]))
            a, b = M.rows(data, lo, w, edges, closed), M.literal(data, lo, w, edges, closed)
            assert a.dtype == b.dtype == np.uint64 and a.shape == (len(lo), len(edges) + 2)
            assert np.array_equal(a, b), (w, closed, len(edges))


def test_rolling_is_rows_at_the_positions(data):
    b, c, w, s = [3, 100, 50, 8000], [4000, 299, 300, 1000], 300, 7
    got, off = M.rolling(data, b, c, w, s, EDGES)
    assert off.tolist() == [0, M.outputs(4000, w, s), M.outputs(4000, w, s), M.outputs(4000, w, s) + 1,
                            M.outputs(4000, w, s) + 1 + 101]
    lo = M.positions(b, c, w, s)
    assert len(lo) == len(got) == int(off[-1]) and lo[0] == 3 and lo[int(off[2])] == 50 and lo[-1] == 8000 + 700
    assert np.array_equal(got, M.literal(data, lo, w, EDGES))


def test_model_is_numpy_histogram_on_finite_data():
    """numpy.histogram's bins are left closed except the last, which holds its right edge too: data that avoids the
    last edge (and every other one, for the right-closed side) makes the three agree"""
    rng = np.random.default_rng(53)
    x = rng.normal(0, 30, 3000)
    edges = np.array([-100.0, -30.0, -1.0, 0.0, 2.5, 40.0, 100.0])
    assert not np.isin(x, edges).any()
    for w in (1, 5, 64, 301):
        lo = np.arange(0, 3000 - w + 1, 37)
        for closed in (M.LEFT_CLOSED, M.RIGHT_CLOSED):
            got = M.rows(x, lo, w, edges, closed)
            for i, a in enumerate(lo):
                want = np.histogram(x[a:a + w], bins=edges)[0]
                assert got[i, 1:len(edges)].tolist() == want.tolist(), (w, a)
                assert got[i, 0] == (x[a:a + w] < edges[0]).sum() and got[i, len(edges)] == (x[a:a + w] > edges[-1]).sum()
                assert got[i, -1] == 0


def test_every_row_sums_to_w(data):
    for closed in (M.LEFT_CLOSED, M.RIGHT_CLOSED):
        for w, s in ((1, 1), (64, 3), (300, 7), (4096, 100)):
            got, off = M.rolling(data, [0, 4900], [N, 500 + w if 5400 + w <= N else N - 4900], w, s, EDGES, closed)
            assert len(got) and np.all(got.sum(axis=1) == w), (w, s)
    # the stretch of NaN: everything in the last counter; the flat stretch on an edge: one bin, which one by the side
    assert M.rows(data, [5000], 100, EDGES)[0].tolist() == [0] * (len(EDGES) + 1) + [100]
    assert M.rows(data, [7000], 50, EDGES, M.LEFT_CLOSED)[0, 5] == 50 and M.rows(data, [7000], 50, EDGES, M.RIGHT_CLOSED)[0, 4] == 50
    # -0.0 and 0.0 are one value against the edge 0.0
    assert M.rows(data, [7100], 10, EDGES, M.LEFT_CLOSED)[0, 3] == 10 and M.rows(data, [7100], 10, EDGES, M.RIGHT_CLOSED)[0, 2] == 10


def test_a_position_does_not_depend_on_range_or_stride(data):
    bins = M.stream_bins(data, EDGES)
    for w in (2, 65, 300, 2049):
        a, off_a = M.rolling(data, [0], [N], w, 1, EDGES, bins=bins)
        assert int(off_a[1]) == N - w + 1
        for begin, stride in ((1, 7), (5, w), (12, 2 * w + 1), (2048, 3)):
            b, off_b = M.rolling(data, [begin, 100], [N - begin, 50 + w], w, stride, EDGES, bins=bins)
            lo = begin + stride * np.arange(int(off_b[1]))
            assert np.array_equal(a[lo], b[: len(lo)]), (w, begin, stride)
            lo2 = 100 + stride * np.arange(int(off_b[2] - off_b[1]))
            assert np.array_equal(a[lo2], b[len(lo):]), (w, begin, stride)


def test_the_rule_that_sizes_a_task():
    """B = clamp(8 ceil(w / s), 64, 2048), by the width and the stride alone"""
    T = M.task_positions
    assert T(1, 1) == 64 and T(8, 1) == 64 and T(9, 1) == 72 and T(20, 1) == 160 and T(300, 15) == 160 and T(3600, 1) == 2048
    assert T(256, 1) == 2048 and T(255, 1) == 2040 and T(257, 1) == 2048 and T(1 << 20, 1) == 2048
    assert T(300, 7) == 8 * 43 and T(64, 8) == 64 and T(65, 8) == 72
    assert T(300, 300) == T(300, 301) == T(300, 1 << 40) == 64 and T(300, 299) == 64 and T(1 << 20, 1 << 10) == 2048 and T(1 << 20, 1 << 13) == 1024
    for w in (1, 20, 300, 3600, 70001, 1 << 20):
        for s in (1, 2, 7, 64, 65, 130, max(w - 1, 1), w, w + 1):
            b = T(w, s)
            assert 64 <= b <= 2048 and (b in (64, 2048) or b == 8 * -(-w // s))
            if s < w:  # a task's span stays far inside 32 bits, as the kernel's indices need
                assert (b - 1) * s + w < 1 << 27


def test_symbols_and_surfaces(A):
    lib = A.capi.lib()
    for name in ("atsc_rolling_histogram_windows_dev", "atsc_rolling_histogram_windows", "atsc_stream_rolling_histogram_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert A.ROLLING_MAX_WIDTH == M.MAX_WIDTH and A.HIST_MAX_EDGES == M.MAX_EDGES
    for owner, name in ((A.Context, "rolling_histogram_windows_host"), (A.DPlan, "rolling_histogram_windows"),
                        (A.CompressedStream, "rolling_histogram_windows"), (A, "rolling_histogram_data_windows")):
        assert getattr(owner, name).__doc__.strip()
