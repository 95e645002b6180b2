"""The windowed across histograms without a GPU: the vectorised NumPy model (tests/across_histogram_model.py) against a
scalar, line-by-line restatement of the rule; hand values (samples equal to an edge under both sides, -0.0 against an
edge of 0.0, +-Inf samples and +-Inf edges, all-NaN columns); rows sum to N, rows of sub-lists add to the whole list's
row, a permuted list gives the same bytes; the rule that sizes a pass of the kernel; the new symbols, the public surfaces
and the command line's argument errors (exit 2 before any GPU work)."""
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import across_histogram_model as M
from tests import across_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATSC = os.path.join(ROOT, "atsc_amd", "bin", "atsc")
NAN, INF = np.nan, np.inf
SIZES = [1, 2, 3, 5, 8, 9, 17, 33, 63, 64]
EDGE_SETS = [[0.0], [-1.0, 0.5], [-1000.0, -1.0, 0.0, 0.5, 4.25, 100.0, 1e5], [-INF, 0.0, INF], [-INF], [INF],
             list(np.linspace(-50.0, 50.0, 1024))]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _columns(rng, n, m):
    """(n, m): mixed magnitudes, both signs, NaN holes, values on the edges, zeros of both signs, +-Inf, a column of NaN"""
    x = rng.normal(0, 1, (n, m)) * 10.0 ** rng.integers(-3, 6, (n, m))
    x[rng.random((n, m)) < 0.1] = NAN
    on_edge = rng.random((n, m))
    x[on_edge < 0.05] = 4.25
    x[(on_edge >= 0.05) & (on_edge < 0.1)] = 0.0
    x[(on_edge >= 0.1) & (on_edge < 0.15)] = -0.0
    x[(on_edge >= 0.15) & (on_edge < 0.17)] = INF
    x[(on_edge >= 0.17) & (on_edge < 0.19)] = -INF
    x[(on_edge >= 0.19) & (on_edge < 0.21)] = -50.0
    x[:, m // 2] = NAN
    return x


def _scalar_row(column, edges, closed):
    """the rule, line by line, on one column"""
    row = [0] * (len(edges) + 2)
    for v in column:
        v = float(v)
        if v != v:
            row[len(edges) + 1] += 1
            continue
        k = 0
        for e in edges:
            if (e < v) if closed == M.RIGHT_CLOSED else (e <= v):
                k += 1
        row[k] += 1
    return row


@pytest.mark.parametrize("closed", (M.LEFT_CLOSED, M.RIGHT_CLOSED))
def test_model_equals_the_rule_line_by_line(closed):
    rng = np.random.default_rng(300 + closed)
    for n in SIZES:
        x = _columns(rng, n, 9)
        for edges in EDGE_SETS[:-1] + [list(np.linspace(-50.0, 50.0, 65))]:
            got = M.rows(x, edges, closed)
            assert got.dtype == np.uint64 and got.shape == (9, len(edges) + 2)
            want = [_scalar_row(x[:, p], edges, closed) for p in range(9)]
            assert got.tolist() == want, (n, len(edges))


def test_hand_values():
    L, R = M.LEFT_CLOSED, M.RIGHT_CLOSED
    col = np.array([[1.0, 2.0, 2.0, 3.0, 0.5, NAN]]).T
    assert M.rows(col, [1.0, 2.0, 3.0], L).tolist() == [[1, 1, 2, 1, 1]]  # an edge's sample goes above it
    assert M.rows(col, [1.0, 2.0, 3.0], R).tolist() == [[2, 2, 1, 0, 1]]  # and below it under `le`
    zeros = np.array([[-0.0, 0.0, -0.0]]).T  # -0.0 equals +0.0, against an edge of either sign
    for e in (0.0, -0.0):
        assert M.rows(zeros, [e], L).tolist() == [[0, 3, 0]] and M.rows(zeros, [e], R).tolist() == [[3, 0, 0]]
    inf = np.array([[INF, -INF, 1.0, NAN]]).T  # +-Inf samples are counted like any value, also against +-Inf edges
    assert M.rows(inf, [0.0], L).tolist() == [[1, 2, 1]]
    assert M.rows(inf, [-INF, INF], L).tolist() == [[0, 2, 1, 1]] and M.rows(inf, [-INF, INF], R).tolist() == [[1, 2, 0, 1]]
    for n in SIZES:  # all-NaN columns
        assert M.rows(np.full((n, 2), NAN), [0.0, 1.0]).tolist() == [[0, 0, 0, n]] * 2
    # `count by (job)(x > 0.9)`: one edge, RIGHT_CLOSED: bin 1
    x = np.array([[0.95, 0.2], [0.9, 0.91], [0.1, NAN]])
    assert M.rows(x, [0.9], R)[:, 1].tolist() == [1, 1]


@pytest.mark.parametrize("closed", (M.LEFT_CLOSED, M.RIGHT_CLOSED))
def test_rows_sum_add_and_ignore_the_order(closed):
    rng = np.random.default_rng(310 + closed)
    for n in SIZES:
        x = _columns(rng, n, 11)
        for edges in EDGE_SETS:
            whole = M.rows(x, edges, closed)
            assert np.all(whole.sum(axis=1) == n)
            assert np.array_equal(whole[:, -1], np.isnan(x).sum(axis=0))
            assert whole[5].tolist() == [0] * (len(edges) + 1) + [n]  # the column of NaN
            if n > 1:
                for cut in sorted({1, n // 2, n - 1}):
                    assert np.array_equal(M.rows(x[:cut], edges, closed) + M.rows(x[cut:], edges, closed), whole)
                singles = sum(M.rows(x[k:k + 1], edges, closed) for k in range(n))
                assert np.array_equal(singles, whole)
            assert M.rows(x[rng.permutation(n)], edges, closed).tobytes() == whole.tobytes()


def test_model_ranges(A):
    fulls = [np.arange(30.0), np.arange(30.0)[::-1].copy(), np.full(30, NAN)]
    got, off = M.across_histogram(fulls, [3, 0, 29, 5], [10, 0, 1, 15], [10.0, 20.0], 4)
    assert off.tolist() == [0, 3, 3, 4, 8] and got.shape == (8, 4) and got.dtype == np.uint64
    assert off.tolist() == A.across_offsets([10, 0, 1, 15], 4).tolist() == AM.offsets([10, 0, 1, 15], 4).tolist()
    # positions 3, 7, 11 | 29 | 5, 9, 13, 17: (p, 29 - p, NaN)
    assert got.tolist() == [[1, 0, 1, 1], [1, 0, 1, 1], [0, 2, 0, 1], [1, 0, 1, 1], [1, 0, 1, 1], [1, 0, 1, 1], [0, 2, 0, 1],
                            [0, 2, 0, 1]]
    empty, off = M.across_histogram(fulls, [], [], [1.0], 1)
    assert empty.shape == (0, 3) and off.tolist() == [0]


def test_the_rule_that_sizes_a_pass():
    """pitch = 4 (ceil((n_edges + 2) / 4) | 1) bytes, G = min(64, 14336 // pitch): the kernel file's head comment"""
    assert M.row_pitch(1) == 4 and M.row_pitch(2) == 4 and M.row_pitch(3) == 12 and M.row_pitch(10) == 12 and M.row_pitch(13) == 20
    assert M.rows_a_pass(1) == M.rows_a_pass(218) == 64 and M.rows_a_pass(219) == 62 and M.rows_a_pass(1024) == 13
    b = M.pass_boundaries()
    assert b[:2] == [218, 219] and all(1 <= e <= M.MAX_EDGES for e in b)
    for e in range(1, M.MAX_EDGES + 1):
        p, g = M.row_pitch(e), M.rows_a_pass(e)
        assert p >= e + 2 and p % 4 == 0 and (p // 4) % 2 == 1  # a row fits; an odd number of 4-byte banks
        assert 1 <= g <= 64 and 8 * e + 4 * g * p <= 65536  # a workgroup's LDS


def test_symbols_are_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_across_histogram_windows_dev", "atsc_across_histogram_windows", "atsc_stream_across_histogram_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name


def test_public_surfaces(A):
    want = {(A.Context, "across_histogram_windows_host"):
            "(self, records_list, begins, counts, edges, stride=1, closed=0, has_count=False)",
            (A.DPlan, "across_histogram_windows"):
            "(self, d_body, others, other_bodies, begins, counts, edges, d_out, stride=1, closed=0, stream=0)",
            (A.CompressedStream, "across_histogram_windows"): "(self, others, begins, counts, edges, stride=1, closed=0)",
            (A.stream, "across_histogram_data_windows"): "(ctx, bros, begins, counts, edges, stride=1, closed=0)"}
    assert A.capi.HIST_LEFT_CLOSED == 0 == M.LEFT_CLOSED and A.capi.HIST_RIGHT_CLOSED == M.RIGHT_CLOSED
    assert A.HIST_MAX_EDGES == M.MAX_EDGES and A.ACROSS_MAX_STREAMS == AM.MAX_STREAMS
    for (owner, name), sig in want.items():
        f = getattr(owner, name)
        assert str(inspect.signature(f)) == sig, name
        assert f.__doc__ and f.__doc__.strip()
    assert A.across_histogram_data_windows is A.stream.across_histogram_data_windows


def test_null_context_is_invalid(A):
    lib = A.capi.lib()
    assert lib.atsc_across_histogram_windows(None, 1, None, None, None, 0, None, None, 1, 1, None, 0, None) == A.capi.E_INVALID
    assert lib.atsc_across_histogram_windows_dev(None, 1, None, None, 0, None, None, 1, 1, None, 0, None, None) == A.capi.E_INVALID
    assert lib.atsc_stream_across_histogram_windows(None, 1, 0, None, None, 1, 1, None, 0, None) == A.capi.E_INVALID


def _run(argv):
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = "-1"  # exit 2 must come before any GPU work
    return subprocess.run(argv, capture_output=True, text=True, env=env, timeout=60)


def test_atsc_cli_argument_errors(A, tmp_path):
    f, other = str(tmp_path / "missing.bro"), str(tmp_path / "other.bro")
    across = ["-u", "--samples", "0:10", "--across", other]
    r = _run([ATSC, "-u", "--samples", "0:10", "--across-histogram", "0,1", f])  # the option without --across
    assert r.returncode == 2 and "'--across-histogram' needs '--across'" in r.stderr, r.stderr
    r = _run([ATSC, "-u", "--across-histogram", "0,1", f])
    assert r.returncode == 2 and "error:" in r.stderr, r.stderr
    for bad in ("1,0", "1,1", "nan", "", "0:1", "0:1:0", "5:1:4", "a,b"):  # --histogram's parser and its messages
        r = _run([ATSC, *across, "--across-histogram", bad, f])
        assert r.returncode == 2 and "for '--across-histogram': expected ascending edges E,E,.. or LO:HI:N" in r.stderr, (bad, r.stderr)
    r = _run([ATSC, *across, "--across-histogram", "0:1:1024", f])
    assert r.returncode == 2 and "for '--across-histogram': more than 1024 edges" in r.stderr, r.stderr
    r = _run([ATSC, *across, "--across-histogram", "0,1", "--histogram-closed", "middle", f])
    assert r.returncode == 2 and "'--histogram-closed': left or right" in r.stderr, r.stderr
    # --histogram keeps its meaning: it needs --buckets, and --across does not go with --buckets
    r = _run([ATSC, *across, "--histogram", "0,1", f])
    assert r.returncode == 2 and "--buckets" in r.stderr, r.stderr
    r = _run([ATSC, "--help"])
    assert "--across-histogram" in r.stdout + r.stderr and "h0 .. h<n_edges>,hnan" in r.stdout + r.stderr
    # a well-formed command line gets past the arguments (and fails on the missing file, not with a usage error)
    for spec in ("0.5", "-inf,0,inf", "0:100:20"):
        r = _run([ATSC, *across, "--across-stride", "3", "--across-moments", "--across-histogram", spec, "--histogram-closed",
                  "right", f])
        assert r.returncode != 2, r.stderr
    # csv-compressor has no --across, so none of its options
    r = _run([os.path.join(ROOT, "atsc_amd", "bin", "csv-compressor"), "--across-histogram", "0,1", f])
    assert r.returncode == 2, r.stderr
