"""CPU-only tests of the windowed histograms: the NumPy model of the contract (tests/hist_model.py) against
numpy.histogram where the two agree and on its edge cases, atsc_histogram_edges_uniform bit for bit against
numpy.linspace and its rejections, the C functions' null-argument checks and the command lines' argument errors (exit
2 before any GPU work)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import hist_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATSC = os.path.join(ROOT, "atsc_amd", "bin", "atsc")
CSV = os.path.join(ROOT, "atsc_amd", "bin", "csv-compressor")


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


# ---- the model ---------------------------------------------------------------------------------------------------
def test_model_matches_numpy_histogram_on_interior_samples():
    rng = np.random.default_rng(1)
    checked = 0
    for it in range(60):
        n_edges = int(rng.choice([2, 3, 17, 255, 1024]))
        edges = np.sort(rng.normal(0, 10, n_edges))
        if len(np.unique(edges)) != n_edges:
            continue
        x = rng.uniform(edges[0], edges[-1], int(rng.integers(1, 4000)))
        x = x[(x >= edges[0]) & (x < edges[-1])]  # numpy.histogram's last bin is closed on both sides: keep below it
        want, _ = np.histogram(x, bins=edges)
        got = M.row(x, edges, M.LEFT_CLOSED)
        assert got.dtype == np.uint64 and len(got) == n_edges + 2
        assert got[0] == 0 and got[n_edges] == 0 and got[n_edges + 1] == 0
        assert np.array_equal(got[1:n_edges], want.astype(np.uint64))
        assert got.sum() == len(x)
        checked += 1
    assert checked > 40


def test_model_sample_on_an_edge():
    edges = [1.0, 2.0, 3.0]
    x = [1.0, 2.0, 2.0, 3.0, 0.5, 3.5]
    assert list(M.row(x, edges, M.LEFT_CLOSED)) == [1, 1, 2, 2, 0]   # edges[k-1] <= v < edges[k]
    assert list(M.row(x, edges, M.RIGHT_CLOSED)) == [2, 2, 1, 1, 0]  # edges[k-1] < v <= edges[k]


def test_model_signed_zero_infinities_denormals():
    # -0.0 equals a 0.0 edge (and 0.0 a -0.0 edge): compared as values
    for edge in (0.0, -0.0):
        for v in (0.0, -0.0):
            assert list(M.row([v], [edge], M.LEFT_CLOSED)) == [0, 1, 0]
            assert list(M.row([v], [edge], M.RIGHT_CLOSED)) == [1, 0, 0]
    # +-Inf samples are counted like any other value
    x = [-np.inf, np.inf, 0.0, np.inf]
    assert list(M.row(x, [-1.0, 1.0], M.LEFT_CLOSED)) == [1, 1, 2, 0]
    assert list(M.row(x, [-1.0, 1.0], M.RIGHT_CLOSED)) == [1, 1, 2, 0]
    # +-Inf edges: a sample equal to the edge follows the closed side like any other
    e = [-np.inf, 0.0, np.inf]
    assert list(M.row(x, e, M.LEFT_CLOSED)) == [0, 1, 1, 2, 0]
    assert list(M.row(x, e, M.RIGHT_CLOSED)) == [1, 1, 2, 0, 0]
    # denormals order as values around a denormal edge
    d = 5e-324
    x = [-d, 0.0, d, 2 * d, 3 * d]
    assert list(M.row(x, [d, 3 * d], M.LEFT_CLOSED)) == [2, 2, 1, 0]
    assert list(M.row(x, [d, 3 * d], M.RIGHT_CLOSED)) == [3, 2, 0, 0]


def test_model_all_nan_and_empty():
    for closed in (M.LEFT_CLOSED, M.RIGHT_CLOSED):
        assert list(M.row(np.full(7, np.nan), [0.0, 1.0], closed)) == [0, 0, 0, 7]
        assert list(M.row([], [0.0, 1.0], closed)) == [0, 0, 0, 0]
        assert list(M.row([np.nan, 0.5, np.nan], [0.0, 1.0], closed)) == [0, 1, 0, 2]


def test_model_windows_paths_agree():
    rng = np.random.default_rng(2)
    full = rng.normal(0, 3, 5000)
    full[rng.integers(0, 5000, 300)] = np.nan
    b = rng.integers(0, 5000, 200)
    c = np.minimum(rng.integers(0, 400, 200), 5000 - b)
    edges = np.linspace(-4, 4, 17)
    for closed in (M.LEFT_CLOSED, M.RIGHT_CLOSED):
        slow = M.windows(full, b, c, edges, closed, prefix=False)
        assert np.array_equal(slow, M.windows(full, b, c, edges, closed, prefix=True))
        assert np.array_equal(slow.sum(axis=1), c.astype(np.uint64))


# ---- atsc_histogram_edges_uniform ----------------------------------------------------------------------------------
def _uniform(A, lo, hi, n):
    out = np.full(A.HIST_MAX_EDGES + 1, 7.0)
    rc = A.capi.lib().atsc_histogram_edges_uniform(float(lo), float(hi), int(n), out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out


def test_edges_uniform_equals_linspace(A):
    rng = np.random.default_rng(3)
    accepted = rejected = 0
    for it in range(6000):
        kind = it % 4
        if kind == 0:
            lo, hi = np.sort(rng.normal(0, 1, 2) * 10.0 ** int(rng.integers(-8, 9)))
        elif kind == 1:
            lo = float(rng.integers(-1000, 1000))
            hi = lo + float(rng.integers(1, 5000))
        elif kind == 2:  # a width of a few ulps of lo up to a few thousand
            lo = rng.normal(0, 1) * 10.0 ** int(rng.integers(-3, 17))
            hi = lo + abs(lo) * 2.0 ** -52 * float(rng.integers(1, 4000))
        else:
            lo, hi = np.sort(rng.uniform(-1e300, 1e300, 2))
        n = int(rng.integers(1, A.HIST_MAX_EDGES))
        rc, out = _uniform(A, lo, hi, n)
        with np.errstate(all="ignore"):
            want = np.linspace(lo, hi, n + 1)
        if rc == 0:
            assert np.array_equal(out[: n + 1].view(np.uint64), want.view(np.uint64)), (lo, hi, n)
            assert np.all(out[n + 1:] == 7.0)
            assert np.all(np.diff(out[: n + 1]) > 0)
            accepted += 1
        else:
            assert rc == A.capi.E_INVALID and np.all(out == 7.0), (lo, hi, n)
            assert not (hi > lo) or not np.all(np.diff(want) > 0), (lo, hi, n)  # only what is not ascending is refused
            rejected += 1
    assert accepted > 3000 and rejected > 20, (accepted, rejected)
    assert np.array_equal(A.histogram_edges_uniform(0.0, 1.0, 4), [0.0, 0.25, 0.5, 0.75, 1.0])
    assert len(A.histogram_edges_uniform(-3.0, 9.0, A.HIST_MAX_EDGES - 1)) == A.HIST_MAX_EDGES


def test_edges_uniform_rejections(A):
    inf, nan = np.inf, np.nan
    cases = [(nan, 1.0, 4), (0.0, nan, 4), (-inf, 1.0, 4), (0.0, inf, 4), (inf, inf, 4),  # not finite
             (1.0, 1.0, 4), (2.0, 1.0, 4), (0.0, -0.0, 4),                               # hi <= lo
             (0.0, 1.0, 0), (0.0, 1.0, A.HIST_MAX_EDGES), (0.0, 1.0, 2 ** 32 - 1),       # n_bins
             (0.0, 5e-324, 2),                                                           # a step of 0
             (1e16, 1e16 + 4, 8), (1.0, 1.0 + 2.0 ** -52, 2),                            # rounded edges not ascending
             (-1e308, 1e308, 3)]                                                         # hi - lo overflows
    for lo, hi, n in cases:
        rc, out = _uniform(A, lo, hi, n)
        assert rc == A.capi.E_INVALID and np.all(out == 7.0), (lo, hi, n, rc)
        with pytest.raises(A.AtscError):
            A.histogram_edges_uniform(lo, hi, n)
    assert A.capi.lib().atsc_histogram_edges_uniform(0.0, 1.0, 4, None) == A.capi.E_INVALID
    rc, out = _uniform(A, 1e16, 1e16 + 16, 8)
    assert rc == 0 and np.array_equal(out[:9], np.linspace(1e16, 1e16 + 16, 9))


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------
def test_null_arguments_are_invalid(A):
    L = A.capi.lib()
    one = (C.c_uint64 * 1)(0)
    edges = (C.c_double * 2)(0.0, 1.0)
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    body = (C.c_uint8 * 16)()
    assert L.atsc_histogram_windows_dev(None, None, None, 1, one, one, 2, edges, 0, C.cast(out, C.c_void_p), None) == A.capi.E_INVALID
    assert L.atsc_histogram_windows(None, body, 16, 0, 1, one, one, 2, edges, 0, out) == A.capi.E_INVALID
    assert L.atsc_stream_histogram_windows(None, 1, one, one, 2, edges, 0, out) == A.capi.E_INVALID
    assert list(out) == [7, 7, 7, 7]


def test_constants(A):
    assert (A.HIST_LEFT_CLOSED, A.HIST_RIGHT_CLOSED, A.HIST_MAX_EDGES) == (0, 1, 1024)
    assert (M.LEFT_CLOSED, M.RIGHT_CLOSED, M.MAX_EDGES) == (0, 1, 1024)
    hdr = open(os.path.join(ROOT, "include", "atsc_hip.h")).read()
    assert "ATSC_HIST_LEFT_CLOSED = 0, ATSC_HIST_RIGHT_CLOSED = 1" in hdr and "ATSC_HIST_MAX_EDGES = 1024" in hdr


# ---- the command lines' argument errors ----------------------------------------------------------------------------
def _run(argv):
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = "-1"  # exit 2 must come before any GPU work
    return subprocess.run(argv, capture_output=True, text=True, env=env, timeout=60)


BAD_SPECS = ["", "1,", ",1", "x", "1,abc", "nan", "1,nan", " 1", "2,1", "1,1", "0.0,-0.0", "inf,inf",  # explicit edges
             "0:1", "0:1:", ":1:4", "0::4", "0:1:x", "0:1:-4", "0:1:4:5", "0:1:0", "1:0:4", "1:1:4", "nan:1:4", "0:inf:4",
             "1e16:10000000000000004:8", "0:1:2.5"]                                                       # uniform
TOO_MANY = [",".join(str(k) for k in range(1025)), "0:1:1024", "0:1:99999999999"]


def _check_cli(prog, pre, needs, tmp_path):
    f = str(tmp_path / "missing.bro")
    r = _run([prog, "-u", "--histogram", "0,1", f])
    assert r.returncode == 2 and needs in r.stderr and "--histogram" in r.stderr, r.stderr
    r = _run([prog, "-u", *pre, "--histogram-closed", "right", f])
    assert r.returncode == 2 and "'--histogram-closed' needs '--histogram'" in r.stderr, r.stderr
    for bad in BAD_SPECS:
        r = _run([prog, "-u", *pre, "--histogram", bad, f])
        assert r.returncode == 2 and "for '--histogram'" in r.stderr, (bad, r.returncode, r.stderr)
    for bad in TOO_MANY:
        r = _run([prog, "-u", *pre, "--histogram", bad, f])
        assert r.returncode == 2 and "for '--histogram'" in r.stderr and "1024" in r.stderr, (bad[:40], r.returncode, r.stderr)
    for bad in ("", "both", "LEFT"):
        r = _run([prog, "-u", *pre, "--histogram", "0,1", "--histogram-closed", bad, f])
        assert r.returncode == 2 and "--histogram-closed" in r.stderr, (bad, r.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == []
    # accepted specs get past the argument checks: the missing input is what fails then
    for good in ("0", "-1,0,1", "-inf,0,inf", "0:1:4", "-5:5:1023", "1e16:10000000000000016:8",
                 ",".join(str(k) for k in range(1024))):
        r = _run([prog, "-u", *pre, "--histogram", good, "--histogram-closed", "right", f])
        assert r.returncode not in (0, 2), (good[:40], r.returncode, r.stderr)
    assert sorted(p.name for p in tmp_path.iterdir()) == []


def test_atsc_cli_histogram_argument_errors(A, tmp_path):
    _check_cli(ATSC, ["--buckets", "60"], "--buckets", tmp_path)


def test_csv_compressor_histogram_argument_errors(A, tmp_path):
    _check_cli(CSV, ["--from", "0", "--to", "100", "--step", "10"], "--step", tmp_path)
