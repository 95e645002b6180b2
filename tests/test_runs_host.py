"""CPU-only tests of the windowed runs' host half: the NumPy model of the contract (tests/runs_model.py) against an
independent itertools.groupby scan, `excess` against exact rational arithmetic within the documented (L + 3) u bound,
atsc_runs_merge (the C function) against the model's merge rule and against the union window's own record, the new
symbols, and the command lines' usage errors."""
import ctypes as C
import itertools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import runs_model as M
from tests.test_delta_host import BEGINS, LENGTHS, _inputs

DENSITIES = [0.0, 0.2, 0.5, 0.8, 1.0]
inf, nan = float("inf"), float("nan")


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _bits(x):
    return np.float64(x).view(np.uint64)


def _inside(x, op, limit):
    """the condition on one sample, in plain Python"""
    if x != x:
        return False
    return {M.GT: x > limit, M.GE: x >= limit, M.LT: x < limit, M.LE: x <= limit, M.EQ: x == limit,
            M.NE: x != limit}[op]


def _scan(v, op, limit):
    """-> the nine integers of the window v by a scan over the groups of equal condition"""
    n = len(v)
    if n == 0:
        return M.EMPTY[:9]
    runs, pos = [], 0
    for inside, grp in itertools.groupby(v, key=lambda q: _inside(float(q), op, limit)):
        k = len(list(grp))
        if inside:
            runs.append((pos, k))
        pos += k
    if not runs:
        return n, 0, 0, 0, M.NONE, M.NONE, M.NONE, 0, 0
    best = max(k for _, k in runs)
    return (n, sum(k for _, k in runs), len(runs), best, next(p for p, k in runs if k == best), runs[0][0],
            runs[-1][0] + runs[-1][1] - 1, runs[0][1] if runs[0][0] == 0 else 0,
            runs[-1][1] if runs[-1][0] + runs[-1][1] == n else 0)


def test_model_against_an_independent_scan():
    rng = np.random.default_rng(101)
    seen_many = seen_none = 0
    for k, n in enumerate(LENGTHS):
        for begin in (0, BEGINS[k % len(BEGINS)]):
            for dens in DENSITIES:
                for op in M.OPS:
                    # values 0 / 1 with the wanted density of `x OP 0.5`-like conditions, then the special values
                    v = (rng.random(n) < dens).astype(np.float64)
                    limit = 0.5
                    kind = (k + op) % 4
                    if kind == 1:  # NaN holes
                        v[rng.random(n) < 0.1] = nan
                    elif kind == 2:  # -0.0 / +0.0 against limit 0.0
                        v = np.where(v > 0, rng.choice([1.0, -1.0], n), rng.choice([0.0, -0.0], n))
                        limit = 0.0
                    elif kind == 3:  # +-Inf samples, and an infinite limit every other time
                        v[rng.random(n) < 0.1] = inf
                        v[rng.random(n) < 0.1] = -inf
                        limit = (inf, -inf, 0.5)[(k + begin) % 3]
                    x = np.concatenate([np.full(begin, 1.0), v, np.full(5, 1.0)])  # the outside must not matter
                    got = M.window_runs(x, begin, n, op, limit)
                    assert got[:9] == _scan(v, op, limit), (n, begin, dens, op, limit)
                    seen_many += got[2] > 1
                    seen_none += got[2] == 0
                    if got[1] == 0:
                        assert _bits(got[9]) == 0
    assert seen_many > 100 and seen_none > 100
    # the contract's own examples
    z = np.array([-0.0, 0.0, 1.0, nan, 0.0])
    assert M.window_runs(z, 0, 5, M.EQ, 0.0)[:9] == (5, 3, 2, 2, 0, 0, 4, 2, 1)
    assert M.window_runs(z, 0, 5, M.GT, 0.0)[:9] == (5, 1, 1, 1, 2, 2, 2, 0, 0)
    assert M.window_runs(z, 0, 5, M.GE, -0.0)[:9] == (5, 4, 2, 3, 0, 0, 4, 3, 1)
    assert M.window_runs(z, 0, 5, M.NE, 7.0)[:9] == (5, 4, 2, 3, 0, 0, 4, 3, 1)  # NaN is not inside under NE either
    assert M.window_runs(z, 1, 0, M.GT, 0.0) == M.EMPTY
    w = np.array([inf, 1.0, -inf, inf])
    assert M.window_runs(w, 0, 4, M.GT, -inf)[:9] == (4, 3, 2, 2, 0, 0, 3, 2, 1)
    assert M.window_runs(w, 0, 4, M.GT, inf)[:9] == (4, 0, 0, 0, M.NONE, M.NONE, M.NONE, 0, 0)
    assert np.isnan(M.window_runs(w, 0, 4, M.GE, inf)[9]) and M.window_runs(w, 0, 4, M.LT, inf)[9] == inf
    full = M.window_runs(np.ones(5000), 100, 4000, M.EQ, 1.0)
    assert full == (4000, 4000, 1, 4000, 0, 0, 3999, 4000, 4000, 0.0)


def test_excess_within_bound_of_exact():
    rng = np.random.default_rng(103)
    worst = 0.0
    for k, n in enumerate(LENGTHS):
        for begin in (0, BEGINS[k % len(BEGINS)]):
            for name, v in _inputs(rng, n).items():
                x = np.concatenate([np.full(begin, 1e300), v, rng.normal(-5, 100, 7)])
                limit = float(np.nanmedian(v))
                for op in (M.GT, M.LE, M.NE):
                    rec = M.window_runs(x, begin, n, op, limit)
                    inside, want = M.exact_excess(v, op, limit)
                    assert rec[1] == inside, (name, begin, n, op)
                    f = Fraction(M.bound_factor(inside))
                    err = abs(Fraction(rec[9]) - want)
                    assert err <= f * want, (name, begin, n, op, float(err), float(f * want))
                    if want:
                        worst = max(worst, float(err / (f * want)))
    print("largest error / bound:", worst)
    assert worst < 1.0


def _record(A, t):
    r = np.zeros(1, dtype=A.WINDOW_RUNS)
    r[0] = t
    return r[0]


def _same(got, want, what):
    for name, w in zip(M.FIELDS[:9], want[:9]):
        assert int(got[name]) == w, (what, name, int(got[name]), w)
    w = want[9]
    assert (np.isnan(w) and np.isnan(got["excess"])) or _bits(w) == _bits(got["excess"]), (what, w, got["excess"])


def test_runs_merge_against_the_model(A):
    rng = np.random.default_rng(107)
    for it in range(400):
        n = int(rng.integers(0, 400))
        dens = DENSITIES[it % 5]
        x = (rng.random(n) < dens).astype(np.float64) * rng.choice([1.0, 2.5, 0.1], n)
        if it % 4 == 0:
            x[rng.random(n) < 0.05] = nan
        parts = int(rng.integers(1, 7))
        cuts = np.sort(rng.integers(0, n + 1, parts - 1)) if n else np.zeros(parts - 1, dtype=np.int64)
        if it % 3 == 0 and parts > 2:
            cuts[1] = cuts[0]  # an empty part
        edges = [0] + [int(c) for c in cuts] + [n]
        recs = [M.window_runs(x, a, b - a, M.GT, 0.0) for a, b in zip(edges[:-1], edges[1:])]
        arr = np.zeros(len(recs), dtype=A.WINDOW_RUNS)
        for i, r in enumerate(recs):
            arr[i] = r
        got = A.runs_merge(arr)
        whole = M.window_runs(x, 0, n, M.GT, 0.0)
        assert tuple(int(got[k]) for k in M.FIELDS[:9]) == whole[:9], (it, edges)  # the union window's nine integers
        _same(got, M.merge_all(recs), (it, edges))  # and the excess as the left-to-right sum, bit for bit


def test_runs_merge_ties_and_u64(A):
    # a run of 3 in a at offset 1; a.tail 1 + b.head 2 joins to 3 as well: the earlier one stays
    a = (6, 4, 2, 3, 1, 1, 5, 0, 1, 4.0)
    b = (5, 3, 2, 2, 0, 0, 4, 2, 1, 3.0)
    _same(A.runs_merge([_record(A, a), _record(A, b)]), (11, 7, 3, 3, 1, 1, 10, 0, 1, 7.0), "a ties with the joined run")
    # the joined run (1 + 2 = 3, at 5) ties with a run of 3 later in b: the joined one stays
    a2 = (6, 1, 1, 1, 5, 5, 5, 0, 1, 1.0)
    b2 = (9, 5, 2, 3, 5, 0, 7, 2, 0, 5.0)
    _same(A.runs_merge([_record(A, a2), _record(A, b2)]), (15, 6, 2, 3, 5, 5, 13, 0, 0, 6.0), "joined ties with b")
    # strictly longer replaces: b's run of 4
    b3 = (9, 6, 2, 4, 4, 0, 7, 2, 0, 6.0)
    _same(A.runs_merge([_record(A, a2), _record(A, b3)]), (15, 7, 2, 4, 10, 5, 13, 0, 0, 7.0), "b is longer")
    # all-inside parts chain head and tail through; none-inside parts cut them
    full = (4, 4, 1, 4, 0, 0, 3, 4, 4, 2.0)
    none = (3, 0, 0, 0, M.NONE, M.NONE, M.NONE, 0, 0, 0.0)
    empty = M.EMPTY
    _same(A.runs_merge([_record(A, t) for t in (full, empty, full, full)]), (12, 12, 1, 12, 0, 0, 11, 12, 12, 6.0), "full")
    _same(A.runs_merge([_record(A, t) for t in (full, none, full)]), (11, 8, 2, 4, 0, 0, 10, 4, 4, 4.0), "none between")
    _same(A.runs_merge([_record(A, t) for t in (none, none)]), (6, 0, 0, 0, M.NONE, M.NONE, M.NONE, 0, 0, 0.0), "none")
    _same(A.runs_merge([_record(A, t) for t in (empty, empty)]), empty, "empty parts")
    _same(A.runs_merge(np.zeros(0, dtype=A.WINDOW_RUNS)), empty, "n == 0")
    # 64-bit unsigned arithmetic, as C does it
    big = 2 ** 63
    ha = (big, big, 1, big, 0, 0, big - 1, big, big, 1.0)
    got = A.runs_merge([_record(A, ha), _record(A, ha)])
    _same(got, M.merge(ha, ha), "u64")
    assert int(got["samples"]) == 0 and int(got["runs"]) == 1 and int(got["last_at"]) == 2 ** 64 - 1
    # excess: one add per record, left to right
    e = [(2, 2, 1, 2, 0, 0, 1, 2, 2, v) for v in (0.1, 0.2, 0.3, 1e16, -1e16 + 2)]
    got = A.runs_merge([_record(A, t) for t in e])
    want = np.float64(0.1)
    for v in (0.2, 0.3, 1e16, -1e16 + 2):
        want = want + np.float64(v)
    assert _bits(got["excess"]) == _bits(want) and int(got["longest"]) == 10
    lib = A.capi.lib()
    out = np.zeros(1, dtype=A.WINDOW_RUNS)
    out["samples"] = 77
    r = np.zeros(1, dtype=A.WINDOW_RUNS)
    assert lib.atsc_runs_merge(None, 1, C.c_void_p(out.ctypes.data)) == A.capi.E_INVALID
    assert lib.atsc_runs_merge(C.c_void_p(r.ctypes.data), 1, None) == A.capi.E_INVALID
    assert int(out["samples"][0]) == 77
    assert lib.atsc_runs_merge(None, 0, C.c_void_p(out.ctypes.data)) == 0
    _same(out[0], empty, "n == 0, null records")


def test_runs_dtype_and_constants(A):
    assert A.WINDOW_RUNS.itemsize == 80 and A.WINDOW_RUNS.names == M.FIELDS
    assert (A.RUNS_GT, A.RUNS_GE, A.RUNS_LT, A.RUNS_LE, A.RUNS_EQ, A.RUNS_NE) == M.OPS
    assert A.RUNS_NONE == M.NONE == 2 ** 64 - 1
    import atsc_amd.engine as E

    assert E.WINDOW_RUNS is A.WINDOW_RUNS and E.RUNS_NE == 5 and E.RUNS_NONE == M.NONE


def test_symbols_exported_and_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_runs_windows_dev", "atsc_runs_windows", "atsc_stream_runs_windows", "atsc_runs_merge"):
        assert name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert A.capi.SIGNATURES["atsc_runs_windows_dev"][1][6:8] == [C.c_int, C.c_double]
    assert A.capi.SIGNATURES["atsc_runs_windows"][1][7:9] == [C.c_int, C.c_double]
    assert A.capi.SIGNATURES["atsc_stream_runs_windows"][1][4:6] == [C.c_int, C.c_double]
    assert callable(A.Context.runs_windows_host) and callable(A.DPlan.runs_windows)
    assert callable(A.CompressedStream.runs_windows) and callable(A.runs_data_windows) and callable(A.runs_merge)


def test_command_line_usage_errors(A, tmp_path):
    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    f = tmp_path / "x.bro"
    f.write_bytes(b"")
    wants = "'--runs' wants OP:LIMIT"
    cases = [([atsc, "-u", "--runs", "gt:1", str(f)], "error: '--runs' needs '--buckets'"),
             ([atsc, "--runs=gt:1", str(f)], "error: '--runs' needs '--buckets'"),
             ([atsc, "--buckets", "5", "--runs", "gt:1", str(f)], "error: '--buckets' needs '-u'"),
             ([csvc, "-u", "--runs", "le:0.5", str(f)], "error: '--runs' needs '--step'"),
             ([csvc, "-u", "--from", "0", "--to", "10", "--runs", "le:0.5", str(f)], "error: '--runs' needs '--step'"),
             ([csvc, "--runs", "le:0.5", str(f)], "error: '--runs' needs '--step'")]
    for bad in ("above:1", "gt", "gt:", "gt:nan", "gt:1x", "gt:1:2", "GT:1", ":1", "gt: 1"):
        cases.append(([atsc, "-u", "--buckets", "5", "--runs", bad, str(f)], wants))
        cases.append(([csvc, "-u", "--from", "0", "--to", "10", "--step", "5", "--runs=" + bad, str(f)], wants))
    for cmd, msg in cases:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (cmd, r.stderr)
        assert msg in r.stderr, (cmd, r.stderr)
    for exe in (atsc, csvc):
        r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--runs" in r.stderr, exe
        for col in ("inside", "longest_at", "first_at", "last_at", "head", "tail", "excess"):
            assert col in r.stderr, (exe, col)
