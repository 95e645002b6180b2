"""CPU-only tests of the windowed select's host half: the NumPy model of the contract (tests/select_model.py) against a
plain Python loop over the samples, the block's size, the new symbols and dtype, and the command lines' usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import select_model as M

inf, nan = float("inf"), float("nan")


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _hit(x, op, limit):
    """the condition on one sample, in plain Python"""
    if x != x:
        return False
    return {M.GT: x > limit, M.GE: x >= limit, M.LT: x < limit, M.LE: x <= limit, M.EQ: x == limit,
            M.NE: x != limit}[op]


def _loop(full, wins, op, limit, cap):
    """-> (offsets, [(value bits, at)]) by a loop over the samples"""
    off, ent = [0], []
    for b, c in wins:
        k = 0
        for j in range(c):
            x = float(full[b + j])
            if _hit(x, op, limit):
                ent.append((int(_bits(x)), j))
                k += 1
        off.append(off[-1] + k)
    return off, ent[:cap]


def _same(got, want):
    off, ent = got
    assert off.dtype == np.uint64 and ent.dtype == M.DTYPE
    assert off.tolist() == want[0]
    assert list(zip(_bits(ent["value"]).tolist(), ent["at"].tolist())) == want[1]


def test_model_against_a_plain_loop():
    rng = np.random.default_rng(211)
    seen_cut = seen_whole = 0
    for kind in range(4):
        for n in (0, 1, 5, 64, 300):
            v = rng.choice([0.0, 1.0, 2.5, -3.0], n)
            limits = [1.0, 0.5]
            if kind == 1:  # NaN holes
                v[rng.random(n) < 0.2] = nan
            elif kind == 2:  # -0.0 / +0.0 against limit 0.0
                v = rng.choice([0.0, -0.0, 1.0, -1.0], n)
                limits = [0.0, -0.0]
            elif kind == 3:  # +-Inf samples and limits
                v[rng.random(n) < 0.2] = inf
                v[rng.random(n) < 0.2] = -inf
                limits = [inf, -inf, 0.5]
            wins = [(0, n), (0, 0), (n // 2, n - n // 2), (n, 0), (n // 3, n // 3), (0, n)]  # empty ones, overlaps
            for op in M.OPS:
                for limit in limits:
                    total = _loop(v, wins, op, limit, 10 ** 9)[0][-1]
                    for cap in sorted({0, 1, total // 2, max(total - 1, 0), total, total + 5}):
                        _same(M.windows_select(v, wins, op, limit, cap), _loop(v, wins, op, limit, cap))
                        seen_cut += cap < total
                        seen_whole += cap >= total > 0
    assert seen_cut > 100 and seen_whole > 100
    # the contract's own examples
    z = np.array([-0.0, 0.0, 1.0, nan, -0.0])
    off, e = M.windows_select(z, [(0, 5)], M.EQ, 0.0, 9)
    assert off.tolist() == [0, 3] and e["at"].tolist() == [0, 1, 4]
    assert _bits(e["value"]).tolist() == [1 << 63, 0, 1 << 63]  # the -0.0 comes back as -0.0
    off, e = M.windows_select(z, [(0, 5)], M.NE, 0.0, 9)
    assert off.tolist() == [0, 1] and e["at"].tolist() == [2]  # NaN is not selected under NE either
    off, e = M.windows_select(z, [(1, 0), (2, 3), (0, 0)], M.GE, -0.0, 1)
    assert off.tolist() == [0, 0, 2, 2] and e["at"].tolist() == [0]  # cap cuts the entries, not the offsets
    w = np.array([inf, 1.0, -inf, inf])
    assert M.windows_select(w, [(0, 4)], M.GT, -inf, 9)[1]["at"].tolist() == [0, 1, 3]
    assert M.windows_select(w, [(0, 4)], M.GT, inf, 9)[0].tolist() == [0, 0]
    assert M.windows_select(w, [(0, 4)], M.GE, inf, 9)[1]["at"].tolist() == [0, 3]
    assert M.windows_select(w, [(0, 4)], M.LE, -inf, 9)[1]["at"].tolist() == [2]
    assert M.windows_select(w, [], M.GT, 0.0, 9)[0].tolist() == [0]


def test_select_bytes_and_dtype(A):
    assert A.SELECTED.itemsize == 16 and A.SELECTED.names == ("value", "at") and A.SELECTED == M.DTYPE
    assert A.select_bytes(0, 0) == 8 and A.select_bytes(1, 0) == 16 and A.select_bytes(3, 5) == 8 * 4 + 16 * 5
    assert A.select_bytes(2 ** 32 - 2, 2 ** 40) == 8 * (2 ** 32 - 1) + 16 * 2 ** 40
    import atsc_amd.engine as E

    assert E._SELECT.block(7, E._SELECT.params(A.RUNS_GT, 0.5, 11)) == A.select_bytes(7, 11)
    assert (A.RUNS_GT, A.RUNS_GE, A.RUNS_LT, A.RUNS_LE, A.RUNS_EQ, A.RUNS_NE) == M.OPS
    with pytest.raises(ValueError):
        E._SELECT.params(A.RUNS_GT, 0.5, -1)


def test_symbols_exported_and_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_select_windows_dev", "atsc_select_windows", "atsc_stream_select_windows"):
        assert name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert A.capi.SIGNATURES["atsc_select_windows_dev"][1][6:9] == [C.c_int, C.c_double, C.c_uint64]
    assert A.capi.SIGNATURES["atsc_select_windows"][1][7:10] == [C.c_int, C.c_double, C.c_uint64]
    assert A.capi.SIGNATURES["atsc_stream_select_windows"][1][4:7] == [C.c_int, C.c_double, C.c_uint64]
    assert callable(A.Context.select_windows_host) and callable(A.DPlan.select_windows)
    assert callable(A.CompressedStream.select_windows) and callable(A.select_data_windows)


def test_command_line_usage_errors(A, tmp_path):
    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    f = tmp_path / "x.bro"
    f.write_bytes(b"")
    wants = "'--where' wants OP:LIMIT"
    cases = [([atsc, "-u", "--where", "gt:1", str(f)], "error: '--where' needs '--samples'"),
             ([atsc, "--where=gt:1", str(f)], "error: '--where' needs '--samples'"),
             ([atsc, "--samples", "0:5", "--where", "gt:1", str(f)], "error: '--samples' needs '-u'"),
             ([atsc, "-u", "--samples", "0:5", "--buckets", "2", "--where", "gt:1", str(f)],
              "error: '--where' cannot be used with '--buckets'"),
             ([atsc, "-u", "--buckets", "2", "--where", "gt:1", str(f)], "error: '--where' needs '--samples'"),
             ([csvc, "-u", "--where", "le:0.5", str(f)], "error: '--where' needs '--from' and '--to'"),
             ([csvc, "--where", "le:0.5", str(f)], "error: '--where' needs '--from' and '--to'"),
             ([csvc, "-u", "--from", "0", "--to", "10", "--step", "5", "--where", "le:0.5", str(f)],
              "error: '--where' cannot be used with '--step'")]
    for bad in ("above:1", "gt", "gt:", "gt:nan", "gt:1x", "gt:1:2", "GT:1", ":1", "gt: 1"):
        cases.append(([atsc, "-u", "--samples", "0:5", "--where", bad, str(f)], wants))
        cases.append(([csvc, "-u", "--from", "0", "--to", "10", "--where=" + bad, str(f)], wants))
    for cmd, msg in cases:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (cmd, r.stderr)
        assert msg in r.stderr and "error:" in r.stderr, (cmd, r.stderr)
    for exe in (atsc, csvc):
        r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--where" in r.stderr and ".sel.csv" in r.stderr, exe
