"""CPU-only tests of the windowed deltas' host half: the NumPy model of the documented pairs, terms and summation order
(tests/delta_model.py) against exact rational arithmetic within the documented (L + 3) u bound, exactness on an integer
counter with resets, atsc_delta_derive bit for bit against its Python restatement, the new symbols, and the command
lines' usage errors."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import delta_model as M

LENGTHS = [2, 3, 5, 63, 64, 65, 255, 256, 257, 511, 2047, 2048, 2049, 4096, 5000, 12289, 40000]
BEGINS = [1, 1000, 2047, 2048, 12345, 3 * 2048 - 1, 4095]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _counter(rng, n):
    """an integer counter: steps of 0 .. 1000, and a restart at a small value about every 500 samples"""
    steps = rng.integers(0, 1000, n).astype(np.float64)
    x = np.empty(n)
    v = 0.0
    for i in range(n):
        v = float(rng.integers(0, 50)) if rng.random() < 0.002 else v + steps[i]
        x[i] = v
    return x


def _inputs(rng, n):
    """the inputs the bound was stated on: N(0, 1); 1e9 +- 1e-3; a random walk; an integer counter with resets; 20 %
    NaN"""
    holes = rng.normal(0, 1, n)
    holes[rng.random(n) < 0.2] = np.nan
    return {"normal": rng.normal(0, 1, n), "offset1e9": 1e9 + rng.normal(0, 1e-3, n),
            "walk": np.cumsum(rng.normal(0, 1, n)), "counter": _counter(rng, n), "nan20": holes}


def _cases():
    """every length and input at the stream's start and at a begin further in"""
    rng = np.random.default_rng(83)
    for k, n in enumerate(LENGTHS):
        for begin in (0, BEGINS[k % len(BEGINS)]):
            for name, v in _inputs(rng, n).items():
                x = np.concatenate([np.full(begin, 1e300), v, rng.normal(-5, 100, 7)])  # the outside must not matter
                yield name, begin, n, x


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_model_within_bound_of_exact():
    worst = 0.0
    for name, begin, count, x in _cases():
        pairs, rises, falls, up, down, after, max_rise, max_fall = M.window_delta(x, begin, count)
        v = x[begin:begin + count]
        e_pairs, e_up, e_down, e_after = M.exact_delta(v)
        assert pairs == e_pairs and rises + falls <= pairs, (name, begin, count)
        if name != "nan20":
            assert pairs == count - 1, (name, begin, count)
        k = M.bound_factor(pairs)
        for what, got, want in (("up", up, e_up), ("down", down, e_down)):
            err = abs(Fraction(got) - want)
            assert err <= Fraction(k) * want, (name, begin, count, what, float(err), k * float(want))
            if want:
                worst = max(worst, float(err / (Fraction(k) * want)))
        assert (rises == 0) == (e_up == 0) and (falls == 0) == (e_down == 0), (name, begin, count)
        assert up >= 0 and down >= 0 and max_rise >= 0 and max_fall >= 0
        assert max_rise <= up and max_fall <= down, (name, begin, count)  # rounding is monotone
        if name == "counter":  # integers below 2^53 in sum: every subtract and every addition is exact
            assert Fraction(up) == e_up and Fraction(down) == e_down and Fraction(after) == e_after, (begin, count)
            assert M.derive(pairs, rises, falls, up, down, after)[2] == v[-1] - v[0]  # net = last - first
    print("largest error / bound:", worst)
    assert worst < 1.0


def test_counter_increase_across_resets():
    """what the record is for: a counter that restarts from zero twice; last - first is wrong, increase is not"""
    x = np.array([5.0, 9, 9, 12, 2, 3, 10, 0, 4, np.nan, 6, 7])
    d = M.window_delta(x, 0, len(x))
    assert d == (9, 6, 2, 4 + 3 + 1 + 7 + 4 + 1, 10 + 10, 2 + 0, 7.0, 10.0)
    changes, variation, net, increase, mean_step = M.derive(*d)
    assert (changes, variation, net, increase) == (8, 40.0, 0.0, 22.0) and mean_step == 40.0 / 9
    # the window's own first slot holds no pair, and nothing reaches across the NaN or in from outside
    assert M.window_delta(x, 4, 4) == (3, 2, 1, 8.0, 10.0, 0.0, 7.0, 10.0)
    assert M.window_delta(x, 8, 3) == (0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    for c in (0, 1):
        assert M.window_delta(x, 3, c) == (0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    z = np.array([-0.0, 0.0, np.inf, np.inf, -np.inf, 1.0])
    p, r, f, up, down, after, mr, mf = M.window_delta(z, 0, 6)
    assert (p, r, f) == (5, 2, 1) and up == np.inf and down == np.inf and after == -np.inf and mr == mf == np.inf
    assert all(_bits(q) == 0 for q in M.window_delta(z, 0, 2)[3:])  # a sum without a term is +0.0


def test_model_ignores_what_lies_outside_the_window():
    rng = np.random.default_rng(89)
    x = rng.normal(0, 1, 9000)
    y = x.copy()
    y[:1000] = 1e300
    y[3000:] = np.nan
    a, b = M.window_delta(x, 1000, 2000), M.window_delta(y, 1000, 2000)
    assert [_bits(q) for q in a[3:]] == [_bits(q) for q in b[3:]] and a[:3] == b[:3] and a[0] == 1999


def test_delta_dtypes(A):
    assert A.WINDOW_DELTA.itemsize == 64 and A.WINDOW_DELTA.names == M.FIELDS
    assert A.WINDOW_DELTA_FIT.itemsize == 40 and A.WINDOW_DELTA_FIT.names == M.FIT_FIELDS


def test_symbols_exported_and_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_delta_windows_dev", "atsc_delta_windows", "atsc_stream_delta_windows", "atsc_delta_derive"):
        assert name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert callable(A.Context.delta_windows_host) and callable(A.DPlan.delta_windows)
    assert callable(A.CompressedStream.delta_windows) and callable(A.delta_data_windows) and callable(A.delta_derive)


def test_delta_derive_bit_for_bit(A):
    rng = np.random.default_rng(97)
    inf, nan = float("inf"), float("nan")
    rows = [(0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0), (0, 3, 4, 1.0, 2.0, 3.0, 4.0, 5.0), (1, 1, 0, 2.5, 0.0, 0.0, 2.5, 0.0),
            (1, 0, 1, 0.0, 2.5, -7.0, 0.0, 2.5), (9, 6, 2, 20.0, 20.0, 2.0, 7.0, 10.0), (3, 1, 1, inf, inf, -inf, inf, inf),
            (3, 1, 1, inf, 1.0, nan, inf, 1.0), (5, 2, 2, 1e308, 1e308, 1e308, 1e308, 1e308),
            (7, 3, 3, 0.1, 0.2, 0.3, 0.1, 0.2), (2 ** 53 + 2, 2 ** 63, 2 ** 63, 0.1, 0.3, 1.5, 0.1, 0.3),
            (6, 2, 2, 1e-320, 1e-321, -0.0, 1e-320, 1e-321), (4, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)]
    for _ in range(300):
        p = int(rng.integers(1, 100000))
        r = int(rng.integers(0, p + 1))
        rows.append((p, r, int(rng.integers(0, p - r + 1)), abs(rng.normal(0, 1e3)), abs(rng.normal(0, 1e3)),
                     rng.normal(0, 1e4), abs(rng.normal(0, 10)), abs(rng.normal(0, 10))))
    d = np.zeros(len(rows), dtype=A.WINDOW_DELTA)
    for i, r in enumerate(rows):
        d[i] = r
    got = A.delta_derive(d)
    assert got.dtype == A.WINDOW_DELTA_FIT and len(got) == len(rows)
    for r, g in zip(rows, got):
        want = M.derive(*r)
        assert int(g["changes"]) == want[0], (r, g)
        for name, w in zip(M.FIT_FIELDS[1:], want[1:]):
            assert (np.isnan(w) and np.isnan(g[name])) or _bits(w) == _bits(g[name]), (r, name, w, g[name])
    assert np.isnan(got[0]["mean_step"]) and np.isnan(got[1]["mean_step"])  # pairs == 0, whatever the other fields hold
    assert got[0]["variation"] == 0.0 and got[1]["variation"] == 3.0 and int(got[1]["changes"]) == 7
    assert got[4]["increase"] == 22.0 and got[4]["net"] == 0.0 and got[4]["mean_step"] == 40.0 / 9
    assert np.isnan(got[5]["net"]) and got[5]["variation"] == inf and np.isnan(got[5]["increase"])
    assert int(got[9]["changes"]) == 0  # 64-bit unsigned, as C adds them
    assert len(A.delta_derive(np.zeros(0, dtype=A.WINDOW_DELTA))) == 0
    lib = A.capi.lib()
    out = np.zeros(1, dtype=A.WINDOW_DELTA_FIT)
    assert lib.atsc_delta_derive(None, 1, C.c_void_p(out.ctypes.data)) == A.capi.E_INVALID
    assert lib.atsc_delta_derive(C.c_void_p(d.ctypes.data), 1, None) == A.capi.E_INVALID
    assert lib.atsc_delta_derive(None, 0, None) == 0


def test_command_line_usage_errors(A, tmp_path):
    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    f = tmp_path / "x.bro"
    f.write_bytes(b"")
    for cmd, msg in (([atsc, "-u", "--deltas", str(f)], "error: '--deltas' needs '--buckets'"),
                     ([atsc, "--deltas", str(f)], "error: '--deltas' needs '--buckets'"),
                     ([atsc, "--buckets", "5", "--deltas", str(f)], "error: '--buckets' needs '-u'"),
                     ([csvc, "-u", "--deltas", str(f)], "error: '--deltas' needs '--step'"),
                     ([csvc, "-u", "--from", "0", "--to", "10", "--deltas", str(f)], "error: '--deltas' needs '--step'"),
                     ([csvc, "--deltas", str(f)], "error: '--deltas' needs '--step'")):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (cmd, r.stderr)
        assert msg in r.stderr, (cmd, r.stderr)
    for exe in (atsc, csvc):
        r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--deltas" in r.stderr and "variation" in r.stderr, exe
