"""CPU-only tests of the windowed extremes' host half: the NumPy model of the contract (tests/extremes_model.py) against a
brute-force Python sort, the two kernels' selection (written as plain functions over k_ext_tiles' slot-to-lane mapping
and k_ext_combine's pop order) against the model, atsc_extremes_merge (the C function) against the model's merge and
against the union window's own record bit for bit, the record's dtype, the new symbols and callables, and the command
lines' usage errors."""
import ctypes as C
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import extremes_model as M

inf, nan = float("inf"), float("nan")
SPECIAL = [0.0, -0.0, nan, 1.0, -1.0, inf, -inf, 2.5, 1.0, 5e-324, -5e-324]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _brute(v, k, largest):
    """positions of the k first non-NaN samples by value (descending if largest), equal values earliest first"""
    def cmp(a, b):
        x, y = v[a], v[b]
        if x != y:  # as values: -0.0 == +0.0
            return -1 if ((x > y) if largest else (x < y)) else 1
        return a - b

    return sorted([i for i in range(len(v)) if v[i] == v[i]], key=functools.cmp_to_key(cmp))[:k]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _check_record(r, v, k, what):
    v = [float(q) for q in v]
    assert int(r["count"]) == len(v) and int(r["nans"]) == sum(q != q for q in v), what
    for name, largest in (("largest", True), ("smallest", False)):
        at = _brute(v, k, largest)
        got = r[name]
        assert [int(a) for a in got["at"][: len(at)]] == at, (what, name)
        assert np.array_equal(_bits(got["value"][: len(at)]), _bits([v[a] for a in at])), (what, name)
        assert np.all(got["at"][len(at):] == M.NONE) and np.all(np.isnan(got["value"][len(at):])), (what, name)


def test_model_against_a_brute_force_sort():
    rng = np.random.default_rng(211)
    corner = np.array([0.0, -0.0, nan, 0.0, inf, -inf, -0.0])
    r = M.window_extremes(corner, 0, 7, 6)
    assert r["largest"]["at"].tolist() == [4, 0, 1, 3, 6, 5] and r["smallest"]["at"].tolist() == [5, 0, 1, 3, 6, 4]
    assert _bits(r["largest"]["value"]).tolist() == _bits([inf, 0.0, -0.0, 0.0, -0.0, -inf]).tolist()  # a -0.0 stays -0.0
    assert int(r["nans"]) == 1 and int(r["count"]) == 7
    for it in range(300):
        n = int(rng.integers(0, 60))
        kind = it % 4
        if kind == 0:
            v = rng.choice(SPECIAL, n)
        elif kind == 1:
            v = rng.integers(-2, 3, n).astype(np.float64)  # ties everywhere
        elif kind == 2:
            v = rng.normal(0, 1, n)
            v[rng.random(n) < 0.3] = nan
        else:
            v = np.full(n, nan) if it % 8 == 3 else np.sort(rng.normal(0, 1, n))
        begin = int(rng.integers(0, 5))
        x = np.concatenate([np.full(begin, 1e300), v, np.full(3, -1e300)])  # the outside must not matter
        for k in (1, 2, 5, 16):
            r = M.window_extremes(x, begin, n, k)
            _check_record(r, v, k, (it, k))
            assert M.dtype(k).itemsize == 16 + 32 * k
    e = M.window_extremes(np.ones(4), 2, 0, 3)
    assert int(e["count"]) == 0 and int(e["nans"]) == 0 and np.all(e["largest"]["at"] == M.NONE)
    assert np.all(np.isnan(e["smallest"]["value"]))
    # a long window goes through the partition cut: the same entries as the plain stable sort
    v = rng.integers(0, 50, 5000).astype(np.float64)
    for k in (1, 16):
        r = M.window_extremes(v, 0, 5000, k)
        assert r["largest"]["at"].tolist() == np.argsort(-v, kind="stable")[:k].tolist()
        assert r["smallest"]["at"].tolist() == np.argsort(v, kind="stable")[:k].tolist()


def _families(rng):
    t = np.arange(M.TILE, dtype=np.float64)
    one_lane = rng.normal(0, 1, M.TILE)
    lane_slots = [512 * q + 2 * (5 + 64 * kk) + e for q in range(4) for kk in range(4) for e in range(2)]
    one_lane[lane_slots] = 100.0 + rng.permutation(32)  # lane 5 holds the whole top
    nanny = rng.normal(0, 1, M.TILE)
    nanny[rng.random(M.TILE) < 0.3] = nan
    return {"ascending": t, "descending": -t, "constant": np.full(M.TILE, 3.0), "steps": np.floor(t / 64),
            "zeros": rng.choice([0.0, -0.0], M.TILE), "random": rng.normal(0, 1, M.TILE), "nan30": nanny,
            "sawtooth": t % 37, "one_lane": one_lane, "all_nan": np.full(M.TILE, nan),
            "few": np.where(rng.random(M.TILE) < 0.003, rng.integers(0, 3, M.TILE).astype(np.float64), nan)}


def test_the_tile_selection_on_the_kernels_lane_mapping():
    """lane-bests, bitonic network, threshold, ballot order and shifting insert give the model's lists on every family
    and range, with at most 31 (k - 1) insertions per tile and end"""
    rng = np.random.default_rng(223)
    worst = {}
    for name, x in _families(rng).items():
        ranges = [(0, M.TILE)] + [tuple(sorted(int(q) for q in rng.integers(0, M.TILE + 1, 2))) for _ in range(2)]
        ranges += [(700, 701), (129, 131)]
        for k in (1, 4, 16):
            for lo, hi in ranges:
                nans, lg, sm, cands = M.tile_select(x, lo, hi, k)
                want = M.window_extremes(x, lo, hi - lo, k)
                assert nans == int(want["nans"]), (name, k, lo, hi)
                for got, w in ((lg, want["largest"]), (sm, want["smallest"])):
                    assert [NONE_OR(a, lo) for a in got] == [int(a) for a in w["at"]], (name, k, lo, hi)
                assert max(cands) <= 31 * (k - 1), (name, k, lo, hi, cands)
                if (lo, hi) == (0, M.TILE):
                    worst[(name, k)] = max(cands)
    assert worst[("ascending", 16)] == 15 and worst[("ascending", 1)] == 0 and worst[("one_lane", 16)] >= 15
    print("insertions per tile and end:", worst)


def NONE_OR(slot, lo):
    return M.NONE if slot is None else slot - lo


def test_the_combine_pop_order():
    """cursors over the partials' lists, the maximum key, the lowest lane of equal keys: the union's first k"""
    rng = np.random.default_rng(227)
    for it in range(60):
        k = (1, 3, 16)[it % 3]
        n_parts = int(rng.integers(1, 65))
        lens = rng.integers(0, 40, n_parts)
        x = rng.choice([0.0, -0.0, 1.0, 2.0, nan, inf, -inf], int(lens.sum())) if it % 2 else rng.normal(0, 1, int(lens.sum()))
        off = np.concatenate(([0], np.cumsum(lens)))
        for end, name in ((0, "largest"), (1, "smallest")):
            parts = []
            for a, b in zip(off[:-1], off[1:]):
                r = M.window_extremes(x, int(a), int(b - a), k)[name]
                parts.append([(float(e["value"]), int(e["at"]) + int(a)) for e in r if int(e["at"]) != M.NONE])
            got = M.combine_pop(parts, k, end)
            w = M.window_extremes(x, 0, len(x), k)[name]
            want = [(float(e["value"]), int(e["at"])) for e in w if int(e["at"]) != M.NONE]
            assert [a for _, a in got] == [a for _, a in want], (it, name)
            assert _bits([v for v, _ in got]).tolist() == _bits([v for v, _ in want]).tolist(), (it, name)


def test_extremes_merge_against_the_model(A):
    rng = np.random.default_rng(229)
    lib = A.capi.lib()
    for it in range(200):
        n = int(rng.integers(0, 300))
        x = rng.choice([0.0, -0.0, 1.0, 2.0, -3.0, inf, -inf, nan] if it % 2 else [1.0, 2.0, 3.0], n)  # ties cross the seams
        parts = int(rng.integers(1, 10))
        cuts = np.sort(rng.integers(0, n + 1, parts - 1)) if n else np.zeros(parts - 1, dtype=np.int64)
        if it % 3 == 0 and parts > 2:
            cuts[1] = cuts[0]  # an empty window
        edges = [0] + [int(c) for c in cuts] + [n]
        for k in (1, 2, 5, 16):
            recs = M.windows_extremes(x, [(a, b - a) for a, b in zip(edges[:-1], edges[1:])], k)
            assert recs.dtype == A.window_extremes_dtype(k)
            got = A.extremes_merge(recs, k)
            whole = M.window_extremes(x, 0, n, k)
            assert np.array_equal(M.words(got), M.words(whole)), (it, k, edges)  # the union's own record, all words
            assert np.array_equal(M.words(got), M.words(M.merge(recs, k))), (it, k, edges)
    # the null and bad-k cases: nothing written
    for k in (1, 16):
        dt = A.window_extremes_dtype(k)
        r = M.windows_extremes(np.arange(5.0), [(0, 5)], k)
        out = np.full(dt.itemsize // 8, 77, dtype=np.uint64)
        po, pr = C.c_void_p(out.ctypes.data), C.c_void_p(r.ctypes.data)
        assert lib.atsc_extremes_merge(None, 1, k, po) == A.capi.E_INVALID
        assert lib.atsc_extremes_merge(pr, 1, k, None) == A.capi.E_INVALID
        assert lib.atsc_extremes_merge(pr, 1, 0, po) == A.capi.E_INVALID
        assert lib.atsc_extremes_merge(pr, 1, 17, po) == A.capi.E_INVALID
        assert np.all(out == 77)
        assert lib.atsc_extremes_merge(None, 0, k, po) == 0
        empty = M.window_extremes(np.zeros(0), 0, 0, k)
        assert np.array_equal(M.words(out.view(dt)), M.words(empty))
        assert lib.atsc_extremes_merge(pr, 1, k, po) == 0 and np.array_equal(M.words(out.view(dt)), M.words(r))
    with pytest.raises(ValueError):
        A.extremes_merge(np.zeros(1, dtype=A.window_extremes_dtype(1)), 17)


def test_dtype_and_constants(A):
    for k in range(1, 17):
        dt = A.window_extremes_dtype(k)
        assert dt.itemsize == 16 + 32 * k and dt == M.dtype(k)
        assert dt.names == ("count", "nans", "largest", "smallest")
        assert dt["largest"].shape == (k,) and dt["smallest"].shape == (k,)
        assert dt["largest"].base.names == ("value", "at") and dt["largest"].base == A.EXTREME
    for k in (0, 17, -1):
        with pytest.raises(ValueError):
            A.window_extremes_dtype(k)
    assert A.EXTREMES_MAX_K == M.MAX_K == 16 and A.EXTREMES_NONE == M.NONE == 2 ** 64 - 1


def test_symbols_and_callables(A):
    lib = A.capi.lib()
    for name in ("atsc_extremes_windows_dev", "atsc_extremes_windows", "atsc_stream_extremes_windows", "atsc_extremes_merge"):
        assert name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert A.capi.SIGNATURES["atsc_extremes_windows_dev"][1][6] is C.c_uint32
    assert A.capi.SIGNATURES["atsc_extremes_windows"][1][7] is C.c_uint32
    assert A.capi.SIGNATURES["atsc_stream_extremes_windows"][1][4] is C.c_uint32
    want = {A.Context.extremes_windows_host: ["self", "records", "begins", "counts", "k", "has_count"],
            A.DPlan.extremes_windows: ["self", "d_body", "begins", "counts", "k", "d_out", "stream"],
            A.CompressedStream.extremes_windows: ["self", "begins", "counts", "k"],
            A.extremes_data_windows: ["ctx", "bro", "begins", "counts", "k"]}
    for fn, names in want.items():
        sig = inspect.signature(fn)
        assert list(sig.parameters) == names, fn
        assert fn.__doc__ and fn.__doc__.strip(), fn
    assert inspect.signature(A.Context.extremes_windows_host).parameters["has_count"].default is False
    assert inspect.signature(A.DPlan.extremes_windows).parameters["stream"].default == 0
    assert list(inspect.signature(A.extremes_merge).parameters) == ["records", "k"] and A.extremes_merge.__doc__.strip()
    assert A.window_extremes_dtype.__doc__.strip()
    import atsc_amd.stream as S

    assert S.extremes_data_windows is A.extremes_data_windows


def test_command_line_usage_errors(A, tmp_path):
    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    f = tmp_path / "x.bro"
    f.write_bytes(b"")
    wants = "for '--extremes': expected 1..=16"
    cases = [([atsc, "-u", "--extremes", "3", str(f)], "error: '--extremes' needs '--buckets'"),
             ([atsc, "--extremes=3", str(f)], "error: '--extremes' needs '--buckets'"),
             ([atsc, "--buckets", "5", "--extremes", "3", str(f)], "error: '--buckets' needs '-u'"),
             ([csvc, "-u", "--extremes", "3", str(f)], "error: '--extremes' needs '--step'"),
             ([csvc, "-u", "--from", "0", "--to", "10", "--extremes", "3", str(f)], "error: '--extremes' needs '--step'"),
             ([csvc, "--extremes", "3", str(f)], "error: '--extremes' needs '--step'")]
    for bad in ("0", "17", "x", "", "3x", "-1", "1.5"):
        cases.append(([atsc, "-u", "--buckets", "5", "--extremes", bad, str(f)], wants))
        cases.append(([csvc, "-u", "--from", "0", "--to", "10", "--step", "5", "--extremes=" + bad, str(f)], wants))
    for cmd, msg in cases:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (cmd, r.stderr)
        assert msg in r.stderr, (cmd, r.stderr)
    for exe in (atsc, csvc):
        r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--extremes" in r.stderr, exe
        for col in ("nans", "max1_at", "maxK_at", "min1", "minK_at"):
            assert col in r.stderr, (exe, col)
