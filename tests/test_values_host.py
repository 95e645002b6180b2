"""CPU-only tests of the windowed value counts' host half: the NumPy model of the contract (tests/values_model.py) against
a brute-force sort-and-count, the two kernels' counting (written as plain functions over k_val_tiles' slot-to-lane mapping
and k_val_combine's cursors) against the model, atsc_values_merge (the C function) against the model's merge and against the union's own
record bit for bit, atsc_values_mode, the record's dtype, the new symbols and callables, and the command lines' usage
errors."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import values_model as M

inf, nan = float("inf"), float("nan")
NAN2 = float(np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)[0])  # a NaN with a sign and a payload
SPECIAL = [0.0, -0.0, nan, NAN2, 1.0, -1.0, inf, -inf, 2.5, 1.0, 5e-324, -5e-324]
ABOVES = [nan, 0.0, -0.0, inf, -inf, 1.0, -1.0, 0.5, 2.5]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _brute(v, k, above):
    """(nans, below, D, the first k (value bits, n)) by a Python sort of the non-NaN samples and a walk over it"""
    v = [float(q) for q in v]
    nans = sum(q != q for q in v)
    rest = [q for q in v if q == q]
    below = 0
    if above == above:
        below = sum(not q > above for q in rest)
        rest = [q for q in rest if q > above]
    rest.sort()
    ents = []
    for q in rest:
        if ents and ents[-1][0] == q:  # as values: -0.0 == +0.0
            ents[-1][1] += 1
        else:
            ents.append([0.0 if q == 0.0 else q, 1])
    return nans, below, len(ents), [(int(_bits(e[0])[0]), e[1]) for e in ents[:k]]


def _check_record(r, v, k, above, what):
    nans, below, D, ents = _brute(v, k, above)
    assert (int(r["count"]), int(r["nans"]), int(r["below"])) == (len(v), nans, below), what
    assert int(r["distinct"]) == min(D, k) and int(r["more"]) == int(D > k), what
    d = len(ents)
    assert [(int(b), int(n)) for b, n in zip(_bits(r["entry"]["value"][:d]), r["entry"]["n"][:d])] == ents, what
    assert np.all(np.isnan(r["entry"]["value"][d:])) and np.all(r["entry"]["n"][d:] == 0), what
    if not int(r["more"]):
        assert int(r["count"]) == nans + below + int(r["entry"]["n"].sum()), what


def test_model_against_a_brute_force_count():
    rng = np.random.default_rng(311)
    corner = np.array([0.0, -0.0, nan, 0.0, inf, -inf, -0.0, NAN2, 3.0, -inf])
    r = M.window_values(corner, 0, 10, 6)
    assert (int(r["count"]), int(r["nans"]), int(r["below"]), int(r["distinct"]), int(r["more"])) == (10, 2, 0, 4, 0)
    assert _bits(r["entry"]["value"][:4]).tolist() == _bits([-inf, 0.0, 3.0, inf]).tolist()  # one +0.0 for the zeros
    assert r["entry"]["n"].tolist() == [2, 4, 1, 1, 0, 0]
    seen = set()
    for it in range(400):
        n = int(rng.integers(0, 80))
        kind = it % 5
        if kind == 0:
            v = rng.choice(SPECIAL, n)
        elif kind == 1:
            v = rng.integers(-2, 3, n).astype(np.float64)  # five values: D below, at and above k
        elif kind == 2:
            v = rng.normal(0, 1, n)
            v[rng.random(n) < 0.3] = nan
        elif kind == 3:
            v = rng.choice([0.0, -0.0], n)
        else:
            v = np.full(n, nan) if it % 10 == 4 else np.round(rng.normal(0, 2, n))
        begin = int(rng.integers(0, 5))
        x = np.concatenate([np.full(begin, -1e300), v, np.full(3, 1e300)])  # the outside must not matter
        for k in (1, 2, 5, 32):
            for above in ABOVES:
                r = M.window_values(x, begin, n, k, above)
                _check_record(r, v, k, above, (it, k, above))
                D = _brute(v, k, above)[2]
                seen.add("below" if D < k else "at" if D == k else "above")
            assert M.dtype(k).itemsize == 32 + 16 * k
    assert seen == {"below", "at", "above"}
    e = M.window_values(np.ones(4), 2, 0, 3)
    assert not M.words(e)[0, :4].any() and np.all(np.isnan(e["entry"]["value"])) and not e["entry"]["n"].any()
    # the special values of above
    v = np.array([-inf, -2.0, -0.0, 0.0, 1.0, inf, nan])
    assert int(M.window_values(v, 0, 7, 8, inf)["distinct"]) == 0 and int(M.window_values(v, 0, 7, 8, inf)["below"]) == 6
    r = M.window_values(v, 0, 7, 8, -inf)
    assert int(r["below"]) == 1 and int(r["distinct"]) == 4 and r["entry"]["value"][:4].tolist() == [-2.0, 0.0, 1.0, inf]
    for z in (0.0, -0.0):
        r = M.window_values(v, 0, 7, 8, z)
        assert int(r["below"]) == 4 and r["entry"]["value"][:2].tolist() == [1.0, inf] and int(r["distinct"]) == 2
    # the prefix rule
    v = rng.integers(0, 9, 200).astype(np.float64)
    full = M.windows_values(v, [(0, 200), (5, 3), (0, 0)], 32, 2.0)
    for j in (1, 3, 6, 7, 31):
        assert np.array_equal(M.words(M.head_of(full, j)), M.words(M.windows_values(v, [(0, 200), (5, 3), (0, 0)], j, 2.0)))


def _families(rng):
    t = np.arange(M.TILE, dtype=np.float64)
    nanny = rng.normal(0, 1, M.TILE)
    nanny[rng.random(M.TILE) < 0.3] = nan
    one_lane = 100.0 + rng.integers(0, 500, M.TILE).astype(np.float64)
    lane_slots = [512 * q + 2 * (5 + 64 * kk) + e for q in range(4) for kk in range(4) for e in range(2)]
    one_lane[lane_slots] = rng.permutation(32).astype(np.float64)  # lane 5 holds the tile's 32 smallest values
    return {"ascending": t, "constant": np.full(M.TILE, 3.0), "steps": np.floor(t / 64), "zeros": rng.choice([0.0, -0.0], M.TILE),
            "states": rng.choice([0.0, 1.0, 2.0, 3.0, 503.0], M.TILE), "random": rng.normal(0, 1, M.TILE), "nan30": nanny,
            "special": rng.choice(SPECIAL, M.TILE), "one_lane": one_lane, "all_nan": np.full(M.TILE, nan),
            "few": np.where(rng.random(M.TILE) < 0.003, rng.integers(0, 3, M.TILE).astype(np.float64), nan)}


def test_the_tile_rounds_on_the_kernels_lane_mapping():
    """keys by the kernel's slot-to-lane mapping, rounds of wave minimum, count and knock-out: the model's record on every
    family and range, in min(D, k) + 1 rounds"""
    rng = np.random.default_rng(331)
    for name, x in _families(rng).items():
        ranges = [(0, M.TILE)] + [tuple(sorted(int(q) for q in rng.integers(0, M.TILE + 1, 2))) for _ in range(2)]
        ranges += [(700, 701), (129, 131), (5, 5)]
        for k, above in ((1, nan), (4, nan), (32, nan), (4, 1.0), (32, 0.0), (3, inf), (3, -inf)):
            for lo, hi in ranges:
                got, rounds = M.tile_count(x, lo, hi, k, above)
                want = M.window_values(x, lo, hi - lo, k, above)
                assert np.array_equal(M.words(got), M.words(want)), (name, k, above, lo, hi)
                D = _brute(x[lo:hi], k, above)[2]
                assert rounds == min(D, k) + 1, (name, k, above, lo, hi, rounds)
    assert M.tile_count(_families(rng)["constant"], 0, M.TILE, 32)[1] == 2  # a constant tile: one counting round and one look
    for v in SPECIAL + [1e300, -1e300, 0.1]:
        if v == v:
            assert _bits(M.key_value(M.key(v)))[0] == _bits(0.0 if v == 0.0 else v)[0] and 0 < M.key(v) < M.NO_KEY
    ordered = [-inf, -1e300, -1.0, -5e-324, 0.0, 5e-324, 1.0, 1e300, inf]
    assert [M.key(v) for v in ordered] == sorted(M.key(v) for v in ordered) and M.key(-0.0) == M.key(0.0) and M.key(nan) == 0


def test_the_combine_rounds():
    """cursors over the partials' lists, the wave minimum, the sums of equal heads: tiles into groups of 64 into the
    window's record, equal to the model's on the whole"""
    rng = np.random.default_rng(337)
    for it in range(40):
        k = (1, 4, 32)[it % 3]
        above = (nan, 2.0)[it % 2]
        n_parts = int(rng.integers(1, 140))
        lens = rng.integers(0, 40, n_parts)
        pool = ([0.0, -0.0, 1.0, 2.0, 3.0, nan, inf, -inf], np.arange(60.0), [5.0])[it % 3]
        x = rng.choice(pool, int(lens.sum()))
        off = np.concatenate(([0], np.cumsum(lens)))
        parts = [M.window_values(x, int(a), int(b - a), k, above) for a, b in zip(off[:-1], off[1:])]
        while len(parts) > 1 or it % 4 == 0:  # (a single partial goes through one pass as well)
            parts = [M.combine(parts[g:g + 64], k) for g in range(0, len(parts), 64)]
            if len(parts) == 1:
                break
        assert np.array_equal(M.words(parts[0]), M.words(M.window_values(x, 0, len(x), k, above))), (it, k, above)
    assert np.array_equal(M.words(M.combine([], 3)), M.words(M.empty(3)))  # an empty window's final pass


def _split(rng, n, parts, kind):
    """n sample indices in `parts` disjoint groups: stretches cut at random places, or every sample dealt at random"""
    if kind == 0:
        cuts = np.sort(rng.integers(0, n + 1, parts - 1)) if n else np.zeros(parts - 1, dtype=np.int64)
        if parts > 2:
            cuts[1] = cuts[0]  # an empty part
        edges = [0] + [int(c) for c in cuts] + [n]
        return [np.arange(a, b) for a, b in zip(edges[:-1], edges[1:])]
    owner = rng.integers(0, parts, n)
    return [np.flatnonzero(owner == p) for p in range(parts)]


def test_values_merge_against_the_model(A):
    rng = np.random.default_rng(313)
    lib = A.capi.lib()
    hidden = 0
    for it in range(240):
        n = int(rng.integers(0, 300))
        pool = ([0.0, -0.0, 1.0, 2.0, -3.0, inf, -inf, nan], [1.0, 2.0, 3.0], np.arange(40.0))[it % 3]
        x = rng.choice(pool, n)
        if it % 3 == 2 and n > 40:
            x[: n // 2] = np.sort(x[: n // 2]) + 100.0  # the first parts hold only large values: their own lists overflow
        parts = int(rng.integers(1, 10))
        groups = _split(rng, n, parts, it % 2)
        order = rng.permutation(parts)
        for k in (1, 2, 5, 32):
            for above in (nan, 1.0):
                recs = np.zeros(parts, dtype=M.dtype(k))
                for j, p in enumerate(order):
                    recs[j] = M.window_values(x[groups[p]], 0, len(groups[p]), k, above)
                assert recs.dtype == A.window_values_dtype(k)
                got = A.values_merge(recs, k)
                whole = M.window_values(x, 0, n, k, above)
                assert np.array_equal(M.words(got), M.words(whole)), (it, k, above)  # the union's own record, all words
                assert np.array_equal(M.words(got), M.words(M.merge(recs, k))), (it, k, above)
                # a part with more set none of whose values the union lists
                cut = float(got["entry"]["value"][int(got["distinct"]) - 1]) if int(got["distinct"]) else nan
                hidden += any(int(r["more"]) and float(r["entry"]["value"][0]) > cut for r in recs)
    assert hidden > 20
    # the null and bad-k cases: nothing written
    for k in (1, 32):
        dt = A.window_values_dtype(k)
        r = M.windows_values(np.arange(5.0), [(0, 5)], k)
        out = np.full(dt.itemsize // 8, 77, dtype=np.uint64)
        po, pr = C.c_void_p(out.ctypes.data), C.c_void_p(r.ctypes.data)
        assert lib.atsc_values_merge(None, 1, k, po) == A.capi.E_INVALID
        assert lib.atsc_values_merge(pr, 1, k, None) == A.capi.E_INVALID
        assert lib.atsc_values_merge(pr, 1, 0, po) == A.capi.E_INVALID
        assert lib.atsc_values_merge(pr, 1, 33, po) == A.capi.E_INVALID
        assert np.all(out == 77)
        assert lib.atsc_values_merge(None, 0, k, po) == 0
        assert np.array_equal(M.words(out.view(dt)), M.words(M.empty(k)))
        assert lib.atsc_values_merge(pr, 1, k, po) == 0 and np.array_equal(M.words(out.view(dt)), M.words(r))
    with pytest.raises(ValueError):
        A.values_merge(np.zeros(1, dtype=A.window_values_dtype(1)), 33)


def test_values_mode(A):
    rng = np.random.default_rng(317)
    x = np.array([3.0, 1.0, 3.0, 1.0, 2.0, nan, 7.0, 7.0, 7.0, -0.0, 0.0])
    wins = [(0, 5), (0, 4), (0, 11), (5, 1), (0, 0), (4, 1), (6, 5)]
    for k in (1, 2, 3, 32):
        recs = M.windows_values(x, wins, k)
        got = A.values_mode(recs, k)
        assert got.dtype == A.VALUE_MODE == M.VALUE_MODE and got.dtype.itemsize == 24
        want = M.mode(recs)
        assert np.array_equal(got["n"], want["n"]) and np.array_equal(got["exact"], want["exact"]) and not got["pad"].any()
        assert np.array_equal(_bits(got["value"])[got["n"] > 0], _bits(want["value"])[want["n"] > 0])
        assert np.all(np.isnan(got["value"][got["n"] == 0]))
    m = A.values_mode(M.windows_values(x, wins, 32), 32)
    assert [(float(v), int(n), int(e)) for v, n, e in zip(m["value"], m["n"], m["exact"])][:3] == [
        (1.0, 2, 1), (1.0, 2, 1), (7.0, 3, 1)]  # ties: the smallest value
    assert math.isnan(m["value"][3]) and (int(m["n"][3]), int(m["exact"][3])) == (0, 1)  # an all-NaN window
    assert math.isnan(m["value"][4]) and (int(m["n"][4]), int(m["exact"][4])) == (0, 1)  # an empty window
    m = A.values_mode(M.windows_values(x, wins, 2), 2)  # more != 0: the mode of what is listed, and not exact
    assert (float(m["value"][2]), int(m["n"][2]), int(m["exact"][2])) == (0.0, 2, 0)
    assert (float(m["value"][0]), int(m["n"][0]), int(m["exact"][0])) == (1.0, 2, 0)
    for it in range(50):
        v = rng.integers(0, 6, 100).astype(np.float64)
        k = int(rng.integers(1, 9))
        recs = M.windows_values(v, [(int(b), int(rng.integers(0, 40))) for b in rng.integers(0, 60, 8)], k, float(rng.integers(-1, 3)))
        got, want = A.values_mode(recs, k), M.mode(recs)
        assert np.array_equal(got.view(np.uint64).reshape(8, 3)[:, 1:], want.view(np.uint64).reshape(8, 3)[:, 1:])
        ok = want["n"] > 0
        assert np.array_equal(got["value"][ok], want["value"][ok]) and np.all(np.isnan(got["value"][~ok]))
    lib = A.capi.lib()
    r = M.windows_values(x, wins[:1], 2)
    out = np.full(3, 77, dtype=np.uint64)
    assert lib.atsc_values_mode(None, 1, 2, C.c_void_p(out.ctypes.data)) == A.capi.E_INVALID
    assert lib.atsc_values_mode(C.c_void_p(r.ctypes.data), 1, 2, None) == A.capi.E_INVALID
    for k in (0, 33):
        assert lib.atsc_values_mode(C.c_void_p(r.ctypes.data), 1, k, C.c_void_p(out.ctypes.data)) == A.capi.E_INVALID
    assert np.all(out == 77) and lib.atsc_values_mode(None, 0, 2, None) == 0
    assert len(A.values_mode(np.zeros(0, dtype=A.window_values_dtype(2)), 2)) == 0


def test_dtype_and_constants(A):
    for k in range(1, 33):
        dt = A.window_values_dtype(k)
        assert dt.itemsize == 32 + 16 * k and dt == M.dtype(k)
        assert dt.names == ("count", "nans", "below", "distinct", "more", "entry")
        assert dt["entry"].shape == (k,) and dt["entry"].base == A.VALUE_COUNT and A.VALUE_COUNT.names == ("value", "n")
        assert dt.fields["distinct"][1] == 24 and dt.fields["more"][1] == 28 and dt.fields["entry"][1] == 32
    for k in (0, 33, -1):
        with pytest.raises(ValueError):
            A.window_values_dtype(k)
    assert A.VALUES_MAX_K == A.capi.VALUES_MAX_K == M.MAX_K == 32
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "atsc_hip.h")).read()
    assert re.search(r"#define ATSC_VALUES_MAX_K 32\b", hdr) and "#define ATSC_VALUES_BYTES(k) (32u + 16u * (size_t)(k))" in hdr


SIGNATURES = {
    ("Context", "values_windows_host"): "(self, records, begins, counts, k, above=nan, has_count=False)",
    ("DPlan", "values_windows"): "(self, d_body, begins, counts, k, d_out, above=nan, stream=0)",
    ("CompressedStream", "values_windows"): "(self, begins, counts, k, above=nan)",
    ("stream", "values_data_windows"): "(ctx, bro, begins, counts, k, above=nan)",
}


def test_symbols_and_callables(A):
    from atsc_amd import engine, stream

    lib = A.capi.lib()
    for name in ("atsc_values_windows_dev", "atsc_values_windows", "atsc_stream_values_windows", "atsc_values_merge",
                 "atsc_values_mode"):
        assert name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert A.capi.SIGNATURES["atsc_values_windows_dev"][1][6:8] == [C.c_uint32, C.c_double]
    assert A.capi.SIGNATURES["atsc_values_windows"][1][7:9] == [C.c_uint32, C.c_double]
    assert A.capi.SIGNATURES["atsc_stream_values_windows"][1][4:6] == [C.c_uint32, C.c_double]
    owners = {"Context": engine.Context, "DPlan": engine.DPlan, "CompressedStream": stream.CompressedStream, "stream": stream}
    for (owner, name), sig in SIGNATURES.items():
        f = getattr(owners[owner], name)
        assert str(inspect.signature(f)) == sig, (owner, name)
        assert f.__doc__ and f.__doc__.strip(), (owner, name)
        assert re.search(r"^\s*def %s\(" % name, inspect.getsource(inspect.getmodule(f)), re.M)  # written out as a def
    assert A.values_data_windows is stream.values_data_windows
    for fn, names in ((A.values_merge, ["records", "k"]), (A.values_mode, ["records", "k"]), (A.window_values_dtype, ["k"])):
        assert list(inspect.signature(fn).parameters) == names and fn.__doc__.strip(), fn
    for name in ("VALUE_COUNT", "VALUE_MODE", "VALUES_MAX_K", "values_merge", "values_mode", "window_values_dtype",
                 "values_data_windows"):
        assert hasattr(A, name), name


def test_command_line_usage_errors(A, tmp_path):
    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    f = tmp_path / "x.bro"
    f.write_bytes(b"")
    wants = "for '--values': expected K[:ABOVE], K in 1..=32, ABOVE a number"
    cases = [([atsc, "-u", "--values", "3", str(f)], "error: '--values' needs '--buckets'"),
             ([atsc, "--values=3:0.5", str(f)], "error: '--values' needs '--buckets'"),
             ([atsc, "--buckets", "5", "--values", "3", str(f)], "error: '--buckets' needs '-u'"),
             ([csvc, "-u", "--values", "3", str(f)], "error: '--values' needs '--step'"),
             ([csvc, "-u", "--from", "0", "--to", "10", "--values", "3:1", str(f)], "error: '--values' needs '--step'"),
             ([csvc, "--values", "3", str(f)], "error: '--values' needs '--step'")]
    for bad in ("0", "33", "x", "", "3x", "-1", "1.5", "3:", "3:x", "3:1x", "3:nan", ":1", "0:1", "33:1", "3: 1", "3:1:2"):
        cases.append(([atsc, "-u", "--buckets", "5", "--values", bad, str(f)], wants))
        cases.append(([csvc, "-u", "--from", "0", "--to", "10", "--step", "5", "--values=" + bad, str(f)], wants))
    for cmd, msg in cases:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, (cmd, r.stderr)
        assert msg in r.stderr, (cmd, r.stderr)
    for exe in (atsc, csvc):
        r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--values <K[:ABOVE]>" in r.stderr, exe
        for col in ("below", "distinct", "more", "v1", "nK"):
            assert col in r.stderr, (exe, col)
