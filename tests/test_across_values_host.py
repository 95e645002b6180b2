"""The windowed across value counts without a GPU: the NumPy model (tests/across_values_model.py) against a scalar,
line-by-line restatement of the rule; hand values (the zero class, `above`, +-Inf, `more` at D = k and D = k + 1); the
merge identities through the library's own atsc_values_merge (the record is the merge of the N one-sample records,
sub-lists merge to the whole, a permuted list gives the same bytes, paging walks a column of 64 distinct values);
atsc_values_mode gives the majority value; the new symbols, the public surfaces and the command line's argument errors
(exit 2 before any GPU work)."""
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

from tests import across_model as AM
from tests import across_values_model as M
from tests import values_model as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATSC = os.path.join(ROOT, "atsc_amd", "bin", "atsc")
NAN, INF = np.nan, np.inf
SIZES = [1, 2, 3, 5, 8, 9, 17, 33, 63, 64]
KS = [1, 2, 3, 31, 32]
ABOVES = [NAN, 1.0, 0.0, -0.0, INF, -INF]


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _columns(rng, n):
    """(n, 8): few distinct values with both zeros, +-Inf and NaN holes; many distinct values; an all-NaN column, an
    all-equal column, a column of n distinct values, a column of one value and NaN"""
    x = np.empty((n, 8))
    x[:, 0] = rng.choice([-2.5, -0.0, 0.0, 1.0, 7.0], n)
    x[:, 1] = rng.choice([-INF, INF, -1.0, 1.0, NAN, 0.0, -0.0], n)
    x[:, 2] = rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 6, n)
    x[:, 3] = np.rint(rng.normal(0, 3, n))
    x[rng.random(n) < 0.3, 3] = NAN
    x[:, 4] = NAN
    x[:, 5] = -3.25
    x[:, 6] = rng.permutation(n) - n / 2.0
    x[:, 7] = np.where(rng.random(n) < 0.5, NAN, 1.0)
    return x


def _bits(v):
    return int(np.float64(v).view(np.uint64))


def _scalar_record(column, k, above):
    """the rule, line by line, on one column -> (count, nans, below, distinct, more, [(value bits, n) ..])"""
    nans = below = 0
    tally = {}
    for v in column:
        v = float(v)
        if v != v:
            nans += 1
            continue
        if above == above and not v > above:
            below += 1
            continue
        if v == 0.0:
            v = 0.0  # the zeros are one class, reported as +0.0
        tally[v] = tally.get(v, 0) + 1
    listed = sorted(tally)
    return (len(column), nans, below, min(len(listed), k), int(len(listed) > k), [(_bits(v), tally[v]) for v in listed[:k]])


def _as_tuple(r):
    d = int(r["distinct"])
    assert np.all(np.isnan(r["entry"]["value"][d:])) and np.all(r["entry"]["n"][d:] == 0)
    return (int(r["count"]), int(r["nans"]), int(r["below"]), d, int(r["more"]),
            [(_bits(e["value"]), int(e["n"])) for e in r["entry"][:d]])


def test_model_equals_the_rule_line_by_line():
    rng = np.random.default_rng(400)
    for n in SIZES:
        x = _columns(rng, n)
        for k in KS:
            for above in ABOVES + [float(x[0, 3]), float(x[0, 6])]:
                got = M.records(x, k, above)
                assert got.dtype == M.dtype(k) and got.shape == (8,)
                for p in range(8):
                    assert _as_tuple(got[p]) == _scalar_record(x[:, p], k, above), (n, k, above, p)


def test_hand_values():
    col = np.array([[-0.0, 0.0, 2.0, NAN, -INF, INF, 2.0, -1.5]]).T
    r = M.records(col, 8)[0]
    assert _as_tuple(r) == (8, 1, 0, 5, 0, [(_bits(-INF), 1), (_bits(-1.5), 1), (_bits(0.0), 2), (_bits(2.0), 2), (_bits(INF), 1)])
    for zero in (0.0, -0.0):  # above = either zero leaves out the zero class and everything negative
        r = M.records(col, 8, zero)[0]
        assert _as_tuple(r) == (8, 1, 4, 2, 0, [(_bits(2.0), 2), (_bits(INF), 1)])
    assert _as_tuple(M.records(col, 8, INF)[0]) == (8, 1, 7, 0, 0, [])  # +Inf lists nothing
    assert _as_tuple(M.records(col, 8, -INF)[0])[2:5] == (1, 4, 0)  # -Inf leaves out only the -Inf sample
    assert _as_tuple(M.records(col, 8, 2.0)[0]) == (8, 1, 6, 1, 0, [(_bits(INF), 1)])  # a listed value as above
    # more at D = k and at D = k + 1
    assert _as_tuple(M.records(col, 5)[0])[3:5] == (5, 0)
    r = M.records(col, 4)[0]
    assert _as_tuple(r)[3:5] == (4, 1) and float(r["entry"]["value"][3]) == 2.0
    for n in SIZES:  # an all-NaN column, an all-equal column
        assert _as_tuple(M.records(np.full((n, 1), NAN), 3)[0]) == (n, n, 0, 0, 0, [])
        assert _as_tuple(M.records(np.full((n, 1), -0.0), 3)[0]) == (n, 0, 0, 1, 0, [(0, n)])


def test_model_ranges(A):
    fulls = [np.arange(30.0) % 3, np.arange(30.0) % 2, np.full(30, NAN)]
    got, off = M.across_values(fulls, [3, 0, 29, 5], [10, 0, 1, 15], 2, 4)
    assert off.tolist() == [0, 3, 3, 4, 8] and got.shape == (8,) and got.dtype == M.dtype(2)
    assert off.tolist() == A.across_offsets([10, 0, 1, 15], 4).tolist()
    # positions 3, 7, 11 | 29 | 5, 9, 13, 17: (p % 3, p % 2, NaN)
    want = [sorted({p % 3, p % 2}) for p in (3, 7, 11, 29, 5, 9, 13, 17)]
    assert [[float(v) for v in r["entry"]["value"][: int(r["distinct"])]] for r in got] == want
    assert np.all(got["count"] == 3) and np.all(got["nans"] == 1)
    empty, off = M.across_values(fulls, [], [], 1)
    assert empty.shape == (0,) and off.tolist() == [0]


def test_merge_identities_through_the_library(A):
    rng = np.random.default_rng(410)
    for n in SIZES:
        x = _columns(rng, n)
        for k in KS:
            for above in (NAN, 0.0, float(x[0, 3])):
                whole = M.records(x, k, above)
                singles = [M.records(x[j:j + 1], k, above) for j in range(n)]
                perm = M.records(x[rng.permutation(n)], k, above)
                assert perm.tobytes() == whole.tobytes()
                for p in range(8):
                    w = VM.words(whole[p])
                    # the record is the merge of the N streams' one-sample records
                    assert np.array_equal(VM.words(A.values_merge(np.array([s[p] for s in singles]), k)), w), (n, k, above, p)
                    for cut in sorted({1, n // 2, n - 1}) if n > 1 else ():
                        parts = np.array([M.records(x[:cut], k, above)[p], M.records(x[cut:], k, above)[p]])
                        assert np.array_equal(VM.words(A.values_merge(parts, k)), w), (n, k, above, p, cut)


def test_paging_walks_a_column_of_64_distinct_values(A):
    col = np.random.default_rng(420).permutation(64) * 0.5 - 7.0
    for k, calls in ((32, 2), (1, 64), (31, 3)):
        pages = M.pages(col, k)
        assert len(pages) == calls == math.ceil(64 / k)
        listed = [float(v) for r in pages for v in r["entry"]["value"][: int(r["distinct"])]]
        assert listed == sorted(col.tolist())
        assert all(int(r["count"]) == 64 and int(r["more"]) == (i + 1 < calls) for i, r in enumerate(pages))
        assert [int(r["below"]) for r in pages] == [min(64, i * k) for i in range(calls)]


def test_mode_is_the_majority_value(A):
    col = np.array([[3.0, 1.0, 3.0, NAN, 2.0, 3.0, 1.0, -0.0, 0.0]]).T
    r = M.records(col, 4)
    m = A.values_mode(r, 4)
    assert float(m["value"][0]) == 3.0 and int(m["n"][0]) == 3 and int(m["exact"][0]) == 1
    tie = M.records(np.array([[5.0, 5.0, -1.0, -1.0, 9.0]]).T, 2)  # of equal n the smallest value; more: not exact
    m = A.values_mode(tie, 2)
    assert float(m["value"][0]) == -1.0 and int(m["n"][0]) == 2 and int(m["exact"][0]) == 0
    assert np.array_equal(A.values_mode(r, 4), VM.mode(r))


def test_symbols_are_bound(A):
    import ctypes as C

    lib = A.capi.lib()
    for name in ("atsc_across_values_windows_dev", "atsc_across_values_windows", "atsc_stream_across_values_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
        assert getattr(lib, name).argtypes[-3 if name.endswith("_dev") else -2] is C.c_double  # above, by value
    assert len(A.capi.SIGNATURES["atsc_across_values_windows_dev"][1]) == 12
    assert len(A.capi.SIGNATURES["atsc_across_values_windows"][1]) == 12
    assert len(A.capi.SIGNATURES["atsc_stream_across_values_windows"][1]) == 9


def test_public_surfaces(A):
    want = {(A.Context, "across_values_windows_host"):
            "(self, records_list, begins, counts, k, stride=1, above=nan, has_count=False)",
            (A.DPlan, "across_values_windows"):
            "(self, d_body, others, other_bodies, begins, counts, k, d_out, stride=1, above=nan, stream=0)",
            (A.CompressedStream, "across_values_windows"): "(self, others, begins, counts, k, stride=1, above=nan)",
            (A.stream, "across_values_data_windows"): "(ctx, bros, begins, counts, k, stride=1, above=nan)"}
    assert A.VALUES_MAX_K == M.MAX_K and A.ACROSS_MAX_STREAMS == AM.MAX_STREAMS
    for (owner, name), sig in want.items():
        f = getattr(owner, name)
        assert str(inspect.signature(f)) == sig, name
        assert f.__doc__ and f.__doc__.strip()
    assert A.across_values_data_windows is A.stream.across_values_data_windows
    for k in KS:
        assert A.window_values_dtype(k) == M.dtype(k)


def test_null_context_is_invalid(A):
    lib = A.capi.lib()
    assert lib.atsc_across_values_windows(None, 1, None, None, None, 0, None, None, 1, 1, NAN, None) == A.capi.E_INVALID
    assert lib.atsc_across_values_windows_dev(None, 1, None, None, 0, None, None, 1, 1, NAN, None, None) == A.capi.E_INVALID
    assert lib.atsc_stream_across_values_windows(None, 1, 0, None, None, 1, 1, NAN, None) == A.capi.E_INVALID


def test_header_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "atsc_hip.h")).read()
    for name in ("atsc_across_values_windows_dev", "atsc_across_values_windows", "atsc_stream_across_values_windows"):
        assert ("int %s(" % name) in hdr, name
    at = hdr.index("Windowed across value counts")
    text = " ".join(hdr[at: hdr.index("int atsc_across_values_windows_dev(")].split())
    for phrase in ("atsc_values_merge", "atsc_values_mode", "count - nans equals atsc_across_windows' count",
                   "entry[0].value equals the across' min", "atsc_across_histogram_windows", "count_values"):
        assert phrase in text, phrase


def _run(argv):
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = "-1"  # exit 2 must come before any GPU work
    return subprocess.run(argv, capture_output=True, text=True, env=env, timeout=60)


def test_atsc_cli_argument_errors(A, tmp_path):
    f, other = str(tmp_path / "missing.bro"), str(tmp_path / "other.bro")
    across = ["-u", "--samples", "0:10", "--across", other]
    r = _run([ATSC, "-u", "--samples", "0:10", "--across-values", "4", f])  # the option without --across
    assert r.returncode == 2 and "'--across-values' needs '--across'" in r.stderr, r.stderr
    r = _run([ATSC, "-u", "--across-values", "4", f])
    assert r.returncode == 2 and "error:" in r.stderr, r.stderr
    for bad in ("0", "33", "-1", "", "a", "4:", "4:nan", "4:x", "4:1:2", "4: 1", "1.5"):  # --values' parser and its messages
        r = _run([ATSC, *across, "--across-values", bad, f])
        assert r.returncode == 2 and "for '--across-values': expected K[:ABOVE], K in 1..=32, ABOVE a number" in r.stderr, (bad, r.stderr)
    # --values keeps its meaning: it needs --buckets, and --across does not go with --buckets
    r = _run([ATSC, *across, "--values", "4", f])
    assert r.returncode == 2 and "--buckets" in r.stderr, r.stderr
    r = _run([ATSC, "--help"])
    assert "--across-values" in r.stdout + r.stderr
    assert "vcount,vnans,vbelow,vdistinct,vmore,v0,n0 .. v<K-1>,n<K-1>" in r.stdout + r.stderr
    # a well-formed command line gets past the arguments (and fails on the missing file, not with a usage error)
    for spec in ("1", "32", "4:0.5", "4:-inf", "4:-0"):
        r = _run([ATSC, *across, "--across-stride", "3", "--across-moments", "--across-values", spec, f])
        assert r.returncode != 2, r.stderr
    # csv-compressor has no --across, so none of its options
    r = _run([os.path.join(ROOT, "atsc_amd", "bin", "csv-compressor"), "--across-values", "4", f])
    assert r.returncode == 2, r.stderr
