"""The windowed rolling runs without a GPU: the NumPy model of the contract (tests/rolling_runs_model.py) -- its nine
integers, read off the chunk partials by the merge rule, against the windowed runs' naive model at every position; its
excess against exact rational arithmetic and, on integers, against the windowed runs' bit for bit; atsc_runs_merge over
disjoint adjacent positions -- and the new symbols and surfaces of the library."""
import ctypes as C
import inspect
from fractions import Fraction

import numpy as np
import pytest

from tests import rolling_runs_model as M
from tests import runs_model as RM

WIDTHS = [1, 2, 3, 8, 9, 64, 65, 300, 2049]
INTS = RM.FIELDS[:9]
LIMIT = 5.0  # a sample value of every stream below: EQ, NE, GE and GT differ


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _planted():
    """7000 integer samples around the limit: runs over it of 1, 7, 8 and 9 samples, one with a NaN inside, runs of 2047,
    2048 and 2049 that cross the multiples of 2048 at different places, and a noisy tail.  Values: 9 inside a run, 5 (the
    limit) and 2 outside"""
    rng = np.random.default_rng(41)
    x = np.where(rng.random(7000) < 0.5, 5.0, 2.0)
    at = 3
    for n in (1, 7, 8, 9):
        x[at - 1] = 2.0
        x[at:at + n] = 9.0
        x[at + n] = 5.0
        at += n + 2
    x[at:at + 9] = 9.0
    x[at + 4] = np.nan  # a NaN inside a run ends it
    at = 50
    for n in (2047, 2048, 2049):
        x[at - 1] = 2.0
        x[at:at + n] = 9.0 + (np.arange(n) % 7)
        x[at + n] = 5.0
        at += n + 2
    tail = slice(at + 5, 7000)
    x[tail] = rng.integers(0, 12, 7000 - at - 5).astype(np.float64)
    x[6500] = np.nan
    return x


def _equal_longest(first_straddles):
    """4300 samples with two runs of 100, the longest, and a shorter one: the earlier over index 2048 and the later inside
    the aligned chunk [3072, 3200), or the earlier inside [1024, 1152) and the later over index 2048"""
    x = np.full(4300, 2.0)
    x[10:60] = 9.0
    for at in ((2000, 3080) if first_straddles else (1030, 2000)):
        x[at:at + 100] = 9.0
    x[4200:4210] = 5.0
    return x


STREAMS = {
    "planted": _planted,
    "inside": lambda: np.full(2200, 9.0),
    "outside": lambda: np.full(2200, 2.0),
    "equal, straddler first": lambda: _equal_longest(True),
    "equal, straddler last": lambda: _equal_longest(False),
}


@pytest.fixture(scope="module")
def streams():
    return {k: f() for k, f in STREAMS.items()}


def _naive_ints(mask, w):
    """the nine integers of every position of the stream at stride 1, each off its own window's mask: no merge"""
    out = np.zeros((len(mask) - w + 1, 9), dtype=np.uint64)
    for lo in range(len(out)):
        out[lo] = RM.mask_record(mask[lo:lo + w])
    return out


def _ints(rec):
    return np.stack([rec[k] for k in INTS], axis=1)


def test_streams_hold_what_they_should(streams):
    x = streams["planted"]
    r = RM.window_runs(x, 0, len(x), RM.GT, LIMIT)
    assert r[3] == 2049 and r[1] > 6144
    m = RM.inside_mask(x, RM.GT, LIMIT)
    d = np.diff(np.concatenate(([0], m.astype(np.int8), [0])))
    lens = set((np.flatnonzero(d == -1) - np.flatnonzero(d == 1)).tolist())
    assert {1, 7, 8, 9, 2047, 2048, 2049} <= lens
    masks = {op: RM.inside_mask(x, op, LIMIT).tobytes() for op in RM.OPS}
    assert len(set(masks.values())) == 6
    for name in ("equal, straddler first", "equal, straddler last"):
        r = RM.window_runs(streams[name], 0, 4300, RM.GT, LIMIT)
        assert r[3] == 100 and r[2] == 3


@pytest.mark.parametrize("name", list(STREAMS))
def test_integers_equal_the_naive_model_at_every_position(streams, name):
    """w x stride x op: the records the model reads off its pyramid by the merge rule, against runs_model's mask_record
    (what runs_model.window_runs returns as its nine integers) of each position's own window"""
    x = streams[name]
    n = len(x)
    naive = {}
    for op in RM.OPS:
        P = M.Pyramid(x, op, LIMIT)
        mask = RM.inside_mask(x, op, LIMIT)
        for w in WIDTHS:
            key = (mask.tobytes(), w)
            if key not in naive:
                naive[key] = _naive_ints(mask, w)
            want = naive[key]
            for stride in sorted({1, 7, w}):
                got, off = P.rolling([0], [n], w, stride)
                assert int(off[1]) == M.outputs(n, w, stride)
                assert np.array_equal(_ints(got), want[::stride]), (name, op, w, stride)
                assert np.all(got["samples"] == w)
    # the literal form at a few positions, all ten fields
    P = M.Pyramid(x, RM.GE, LIMIT)
    for w in WIDTHS:
        lo = sorted({0, 1, 47, min(2047, n - w), n - w} & set(range(n - w + 1)))
        got = P.records(lo, w)
        for i, b in enumerate(lo):
            lit = np.array([M.window_record(x, b, w, RM.GE, LIMIT)], dtype=M.RECORD)
            assert got[i:i + 1].tobytes() == lit.tobytes(), (name, b, w)


def test_of_equal_longest_runs_the_earliest_wins_in_the_tree(streams):
    for name, first, second in (("equal, straddler first", 2000, 3080), ("equal, straddler last", 1030, 2000)):
        x = streams[name]
        P = M.Pyramid(x, RM.GT, LIMIT)
        w = 2049
        lo = np.arange(0, len(x) - w + 1)
        got = P.records(lo, w)
        both = (lo <= first) & (lo + w >= second + 100)
        assert both.any()
        assert np.all(got["longest"][both] == 100) and np.all(got["longest_at"][both] == first - lo[both]), name


def test_excess_within_the_bound_of_exact():
    """|excess - exact| <= (3 L + 1) u exact against exact rational arithmetic, on samples of mixed magnitudes with NaN
    holes and a limit that is no sample: the worst seen is 0.20 of the bound"""
    rng = np.random.default_rng(17)
    x = rng.normal(0, 1, 6000) * 10.0 ** rng.integers(-3, 6, 6000)
    x[rng.random(6000) < 0.03] = np.nan
    x[3000:3050] = np.nan
    worst = 0.0
    for op, limit in ((RM.GT, 0.37), (RM.LE, -12.5), (RM.NE, 1e-3)):
        P = M.Pyramid(x, op, limit)
        for w in WIDTHS + [4097]:
            lo = [v for v in (0, 1, 777, 2047, 2990, 3000, 3049, len(x) - w) if 0 <= v <= len(x) - w]
            got = P.records(lo, w)
            for i, b in enumerate(lo):
                inside, exact = RM.exact_excess(x[b:b + w], op, limit)
                assert int(got[i]["inside"]) == inside
                if inside == 0:
                    assert got[i]["excess"] == 0.0 and not np.signbit(got[i]["excess"])
                    continue
                err, bound = abs(Fraction(float(got[i]["excess"])) - exact), Fraction(M.bound_factor(w)) * exact
                assert err <= bound, (op, b, w, float(err), float(bound))
                if bound:
                    worst = max(worst, float(err / bound))
    print("largest error / bound:", worst)
    assert 0.0 < worst < 1.0


def test_integer_data_is_exact_and_equals_the_windowed_runs(streams):
    x = streams["planted"]
    for op, limit in ((RM.GT, LIMIT), (RM.NE, LIMIT), (RM.LE, 3.0)):
        P = M.Pyramid(x, op, limit)
        for w in WIDTHS:
            lo = sorted({0, 1, 2, 40, 49, 50, 2046, 2047, 2048, 2100, 4096, 4150, len(x) - w} & set(range(len(x) - w + 1)))
            got = P.records(lo, w)
            want = RM.windows_runs(x, [(b, w) for b in lo], op, limit)
            assert got.tobytes() == want.tobytes(), (op, w)
            for i, b in enumerate(lo):
                assert Fraction(float(got[i]["excess"])) == RM.exact_excess(x[b:b + w], op, limit)[1]


def test_runs_merge_folds_disjoint_adjacent_positions(A, streams):
    x = streams["planted"]
    for op in (RM.GT, RM.EQ):
        P = M.Pyramid(x, op, LIMIT)
        for w in (1, 3, 9, 64, 300):
            rec, off = P.rolling([2], [len(x) - 2], w, w)
            for first, n in ((0, 2), (1, 5), (3, int(off[1]) - 3)):
                n = min(n, 40)
                got = A.runs_merge(rec[first:first + n])
                want = RM.mask_record(RM.inside_mask(x[2 + first * w:2 + (first + n) * w], op, LIMIT))
                assert tuple(int(got[k]) for k in INTS) == want, (op, w, first, n)


def test_symbols_and_surfaces(A):
    lib = A.capi.lib()
    for name in ("atsc_rolling_runs_windows_dev", "atsc_rolling_runs_windows", "atsc_stream_rolling_runs_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES
        assert getattr(lib, name).argtypes == A.capi.SIGNATURES[name][1], name
    assert A.WINDOW_RUNS.itemsize == 80 and A.WINDOW_RUNS.names == RM.FIELDS and M.RECORD == A.WINDOW_RUNS
    want = {(A.Context, "rolling_runs_windows_host"): ["self", "records", "begins", "counts", "width", "op", "limit", "stride", "has_count"],
            (A.DPlan, "rolling_runs_windows"): ["self", "d_body", "begins", "counts", "width", "stride", "op", "limit", "d_out", "stream"],
            (A.CompressedStream, "rolling_runs_windows"): ["self", "begins", "counts", "width", "op", "limit", "stride"],
            (A, "rolling_runs_data_windows"): ["ctx", "bro", "begins", "counts", "width", "op", "limit", "stride"]}
    for (owner, name), params in want.items():
        f = getattr(owner, name)
        assert f.__doc__.strip()
        sig = inspect.signature(f)
        assert list(sig.parameters) == params, name
        assert sig.parameters["stride"].default == (inspect.Parameter.empty if owner is A.DPlan else 1)
    assert A.rolling_runs_data_windows is A.stream.rolling_runs_data_windows


def test_bad_parameters_are_invalid_without_a_gpu(A):
    """a NaN limit, op = 6, width = 0 and stride = 0: ATSC_E_INVALID, with no context and so no device to turn to"""
    lib = A.capi.lib()
    body = (C.c_uint8 * 4)()
    one = (C.c_uint64 * 1)(0)
    cnt = (C.c_uint64 * 1)(10)
    out = np.full(10, 7, dtype=A.WINDOW_RUNS)
    po = C.c_void_p(out.ctypes.data)
    for width, stride, op, limit in ((3, 1, A.RUNS_GT, float("nan")), (3, 1, 6, 0.0), (3, 1, -1, 0.0), (0, 1, A.RUNS_GT, 0.0),
                                     (3, 0, A.RUNS_GT, 0.0)):
        assert lib.atsc_rolling_runs_windows(None, body, 4, 1, 1, one, cnt, width, stride, op, limit, po) == A.capi.E_INVALID
        assert lib.atsc_rolling_runs_windows_dev(None, None, None, 1, one, cnt, width, stride, op, limit, po, None) == A.capi.E_INVALID
        assert lib.atsc_stream_rolling_runs_windows(None, 1, one, cnt, width, stride, op, limit, po) == A.capi.E_INVALID
    assert out.tobytes() == np.full(10, 7, dtype=A.WINDOW_RUNS).tobytes()
