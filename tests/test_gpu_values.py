"""Windowed value counts on the GPU: every window of every case against the NumPy model of the contract
(tests/values_model.py) applied to the GPU's own full decode -- all 4 + 2 k words bit for bit, any NaN equal to any NaN,
no tolerance, no window left out.  The streams, seam windows and piece windows are tests/test_gpu_delta.py's; on top of
them a five-level state series under the auto selector, values placed by hand (through IDW records with f64 points) at
the tile, lane and combine-group seams, signed zeros, +-Inf and NaN; paging with `above`; the least budget; validation
and malformed payloads; aggregate, extremes and value-count calls interleaved on one plan; the dev, host, stream and
.bro entry points, atsc_values_merge over buckets, and both command lines.

The placed-pattern stream is 36 x 4096 samples (72 tiles): a window over all of them needs two combine passes."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import runs_model as RM
from tests import values_model as M
from tests.test_gpu_delta import (LARGE, PIECE, SMALL, A, _idw_record, _rec, _rows, _run, _seam_windows,  # noqa: F401
                                  _windows, ctx, decoded, large, mixed, torch)

pytestmark = pytest.mark.gpu

T = M.TILE
inf, nan = float("inf"), float("nan")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _equal(got, want):
    """all words equal; any NaN equals any NaN"""
    return len(got) == len(want) and got.dtype == want.dtype and np.array_equal(M.words(got), M.words(want))


def _check(full, wins, got, k, above=nan, label="", want=None):
    """every window against the model on the full decode"""
    assert len(got) == len(wins) and got.dtype == M.dtype(k), label
    if want is None:
        want = M.windows_values(full, wins, k, above)
    gw, ww = M.words(got), M.words(want)
    for i, (b, c) in enumerate(wins):
        assert np.array_equal(gw[i], ww[i]), (label, k, above, b, c, got[i], want[i])
    return want


def _dev(A, ctx, torch, recs, wins, k, above=nan, dp=None):
    own = dp is None
    if own:
        dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    d_out = torch.full((max(len(wins), 1) * (4 + 2 * k),), -1, dtype=torch.int64, device="cuda")
    dp.values_windows(body, [w[0] for w in wins], [w[1] for w in wins], k, d_out, above, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(A.window_values_dtype(k))[: len(wins)].copy()
    if own:
        dp.close()
    return out


def _host(ctx, recs, wins, k, above=nan):
    return ctx.values_windows_host(recs, [w[0] for w in wins], [w[1] for w in wins], k, above)


def _entries(r):
    """the filled entries as (value, n)"""
    return [(float(e["value"]), int(e["n"])) for e in r["entry"][: int(r["distinct"])]]


def _unique(v):
    """np.unique of the non-NaN samples with the zeros as one +0.0 -> [(value, n)]"""
    v = np.asarray(v, dtype=np.float64)
    u, c = np.unique(v[~np.isnan(v)] + 0.0, return_counts=True)
    return [(float(a), int(b)) for a, b in zip(u, c)]


@pytest.mark.parametrize("which", ["mixed", "large"])
def test_parity_with_full_decode(A, ctx, torch, decoded, which):
    recs, full = decoded[which]
    total = len(full)
    assert total == (sum(SMALL) * 35 if which == "mixed" else sum(LARGE))
    wins = _windows(total, np.random.default_rng(29))
    b, c = [w[0] for w in wins], [w[1] for w in wins]
    st = ctx.aggregate_windows_host(recs, b, c)
    identity = 0
    for above in (nan, float(np.median(full[~np.isnan(full)]))):
        want32 = M.windows_values(full, wins, 32, above)
        got = {}
        for k in (1, 3, 32):
            got[k] = _host(ctx, recs, wins, k, above)
            _check(full, wins, got[k], k, above, which, want=M.head_of(want32, k))
            assert _equal(_dev(A, ctx, torch, recs, wins, k, above), got[k]), (k, above)
            try:  # the least budget: pieces of 65536 samples, the same bytes
                ctx.set_aggregate_scratch(1)
                assert _equal(_host(ctx, recs, wins, k, above), got[k]), (k, above)
            finally:
                ctx.set_aggregate_scratch(0)
        # the header's consequences: the prefix rule ...
        assert _equal(M.head_of(got[32], 3), got[3]) and _equal(M.head_of(got[32], 1), got[1]) and _equal(M.head_of(got[3], 1), got[1])
        assert np.array_equal(got[3]["count"], np.array(c, dtype=np.uint64))
        for k in (1, 3, 32):  # ... count == nans + below + sum n where more == 0 ...
            r = got[k]
            done = r["more"] == 0
            assert np.array_equal(r["count"][done], (r["nans"] + r["below"] + r["entry"]["n"].sum(axis=1))[done]), k
            identity += int(done.sum())
        some = got[3]["distinct"] > 0
        if math.isnan(above):  # ... entry[0] is the aggregates' min, as a value ...
            assert some.sum() > 100 and np.array_equal(some, got[3]["count"] > got[3]["nans"])
            assert not got[3]["below"].any()
            for k in (1, 3, 32):
                assert np.array_equal(got[k]["entry"]["value"][some, 0], st["min"][some]), k
        # ... and the n of a listed value is the runs' inside under EQ
        for i in np.flatnonzero(some)[:12]:
            for v, n in _entries(got[3][i]):
                rr = ctx.runs_windows_host(recs, [b[i]], [c[i]], RM.EQ, v)
                assert int(rr["inside"][0]) == n, (wins[i], v, n)
    assert identity > 100
    whole = wins.index((0, total))
    assert total > 64 * T and int(got[32]["count"][whole]) == total  # more than one combine group: two passes


def test_a_state_series(A, ctx, torch):
    """five levels with long dwell times under the auto selector: RLE or Constant frames, 60-sample buckets and the
    whole stream, the buckets' records folded into the whole window's"""
    rng = np.random.default_rng(83)
    n, frame, K = 61440 + 77, 256, 8
    levels = np.array([0.0, 1.0, 2.0, 3.0, 503.0])
    x = np.empty(n)
    at = 0
    while at < n:
        d = int(rng.integers(200, 3000))
        x[at:at + d] = levels[int(rng.integers(0, 5))]
        at += d
    off = H.frame_offsets(n, frame)
    recs, _, chosen, _ = ctx.compress_host(x, off, A.AUTO, True, 0.0, 0)
    assert np.isin(chosen, [A.RLE, A.CONSTANT]).any(), np.unique(chosen)
    full = ctx.decompress_host(recs)
    bb, bc = A.bucket_windows(0, n, 60)
    wins = list(zip(bb.tolist(), bc.tolist()))
    parts = _host(ctx, recs, wins, K)
    whole = _host(ctx, recs, [(0, n)], K)
    assert _equal(_dev(A, ctx, torch, recs, wins, K), parts) and _equal(_dev(A, ctx, torch, recs, [(0, n)], K), whole)
    assert not parts["more"].any() and int(whole["more"][0]) == 0
    for r, (b, c) in zip(parts, wins):
        assert _entries(r) == _unique(full[b:b + c]), (b, c)
    assert _entries(whole[0]) == _unique(full) and 2 <= int(whole["distinct"][0]) <= K
    assert int(parts["distinct"].max()) >= 2 and int(parts["distinct"].min()) == 1  # buckets across a change, and inside a dwell
    assert np.array_equal(M.words(A.values_merge(parts, K)), M.words(whole))
    assert np.array_equal(M.words(A.values_merge(parts[np.random.default_rng(5).permutation(len(parts))], K)), M.words(whole))
    m = A.values_mode(whole, K)
    assert (float(m["value"][0]), int(m["n"][0])) == max(_unique(full), key=lambda e: (e[1], -e[0])) and int(m["exact"][0]) == 1


LANE5 = [512 * q + 2 * (5 + 64 * kk) + e for q in range(4) for kk in range(4) for e in range(2)]  # one lane's 32 slots


ONCE = [t for t in range(72) if t not in (16, 71)]  # the 70 tiles that hold one copy of the smallest value


def _placed():
    """36 x 4096 samples, most of them one of 3000 values in [10, 40), with smaller and larger values at the places the
    kernels can go wrong.  Every value has at most five decimals, which the IDW decode's rounding to 1e-5 keeps bit for
    bit"""
    n = 36 * 4096
    x = np.random.default_rng(79).integers(1000, 4000, n) / 100.0
    x[16 * T:17 * T] = 5.0                      # a constant tile
    # tiles 40 .. 47 hold three values and the once-per-tile one: exactly four; the next tile brings a fifth
    x[40 * T:48 * T] = np.array([6.0, 6.25, 6.5])[np.random.default_rng(81).integers(0, 3, 8 * T)]
    # tile 50 holds 42 distinct values, so its own list overflows; the smallest values of (50 T, 3 T) lie in tile 52
    x[50 * T:52 * T] = 9.5
    x[50 * T:50 * T + 40] = 20.0 + np.arange(40.0)
    x[52 * T:53 * T] = np.array([7.0, 7.25, 7.5])[np.random.default_rng(82).integers(0, 3, T)]
    for t in ONCE:                              # one value once per tile in 70 tiles: both combine passes
        x[t * T + 1000 + t] = -9.0
    x[2 * T] = 1.5                              # only at slot 0, a window's first sample
    x[2 * T + 2047] = 1.25                      # only at slot 2047, a window's last sample
    x[5 * T + 99] = 2.5                         # just in front of the window (5 T + 100, 300), in its tile ...
    x[5 * T + 100] = 2.5                        # ... and at its first sample
    x[5 * T + 399] = 2.75                       # at its last sample ...
    x[5 * T + 400] = 2.75                       # ... and just behind it
    x[10 * T + 20] = x[10 * T + 21] = 3.5       # one lane's two adjacent slots
    x[11 * T + 30] = x[11 * T + 542] = 3.25     # one lane's slots 512 apart
    x[12 * T + 126] = x[12 * T + 128] = 3.75    # lane 63 and lane 0
    for r, s in enumerate(LANE5):               # 32 distinct values below the rest inside one lane's slots, in no order
        x[14 * T + s] = 4.0 + ((r * 7) % 32) / 32.0
    # four values above the rest in the first 64 tiles, a fifth only in tile 66: the second combine group of (0, 66 T + 1)
    x[T + 1500] = x[20 * T + 1501] = 100.0
    x[3 * T + 1502] = x[3 * T + 1600] = 101.0
    x[33 * T + 1503] = 102.0
    x[63 * T + 2047] = 103.0
    x[66 * T] = 104.0
    x[25 * T + 10:25 * T + 20] = nan            # a NaN stretch: an all-NaN window
    x[27 * T + 100:27 * T + 108] = [0.0, -0.0, 0.0, -0.0, -0.0, 0.0, 0.5, -0.0]
    x[65536 - 1] = 8.0                          # equal values on both sides of a piece boundary under the least budget
    x[65536] = 8.0
    x[71 * T + 5:71 * T + 11] = [inf, -inf, 1.0, nan, inf, -inf]
    return x


@pytest.fixture(scope="module")
def placed(ctx):
    x = _placed()
    recs = b"".join(_idw_record(x[k:k + 4096].tolist()) for k in range(0, len(x), 4096))
    full = ctx.decompress_host(recs)
    ok = ~np.isnan(x)
    assert np.array_equal(np.isnan(full), ~ok) and np.array_equal(_bits(full[ok]), _bits(x[ok]))
    return recs, full


def _placed_windows(n):
    rng = np.random.default_rng(89)
    wins = _seam_windows(n)
    wins += [(2 * T, T), (2 * T, T + 1), (2 * T + 1, T - 1), (2 * T + 1, T - 2), (2 * T - 3, T + 6), (2 * T, 1), (2 * T + 2047, 1),
             (5 * T + 100, 300), (5 * T + 99, 302), (5 * T + 101, 298), (5 * T, T), (0, 70 * T), (0, 71 * T), (0, 72 * T),
             (T, 69 * T), (1001, 70 * T), (10 * T, T), (10 * T + 20, 2), (10 * T + 21, 5), (11 * T, T), (11 * T + 30, 513),
             (11 * T + 31, 512), (12 * T, T), (12 * T + 126, 3), (12 * T + 127, 2), (14 * T, T), (14 * T - 100, T + 200),
             (13 * T, 3 * T), (16 * T, T), (16 * T + 5, T - 5), (15 * T + 2000, T + 100), (16 * T, 1016), (16 * T + 1017, 1031),
             (40 * T, 8 * T), (40 * T, 8 * T + 1), (40 * T - 1, 8 * T + 1), (41 * T + 5, 3 * T), (50 * T, 3 * T), (50 * T + 40, 3 * T - 40),
             (50 * T, T), (51 * T, 2 * T), (25 * T + 10, 10), (25 * T + 9, 12), (25 * T + 10, 1), (27 * T + 100, 8),
             (27 * T + 100, 4), (27 * T + 101, 5), (27 * T + 90, 30), (65535, 2), (65536 - 100, 200), (65000, 3000),
             (71 * T, T), (71 * T + 5, 6), (71 * T + 5, 2), (71 * T + 6, 1), (71 * T + 8, 1),
             (30 * T + 5, 6 * T), (31 * T + 700, 6 * T), (33 * T + 10, 2 * T + 77), (33 * T, T)]  # shared mid tiles
    for at in (2 * T, 3 * T - 1, 5 * T + 100, 70 * T + 1070, 66 * T, 25 * T + 10):  # counts 0 .. 3 on and around a placed sample
        wins += [(at, c) for c in (0, 1, 2, 3)] + [(at - 1, c) for c in (1, 2, 3)] + [(at + 1, c) for c in (1, 2)]
    wins += [(int(b), int(rng.integers(0, 9000))) for b in rng.integers(0, n - 9000, 30)]
    return wins


def test_placed_patterns(A, ctx, torch, placed):
    recs, full = placed
    n = len(full)
    wins = _placed_windows(n)
    r = {}
    want32 = M.windows_values(full, wins, 32)
    for k in (4, 5, 32):
        got = _host(ctx, recs, wins, k)
        _check(full, wins, got, k, nan, "placed", want=M.head_of(want32, k))
        assert _equal(_dev(A, ctx, torch, recs, wins, k), got), k
        r[k] = dict(zip(wins, got))

    def en(w, k=4):
        return _entries(r[k][w])

    def more(w, k=4):
        return int(r[k][w]["more"])

    assert en((2 * T, T))[:3] == [(-9.0, 1), (1.25, 1), (1.5, 1)]               # slot 2047 and slot 0, last and first sample
    assert en((2 * T + 1, T - 1))[:2] == [(-9.0, 1), (1.25, 1)] and en((2 * T + 1, T - 1))[2][0] >= 10.0
    assert en((2 * T + 1, T - 2))[0] == (-9.0, 1) and en((2 * T + 1, T - 2))[1][0] >= 10.0
    assert en((2 * T, 1)) == [(1.5, 1)] and en((2 * T + 2047, 1)) == [(1.25, 1)]
    assert en((5 * T + 100, 300))[:2] == [(2.5, 1), (2.75, 1)]                  # the copies just outside are not counted
    assert en((5 * T + 99, 302))[:2] == [(2.5, 2), (2.75, 2)]
    assert en((5 * T + 101, 298))[0][0] >= 10.0
    assert en((5 * T, T))[:3] == [(-9.0, 1), (2.5, 2), (2.75, 2)]
    assert en((0, 71 * T))[0] == (-9.0, 70) and en((T, 69 * T))[0] == (-9.0, 68)  # once per tile in 70 tiles, two passes
    assert en((0, 72 * T))[:2] == [(-inf, 2), (-9.0, 70)] and en((1001, 70 * T))[0] == (-9.0, 68)
    assert en((10 * T, T))[:2] == [(-9.0, 1), (3.5, 2)] and en((10 * T + 20, 2)) == [(3.5, 2)]
    assert en((10 * T + 21, 5))[0] == (3.5, 1)
    assert en((11 * T, T))[:2] == [(-9.0, 1), (3.25, 2)] and en((11 * T + 30, 513))[0] == (3.25, 2)
    assert en((11 * T + 31, 512))[0] == (3.25, 1)
    assert en((12 * T, T))[:2] == [(-9.0, 1), (3.75, 2)] and en((12 * T + 126, 3))[0] == (3.75, 2)
    assert en((12 * T + 127, 2))[0] == (3.75, 1)
    lane = sorted(4.0 + j / 32.0 for j in range(32))                            # all of one lane's slots
    assert en((14 * T, T), 32) == [(-9.0, 1)] + [(v, 1) for v in lane[:31]] and more((14 * T, T), 32) == 1
    assert en((16 * T, T)) == [(5.0, T)] and more((16 * T, T)) == 0             # a constant tile: n == 2048
    assert en((16 * T, 1016)) == [(5.0, 1016)] and en((16 * T + 1017, 1031)) == [(5.0, 1031)]  # n == the whole range
    # exactly k distinct values, and k + 1 where the extra one lives in another tile
    w4 = r[4][(40 * T, 8 * T)]
    assert [v for v, _ in _entries(w4)] == [-9.0, 6.0, 6.25, 6.5] and int(w4["more"]) == 0 and int(w4["distinct"]) == 4
    assert sum(m for _, m in _entries(w4)) == 8 * T
    assert more((40 * T, 8 * T + 1)) == 1 and more((40 * T - 1, 8 * T + 1)) == 1 and more((41 * T + 5, 3 * T)) == 0
    assert more((40 * T, 8 * T + 1), 5) == 0 and int(r[5][(40 * T, 8 * T + 1)]["distinct"]) == 5
    # a tile whose own list overflows while the window's first k come from other tiles
    assert more((50 * T, T)) == 1 and en((50 * T, T)) == [(-9.0, 1), (9.5, T - 41), (20.0, 1), (21.0, 1)]
    assert en((50 * T, 3 * T)) == [(-9.0, 3)] + [(v, int((full[52 * T:53 * T] == v).sum())) for v in (7.0, 7.25, 7.5)]
    assert more((50 * T, 3 * T)) == 1 and more((50 * T + 40, 3 * T - 40)) == 1 and more((50 * T + 40, 3 * T - 40), 5) == 0
    assert en((50 * T + 40, 3 * T - 40), 5)[4] == (9.5, 2 * T - 42)
    a = r[4][(25 * T + 10, 10)]                                                 # an all-NaN window
    assert (int(a["count"]), int(a["nans"]), int(a["distinct"]), int(a["more"])) == (10, 10, 0, 0)
    assert np.all(np.isnan(a["entry"]["value"])) and not a["entry"]["n"].any()
    assert int(r[4][(25 * T + 9, 12)]["nans"]) == 10 and int(r[4][(25 * T + 9, 12)]["distinct"]) <= 2
    z = r[4][(27 * T + 100, 8)]  # 0 -0 0 -0 -0 0 0.5 -0: one +0.0 entry
    assert _entries(z) == [(0.0, 7), (0.5, 1)] and _bits(z["entry"]["value"][:1]).tolist() == [0]
    z = r[4][(27 * T + 101, 5)]  # -0 0 -0 -0 0
    assert _entries(z) == [(0.0, 5)] and _bits(z["entry"]["value"][:1]).tolist() == [0]
    assert en((71 * T + 5, 6)) == [(-inf, 2), (1.0, 1), (inf, 2)] and int(r[4][(71 * T + 5, 6)]["nans"]) == 1
    assert en((71 * T + 8, 1)) == [] and int(r[4][(71 * T + 8, 1)]["nans"]) == 1
    assert en((65535, 2)) == [(8.0, 2)]                                         # across sample 65536
    for c in (0, 1, 2, 3):  # windows of 0 .. 3 samples
        w = r[4][(2 * T, c)]
        assert int(w["count"]) == c and sum(m for _, m in _entries(w)) == c
    # two overlapping windows share mid tiles 32 .. 35; the third one's head tile, 33, is one of them
    assert en((30 * T + 5, 6 * T))[0] == (-9.0, 6) and en((31 * T + 700, 6 * T))[0] == (-9.0, 6) and en((33 * T, T))[0] == (-9.0, 1)


def test_placed_patterns_under_the_least_budget(A, ctx, torch, placed):
    recs, full = placed
    wins = [(0, len(full)), (65535, 2), (65536 - 100, 200), (0, 71 * T), (30 * T + 5, 6 * T), (31 * T + 700, 6 * T),
            (40 * T, 8 * T + 1), (50 * T, 3 * T), (0, 66 * T + 1)]
    for k, above in ((4, nan), (32, 6.25)):
        alone = _host(ctx, recs, wins, k, above)
        _check(full, wins, alone, k, above, "placed")
        try:
            ctx.set_aggregate_scratch(1)
            assert _equal(_host(ctx, recs, wins, k, above), alone)
            assert _equal(_dev(A, ctx, torch, recs, wins, k, above), alone)
        finally:
            ctx.set_aggregate_scratch(0)
    assert _entries(alone[1]) == [(8.0, 2)]


def test_the_second_combine_group(A, ctx, torch, placed):
    """above = 99 leaves the five placed values above the rest: a window of 64 tiles lists exactly k = 4 of them, and the
    fifth, in tile 66 only, reaches a longer window through its second combine group alone; above = -9 leaves the 32
    values of one lane as a tile's first 32"""
    recs, full = placed
    wins = [(0, 64 * T), (0, 66 * T), (0, 66 * T + 1), (T, 66 * T), (0, 72 * T), (66 * T, 1), (64 * T, 2 * T), (T + 1501, 65 * T)]
    r = {}
    for k in (4, 5):
        got = _host(ctx, recs, wins, k, 99.0)
        _check(full, wins, got, k, 99.0, "second group")
        assert _equal(_dev(A, ctx, torch, recs, wins, k, 99.0), got), k
        r[k] = dict(zip(wins, got))
    four = [(100.0, 2), (101.0, 2), (102.0, 1), (103.0, 1)]
    for w in ((0, 64 * T), (0, 66 * T)):
        assert _entries(r[4][w]) == four and int(r[4][w]["more"]) == 0 and int(r[4][w]["below"]) == w[1] - 6 - int(np.isnan(full[:w[1]]).sum())
    assert _entries(r[4][(0, 66 * T + 1)]) == four and int(r[4][(0, 66 * T + 1)]["more"]) == 1
    assert _entries(r[5][(0, 66 * T + 1)]) == four + [(104.0, 1)] and int(r[5][(0, 66 * T + 1)]["more"]) == 0
    assert _entries(r[4][(T, 66 * T)]) == four and int(r[4][(T, 66 * T)]["more"]) == 1
    assert _entries(r[5][(0, 72 * T)]) == four + [(104.0, 1)] and int(r[5][(0, 72 * T)]["more"]) == 1  # +Inf is cut
    assert _entries(r[4][(66 * T, 1)]) == [(104.0, 1)] and _entries(r[4][(64 * T, 2 * T)]) == []
    assert _entries(r[4][(T + 1501, 65 * T)]) == [(100.0, 1), (101.0, 2), (102.0, 1), (103.0, 1)]
    got = _host(ctx, recs, [(14 * T, T)], 32, -9.0)
    _check(full, [(14 * T, T)], got, 32, -9.0, "one lane")
    assert _entries(got[0]) == [(4.0 + j / 32.0, 1) for j in range(32)] and int(got[0]["more"]) == 1 and int(got[0]["below"]) == 1


def test_paging(A, ctx, torch, placed):
    """k = 4 and `above` walked from NaN to the last listed value until more == 0: np.unique of the window"""
    recs, full = placed
    for b, c in ((50 * T, T), (27 * T + 90, 30), (71 * T, T), (25 * T + 5, 30)):
        v = full[b:b + c]
        want = _unique(v)
        above, seen, calls, below = nan, [], 0, 0
        while True:
            r = _host(ctx, recs, [(b, c)], 4, above)[0]
            calls += 1
            assert int(r["below"]) == below and int(r["nans"]) == int(np.isnan(v).sum()) and int(r["count"]) == c
            seen += _entries(r)
            below += sum(m for _, m in _entries(r))
            if not int(r["more"]):
                break
            above = seen[-1][0]
        assert seen == want and calls == max(1, -(-len(want) // 4)), (b, c, calls)
        assert below + int(np.isnan(v).sum()) == c
    assert len(_unique(full[50 * T:51 * T])) == 42
    # the special values of above, on the host and the dev call
    wins = [(71 * T, T), (27 * T + 90, 30), (0, len(full)), (71 * T + 5, 6), (3, 0)]
    for above in (0.0, -0.0, inf, -inf, 10.0, -9.0):
        for k in (2, 32):
            got = _host(ctx, recs, wins, k, above)
            _check(full, wins, got, k, above, "above")
            assert _equal(_dev(A, ctx, torch, recs, wins, k, above), got), (k, above)
    e = {a: _host(ctx, recs, [(71 * T + 5, 6), (27 * T + 100, 8)], 4, a) for a in (0.0, -0.0, inf, -inf)}
    assert _entries(e[inf][0]) == [] and int(e[inf][0]["below"]) == 5 and int(e[inf][0]["more"]) == 0
    assert _entries(e[-inf][0]) == [(1.0, 1), (inf, 2)] and int(e[-inf][0]["below"]) == 2
    for z in (0.0, -0.0):  # leaves out the zero class and everything negative
        assert _entries(e[z][0]) == [(1.0, 1), (inf, 2)] and int(e[z][0]["below"]) == 2
        assert _entries(e[z][1]) == [(0.5, 1)] and int(e[z][1]["below"]) == 7


def test_validation(A, ctx, torch):
    n, nf = 256, 8
    x = H.synth_series(1913, n * nf, klass=2)
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.05)), 0)
    good = ctx.decompress_host(recs)
    frames = H.parse_bro_body(recs, with_count=False)
    pos = sum(len(_rec(f[1], f[2], f[3])) for f in frames[:3])
    rec3 = _rec(frames[3][1], frames[3][2], frames[3][3])
    pay = pos + len(rec3) - len(frames[3][3])
    assert recs[pay] == 15 and recs[pay + 1] < 200
    bad = bytearray(recs)
    bad[pay + 1] = 250  # frame 3: more stored bins than the transform has; the record walk stays valid
    bad = bytes(bad)
    K = 3
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 10, 10), (5 * n + 3, 100), (0, 0), (3 * n + 5, 0)]
    _check(good, outside, _host(ctx, bad, outside, K), K, nan, "outside")
    lib = A.capi.lib()
    bb = np.frombuffer(bad, dtype=np.uint8)
    gb = np.frombuffer(recs, dtype=np.uint8)
    p = C.POINTER(C.c_uint64)
    FILL = 0x0707070707070707

    def raw(buf, wins, k=K):
        out = np.full(max(len(wins), 1) * (4 + 2 * 33), FILL, dtype=np.uint64)
        b = np.array([w[0] for w in wins], dtype=np.uint64)
        c = np.array([w[1] for w in wins], dtype=np.uint64)
        rc = lib.atsc_values_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(wins),
                                     b.ctypes.data_as(p), c.ctypes.data_as(p), k, nan, C.c_void_p(out.ctypes.data))
        return rc, out

    for wins in ([(3 * n, 1)], [(0, nf * n)], [(0, 10), (3 * n - 1, 2)], [(4 * n - 1, 1), (6 * n, 5)]):
        rc, out = raw(bb, wins)
        assert rc == A.capi.E_FORMAT and np.all(out == FILL), (wins, rc)
    for wins in ([(nf * n - 2, 4)], [(0, 5), (nf * n + 1, 0)], [(2 ** 63, 2 ** 63)]):
        rc, out = raw(gb, wins)
        assert rc == A.capi.E_INVALID and np.all(out == FILL), (wins, rc)
    for k in (0, 33, 2 ** 32 - 1):
        for wins in ([(0, 5)], [(0, 0)], []):
            rc, out = raw(gb, wins, k)
            assert rc == A.capi.E_INVALID and np.all(out == FILL), (k, wins)
    rc, _ = raw(gb, [])
    assert rc == 0
    e = _host(ctx, recs, [(5, 0), (nf * n, 0)], K)
    assert _equal(e, M.windows_values(good, [(5, 0), (nf * n, 0)], K)) and not M.words(e)[:, :4].any()
    assert np.all(np.isnan(e["entry"]["value"])) and not e["entry"]["n"].any()
    assert len(_host(ctx, recs, [], K)) == 0
    for k in (0, 33):
        with pytest.raises(A.AtscError):
            _host(ctx, recs, [(0, 5)], k)
    # the device call: a bad k, a window beyond the plan, a misaligned or null result, a null plan -- nothing enqueued
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(gb.copy()).to("cuda")
    d_out = torch.full((2 * (4 + 2 * 33) + 1,), -1, dtype=torch.int64, device="cuda")
    one = np.array([0], dtype=np.uint64)
    cnt = np.array([nf * n + 1], dtype=np.uint64)

    def dev(h_dp, d_body, nw, b, c, ptr, k=K):
        return lib.atsc_values_windows_dev(ctx._h, h_dp, C.c_void_p(d_body), nw, b.ctypes.data_as(p), c.ctypes.data_as(p),
                                           k, nan, C.c_void_p(ptr), None)

    assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    cnt[0] = 10
    assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr() + 4) == A.capi.E_INVALID
    assert dev(dp._h, body.data_ptr(), 1, one, cnt, 0) == A.capi.E_INVALID
    assert dev(None, body.data_ptr(), 1, one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    for k in (0, 33):
        assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr(), k) == A.capi.E_INVALID
        assert dev(dp._h, body.data_ptr(), 0, one, cnt, d_out.data_ptr(), k) == A.capi.E_INVALID
    assert dev(dp._h, body.data_ptr(), 0, one, cnt, d_out.data_ptr()) == 0  # n_windows == 0
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())
    for k in (1, 32):  # the edges of k are valid; a result that is only 8-byte aligned
        assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr() + 8, k) == 0
        torch.cuda.synchronize()
        h = d_out.cpu().numpy()
        got = h[1:1 + 4 + 2 * k].copy().view(A.window_values_dtype(k))
        assert _equal(got, M.windows_values(good, [(0, 10)], k)) and h[0] == -1 and np.all(h[1 + 4 + 2 * k:] == -1)
        d_out.fill_(-1)
    dp.close()


def test_interleaved_with_aggregates_and_extremes(A, ctx, torch, decoded):
    """aggregate, extremes and value-count calls on one plan, enqueued back to back and three times over: the aggregate
    and extremes results are the bytes of plans that never saw a value-count call, the value counts those of a plan of
    their own"""
    recs, full = decoded["mixed"]
    total = len(full)
    rng = np.random.default_rng(67)
    wa = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, total - 100000, 30)] + [(0, total)]
    wv = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, total - 100000, 40)] + [(7, total - 7)]
    mid = float(np.median(full))
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(method, words, wins, *params):
        d = torch.full((len(wins) * words,), -1, dtype=torch.int64, device="cuda")
        method(body, [w[0] for w in wins], [w[1] for w in wins], *params, d, s)
        return d

    def values(dp, wins, k, above):
        d = torch.full((len(wins) * (4 + 2 * k),), -1, dtype=torch.int64, device="cuda")
        dp.values_windows(body, [w[0] for w in wins], [w[1] for w in wins], k, d, above, s)
        return d

    def alone(name, words, wins, *params):
        dp = A.DPlan(ctx, recs)
        d = call(getattr(dp, name), words, wins, *params)
        torch.cuda.synchronize()
        out = d.cpu().numpy().tobytes()
        dp.close()
        return out

    a_alone, e_alone = alone("aggregate_windows", 6, wa), alone("extremes_windows", 2 + 4 * 5, wa, 5)
    v_alone = _dev(A, ctx, torch, recs, wv, 5)
    _check(full, wv, v_alone, 5, nan, "alone")
    dp = A.DPlan(ctx, recs)
    outs = []
    for _ in range(3):
        outs.append((call(dp.aggregate_windows, 6, wa), values(dp, wv, 5, nan), call(dp.extremes_windows, 22, wa, 5),
                     values(dp, wa, 32, mid), call(dp.aggregate_windows, 6, wv[:5]), values(dp, wv, 1, nan)))
    torch.cuda.synchronize()
    want32 = M.windows_values(full, wa, 32, mid)
    for a, v, e, v2, _, v3 in outs:
        assert a.cpu().numpy().tobytes() == a_alone
        assert e.cpu().numpy().tobytes() == e_alone
        assert _equal(v.cpu().numpy().view(M.dtype(5)), v_alone)
        assert _equal(v2.cpu().numpy().view(M.dtype(32)), want32)
        assert _equal(v3.cpu().numpy().view(M.dtype(1)), M.head_of(v_alone, 1))
    dp.close()


def test_entry_points_agree(A, ctx, torch, oracle, golden_dir):
    rng = np.random.default_rng(71)
    for name in ("go_gc_heap_goal_bytes", "uptime"):
        x = H.read_wbro(os.path.join(golden_dir, "wbros", name + ".wbro"))
        for comp, err in ((oracle.AUTO, 3), (oracle.FFT, 1), (oracle.NOOP, 0)):
            bro = oracle.compress_data(x, comp, err)
            full = A.decompress_data(ctx, bro)
            _, frames = H.parse_bro(bro)
            wins = _windows(len(full), rng, n_random=15, longest=len(full))
            b = [w[0] for w in wins]
            c = [w[1] for w in wins]
            for k, above in ((2, nan), (32, float(np.median(full)))):
                via_bro = A.values_data_windows(ctx, bro, b, c, k, above)
                _check(full, wins, via_bro, k, above, name)
                records = bro[9:]  # with the frame-count varint
                assert _equal(ctx.values_windows_host(records, b, c, k, above, has_count=True), via_bro), (name, comp)
                s = A.CompressedStream.from_bytes(ctx, bro)
                assert _equal(s.values_windows(b, c, k, above), via_bro), (name, comp)
                n0, p0 = H.varint_decode(bro, 9)
                assert n0 == len(frames)
                assert _equal(_dev(A, ctx, torch, bro[p0:], wins, k, above), via_bro), (name, comp)
                # the buckets of a range fold into the range's own record, in any order: all words
                for (b0, c0), bucket in (((0, len(full)), 60), ((0, len(full)), 2048), ((37, len(full) - 100), 1000)):
                    bb, bc = A.bucket_windows(b0, c0, bucket)
                    parts = A.values_data_windows(ctx, bro, bb, bc, k, above)
                    whole = A.values_data_windows(ctx, bro, [b0], [c0], k, above)
                    for order in (np.arange(len(parts)), rng.permutation(len(parts))):
                        folded = A.values_merge(parts[order], k)
                        assert np.array_equal(M.words(folded), M.words(whole)), (name, comp, b0, c0, bucket, k)
    s = A.CompressedStream(ctx)  # a stream without a frame holds only empty windows at 0
    e = s.values_windows([0, 0], [0, 0], 3)
    assert len(e) == 2 and _equal(e, M.windows_values(np.zeros(0), [(0, 0), (0, 0)], 3))
    with pytest.raises(A.AtscError):
        s.values_windows([0], [1], 3)
    for k in (0, 33):
        with pytest.raises(A.AtscError):
            s.values_windows([0], [0], k)


def _cols(k):
    return ",nans,below,distinct,more" + "".join(",v%d,n%d" % (j, j) for j in range(1, k + 1))


def _got_cols(rows, k):
    """the 4 + 2 k new columns: the four integers, then per entry the value's bits and n; an unused entry as (None, None)"""
    out = []
    for r in rows:
        cells = r[-(4 + 2 * k):]
        row = [int(v) for v in cells[:4]]
        for j in range(k):
            v, m = cells[4 + 2 * j], cells[5 + 2 * j]
            row += [int(_bits(float(v))[0]) if v else None, int(m) if m else None]
        out.append(row)
    return out


def _want_cols(d):
    out = []
    for r in d:
        row = [int(r["nans"]), int(r["below"]), int(r["distinct"]), int(r["more"])]
        for j, e in enumerate(r["entry"]):
            row += [int(_bits(e["value"])[0]), int(e["n"])] if j < int(r["distinct"]) else [None, None]
        out.append(row)
    return out


def test_command_lines(A, ctx, golden_dir, tmp_path):
    from oracle import vsri_oracle as VO

    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    mid = float(np.median(full))
    seen = set()
    for extra, (b0, c0), nb, more, k, above in (
            ((), (0, len(full)), 60, (), 3, nan),
            (("--samples", "100:50"), (100, 50), 7, ("--runs", "gt:0.5", "--extremes", "2", "--moments"), 32, mid),
            ((), (0, len(full)), len(full) + 1, ("--deltas",), 1, nan)):
        flag = str(k) if math.isnan(above) else "%d:%r" % (k, above)
        _run(atsc, "-u", "--buckets", nb, *extra, *more, tmp_path / "uptime.bro")
        plain = open(tmp_path / "uptime.agg.csv").read()
        _run(atsc, "-u", "--buckets", nb, "--values", flag, *extra, *more, tmp_path / "uptime.bro")
        text = open(tmp_path / "uptime.agg.csv").read()
        head, rows = _rows(tmp_path / "uptime.agg.csv")
        cols = _cols(k)
        # without the flag the file is what it was: the new columns come after all the others
        assert head.endswith(cols) and head[: -len(cols)] == plain.split("\n")[0]
        assert [",".join(r[:-(4 + 2 * k)]) for r in rows] == [l for l in plain.split("\n")[1:] if l], (extra, nb)
        assert text.endswith("\n")
        bb, bc = A.bucket_windows(b0, c0, nb)
        assert [int(r[0]) for r in rows] == bb.tolist()
        d = A.values_data_windows(ctx, bro, bb, bc, k, above)
        _check(full, list(zip(bb.tolist(), bc.tolist())), d, k, above, "atsc")
        assert _got_cols(rows, k) == _want_cols(d), (extra, nb)
        seen |= {v is None for r in _got_cols(rows, k) for v in r[4:]}
    assert seen == {True, False}  # unused entries and filled ones were both written
    # csv-compressor -u --from --to --step --values on the reference's cpu_utilization values and times
    lines = open(os.path.join(golden_dir, "csv", "cpu_utilization.csv")).read().split("\n")[1:]
    rows = [l.split(",") for l in lines if l]
    ts = [int(t) * 1000 for t, _ in rows]
    vals = [float(v) for _, v in rows]
    m = tmp_path / "cpu.csv"
    m.write_text(VO.samples_to_csv_text(ts, vals))
    _run(csvc, "--output-vsri", "--compressor", "fft", "-e", "3", m)
    _run(csvc, "-u", "-o", tmp_path / "all", tmp_path / "cpu.bro")
    all_rows = [r for r in (tmp_path / "all.csv").read_text().split("\n")[1:] if r]
    all_vals = A.wbro_read(tmp_path / "all.wbro")
    times = np.array([int(r.split(",")[0]) for r in all_rows])
    cbro = (tmp_path / "cpu.bro").read_bytes()
    index = A.Vsri.load(str(tmp_path / "cpu.vsri"))
    lim = float(np.median(all_vals))
    for t0, t1, step, more, k, above in ((times[0], times[-1], 600, (), 2, nan),
                                         (times[10] + 1, times[50] - 1, 60, ("--runs", "le:%r" % lim, "--deltas"), 5, lim)):
        flag = str(k) if math.isnan(above) else "%d:%r" % (k, above)
        for f in tmp_path.glob("win*"):
            f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, *more, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        plain = open(tmp_path / "win.agg.csv").read()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "--values", flag, *more, "-o", tmp_path / "win",
             tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.agg.csv"]
        head, got = _rows(tmp_path / "win.agg.csv")
        cols = _cols(k)
        assert head == plain.split("\n")[0] + cols
        assert [",".join(r[:-(4 + 2 * k)]) for r in got] == [l for l in plain.split("\n")[1:] if l]
        wb, wc = index.step_windows(int(t0), int(t1), int(step))
        d = A.values_data_windows(ctx, cbro, wb, wc, k, above)
        _check(all_vals, list(zip(wb.tolist(), wc.tolist())), d, k, above, "csv-compressor")
        assert _got_cols(got, k) == _want_cols(d), (t0, t1, step)
        assert (d["distinct"] >= 1).any()
