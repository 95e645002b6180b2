"""Windowed extremes on the GPU: every window of every case against the NumPy model of the contract
(tests/extremes_model.py) applied to the GPU's own full decode -- all 2 + 4 k words bit for bit, any NaN equal to any
NaN, no tolerance, no window left out.  The streams, seam windows and piece windows are tests/test_gpu_delta.py's; on top
of them extremes placed by hand (through IDW records with f64 points) at the tile, lane and combine-group seams, ties
between equal values, NaN, signed zeros and +-Inf; k at its edges; the least budget; validation and malformed payloads;
aggregate, runs and extremes calls interleaved on one plan; the dev, host, stream and .bro entry points,
atsc_extremes_merge over buckets, and both command lines.

The placed-pattern stream is 36 x 4096 samples (72 tiles): a tie between tiles 0 and 70 of one window is settled in the
second combine pass."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import extremes_model as M
from tests import helpers as H
from tests import runs_model as RM
from tests.test_gpu_delta import (LARGE, PIECE, SMALL, A, _idw_record, _rec, _rows, _run, _seam_windows,  # noqa: F401
                                  _windows, ctx, decoded, large, mixed, torch)

pytestmark = pytest.mark.gpu

T = M.TILE
inf, nan = float("inf"), float("nan")
NONE = M.NONE


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _bit1(v):
    return int(np.float64(v).view(np.uint64))


def _equal(got, want):
    """all words equal; any NaN equals any NaN"""
    return len(got) == len(want) and got.dtype == want.dtype and np.array_equal(M.words(got), M.words(want))


def _check(full, wins, got, k, label="", want=None):
    """every window against the model on the full decode"""
    assert len(got) == len(wins) and got.dtype == M.dtype(k), label
    if want is None:
        want = M.windows_extremes(full, wins, k)
    gw, ww = M.words(got), M.words(want)
    for i, (b, c) in enumerate(wins):
        assert np.array_equal(gw[i], ww[i]), (label, k, b, c, got[i], want[i])
    return want


def _dev(A, ctx, torch, recs, wins, k, dp=None):
    own = dp is None
    if own:
        dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    d_out = torch.full((max(len(wins), 1) * (2 + 4 * k),), -1, dtype=torch.int64, device="cuda")
    dp.extremes_windows(body, [w[0] for w in wins], [w[1] for w in wins], k, d_out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(A.window_extremes_dtype(k))[: len(wins)].copy()
    if own:
        dp.close()
    return out


def _host(ctx, recs, wins, k):
    return ctx.extremes_windows_host(recs, [w[0] for w in wins], [w[1] for w in wins], k)


def _entries(r, name):
    """the filled entries of a list as (value, at)"""
    return [(float(e["value"]), int(e["at"])) for e in r[name] if int(e["at"]) != NONE]


@pytest.mark.parametrize("which", ["mixed", "large"])
def test_parity_with_full_decode(A, ctx, torch, decoded, which):
    recs, full = decoded[which]
    total = len(full)
    assert total == (sum(SMALL) * 35 if which == "mixed" else sum(LARGE))
    wins = _windows(total, np.random.default_rng(23))
    b, c = [w[0] for w in wins], [w[1] for w in wins]
    want16 = M.windows_extremes(full, wins, 16)
    got = {}
    for k in (1, 3, 16):
        got[k] = _host(ctx, recs, wins, k)
        _check(full, wins, got[k], k, which, want=M.head_of(want16, k))
        assert _equal(_dev(A, ctx, torch, recs, wins, k), got[k]), k
    assert _equal(M.head_of(got[16], 3), got[3]) and _equal(M.head_of(got[16], 1), got[1])
    st = ctx.aggregate_windows_host(recs, b, c)
    some = got[3]["count"] - got[3]["nans"] > 0
    assert some.sum() > 100 and np.array_equal(got[3]["count"], np.array(c, dtype=np.uint64))
    for k in (1, 3, 16):
        assert np.array_equal(got[k]["largest"]["value"][some, 0], st["max"][some]), k  # as values
        assert np.array_equal(got[k]["smallest"]["value"][some, 0], st["min"][some]), k
    whole = wins.index((0, total))
    assert total > 64 * T and int(got[16]["count"][whole]) == total  # more than one combine group: two passes


LANE5 = [512 * q + 2 * (5 + 64 * kk) + e for q in range(4) for kk in range(4) for e in range(2)]  # one lane's 32 slots


def _placed():
    """36 x 4096 samples in [0, 1) with larger and smaller values at the places the kernels can go wrong.  Every value
    has at most five decimals, which the IDW decode's rounding to 1e-5 keeps bit for bit"""
    n = 36 * 4096
    x = np.random.default_rng(71).integers(0, 100000, n) / 100000.0
    x[2 * T] = 50.0             # slot 0, a window's first sample
    x[2 * T + 2047] = 51.0      # slot 2047, a window's last sample
    x[3 * T] = 52.0             # slot 2048 of the stream's second record
    x[3 * T + 2047] = -5.0
    x[4 * T] = -6.0
    x[5 * T + 99] = 1000.0      # in front of and behind the window (5 T + 100, 300), in its tile
    x[5 * T + 400] = 1000.0
    x[5 * T + 99 + 1] = -7.5    # the window's first and last sample are its smallest
    x[5 * T + 399] = -7.5
    x[8 * T + 7] = 77.0         # equal values in two tiles
    x[9 * T + 9] = 77.0
    x[5] = 88.0                 # ... and in tiles 0 and 70 of one window
    x[70 * T + 3] = 88.0
    x[10 * T + 20] = x[10 * T + 21] = 60.0    # one lane's two adjacent slots
    x[11 * T + 30] = x[11 * T + 542] = 61.0   # one lane's slots 512 apart
    x[12 * T + 126] = x[12 * T + 128] = 62.0  # lane 63 and lane 0: position order is not lane order
    x[12 * T + 127] = x[12 * T + 129] = -4.0
    for r, s in enumerate(LANE5):             # the whole top 32 inside one lane's slots, in no order
        x[14 * T + s] = 70.0 + ((r * 7) % 32) / 32.0
    x[16 * T:17 * T] = 5.0                    # a constant tile
    for t in range(70):                       # 70 copies of the minimum, one per tile
        x[t * T + 1000 + t] = -9.0
    for t in range(4):                        # k entries from k different tiles
        x[(20 + t) * T + 100 * (t + 1)] = 40.0 + t
    x[25 * T + 10:25 * T + 20] = nan          # an all-NaN window
    x[26 * T + 49] = nan                      # NaN on both sides of a maximum
    x[26 * T + 50] = 45.0
    x[26 * T + 51] = nan
    x[27 * T + 100:27 * T + 108] = [0.0, -0.0, 0.0, -0.0, -0.0, 0.0, 0.5, -0.0]
    x[65536 - 1] = 30.0                       # on both sides of a piece boundary under the least budget
    x[65536] = 30.0
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
    rng = np.random.default_rng(73)
    wins = _seam_windows(n)
    wins += [(2 * T, T), (2 * T, T + 1), (2 * T + 1, T - 1), (2 * T - 3, T + 6), (3 * T, T), (3 * T + 2047, 2), (4 * T, 1),
             (5 * T + 100, 300), (5 * T + 99, 302), (5 * T + 100, 301), (5 * T, T), (8 * T, 2 * T), (8 * T + 7, T + 3),
             (0, 71 * T), (0, 72 * T), (6, 71 * T - 6), (10 * T, T), (10 * T + 20, 2), (11 * T, T), (11 * T + 30, 513),
             (12 * T, T), (12 * T + 126, 3), (12 * T + 100, 60), (14 * T, T), (14 * T - 100, T + 200), (13 * T, 3 * T),
             (16 * T, T), (16 * T + 5, T - 5), (15 * T + 2000, T + 100), (20 * T, 4 * T), (20 * T + 100, 3 * T + 301),
             (25 * T + 10, 10), (25 * T + 9, 12), (25 * T + 10, 1), (26 * T + 49, 3), (26 * T, T), (27 * T + 100, 8),
             (27 * T + 100, 4), (27 * T + 101, 5), (27 * T + 90, 30), (65535, 2), (65536 - 100, 200), (65000, 3000),
             (71 * T, T), (71 * T + 5, 6), (71 * T + 5, 2), (71 * T + 6, 1), (71 * T + 8, 1),
             (30 * T + 5, 6 * T), (31 * T + 700, 6 * T), (33 * T + 10, 2 * T + 77), (33 * T, T)]  # shared mid tiles
    for at in (2 * T, 3 * T - 1, 5 * T + 100, 70 * T + 3, 25 * T + 10):  # counts 0 .. 3 on and around a placed sample
        wins += [(at, c) for c in (0, 1, 2, 3)] + [(at - 1, c) for c in (1, 2, 3)] + [(at + 1, c) for c in (1, 2)]
    wins += [(int(b), int(rng.integers(0, 9000))) for b in rng.integers(0, n - 9000, 30)]
    return wins


def test_placed_patterns(A, ctx, torch, placed):
    recs, full = placed
    n = len(full)
    wins = _placed_windows(n)
    r = {}
    want16 = M.windows_extremes(full, wins, 16)
    for k in (4, 16):
        got = _host(ctx, recs, wins, k)
        _check(full, wins, got, k, "placed", want=M.head_of(want16, k))
        assert _equal(_dev(A, ctx, torch, recs, wins, k), got), k
        r[k] = dict(zip(wins, got))
    e = r[4]

    def lg(w, k=4):
        return _entries(r[k][w], "largest")

    def sm(w, k=4):
        return _entries(r[k][w], "smallest")

    assert lg((2 * T, T))[:2] == [(51.0, 2047), (50.0, 0)]                    # slot 2047 and slot 0, last and first sample
    assert lg((2 * T, T + 1))[:3] == [(52.0, T), (51.0, 2047), (50.0, 0)]     # slot 2048
    assert lg((2 * T + 1, T - 1))[0] == (51.0, 2046) and lg((2 * T + 1, T - 1))[1][0] < 1.0
    assert sm((3 * T + 2047, 2)) == [(-6.0, 1), (-5.0, 0)] and lg((3 * T + 2047, 2)) == [(-5.0, 0), (-6.0, 1)]
    assert lg((5 * T + 100, 300))[0][0] < 1.0                                  # the 1000s at begin - 1 and begin + count
    assert sm((5 * T + 100, 300))[:2] == [(-7.5, 0), (-7.5, 299)]              # first and last sample
    assert lg((5 * T + 99, 302))[:2] == [(1000.0, 0), (1000.0, 301)]
    assert lg((5 * T + 100, 301))[0] == (1000.0, 300) and lg((5 * T + 100, 301))[1][0] < 1.0
    assert lg((8 * T, 2 * T))[:2] == [(77.0, 7), (77.0, T + 9)]               # a tie over two tiles: the earliest first
    assert lg((0, 71 * T)) == [(1000.0, 5 * T + 99), (1000.0, 5 * T + 400), (88.0, 5), (88.0, 70 * T + 3)]  # tiles 0, 70
    assert lg((6, 71 * T - 6))[2:] == [(88.0, 70 * T + 3 - 6), (77.0, 8 * T + 7 - 6)]
    assert sm((0, 71 * T)) == [(-9.0, t * T + 1000 + t) for t in range(4)]     # 70 copies over 70 tiles: the first four
    assert sm((0, 72 * T), 16)[0] == (-inf, 71 * T + 6) and sm((0, 72 * T), 16)[2:] == [(-9.0, t * T + 1000 + t) for t in range(14)]
    assert lg((10 * T, T))[:2] == [(60.0, 20), (60.0, 21)] and lg((10 * T + 20, 2)) == [(60.0, 0), (60.0, 1)]
    assert lg((11 * T, T))[:2] == [(61.0, 30), (61.0, 542)]
    assert lg((12 * T, T))[:2] == [(62.0, 126), (62.0, 128)] and sm((12 * T, T))[:3] == [(-9.0, 1012), (-4.0, 127), (-4.0, 129)]
    assert sm((12 * T + 126, 3)) == [(-4.0, 1), (62.0, 0), (62.0, 2)]
    top = sorted(LANE5, key=lambda s: (-full[14 * T + s], s))
    assert lg((14 * T, T), 16) == [(float(full[14 * T + s]), s) for s in top[:16]]  # all sixteen from one lane
    assert lg((16 * T, T)) == [(5.0, j) for j in range(4)]                     # a constant tile: the first k positions
    assert sm((16 * T, T))[0] == (-9.0, 1016) and sm((16 * T, T))[1:] == [(5.0, j) for j in range(3)]
    assert lg((20 * T, 4 * T)) == [(43.0, 3 * T + 400), (42.0, 2 * T + 300), (41.0, T + 200), (40.0, 100)]  # four tiles
    a = e[(25 * T + 10, 10)]
    assert (int(a["count"]), int(a["nans"])) == (10, 10) and lg((25 * T + 10, 10)) == [] and sm((25 * T + 10, 10)) == []
    assert np.all(np.isnan(a["largest"]["value"])) and np.all(a["smallest"]["at"] == NONE)
    assert lg((26 * T + 49, 3)) == [(45.0, 1)] == sm((26 * T + 49, 3)) and int(e[(26 * T + 49, 3)]["nans"]) == 2
    z = e[(27 * T + 100, 4)]  # 0.0 -0.0 0.0 -0.0: equal as values, position decides, bits kept
    for name in ("largest", "smallest"):
        assert z[name]["at"].tolist() == [0, 1, 2, 3]
        assert _bits(z[name]["value"]).tolist() == _bits([0.0, -0.0, 0.0, -0.0]).tolist()
    z = e[(27 * T + 100, 8)]  # 0 -0 0 -0 -0 0 0.5 -0
    assert z["largest"]["at"].tolist() == [6, 0, 1, 2] and z["smallest"]["at"].tolist() == [0, 1, 2, 3]
    assert _bits(z["largest"]["value"]).tolist() == _bits([0.5, 0.0, -0.0, 0.0]).tolist()
    assert lg((71 * T + 5, 6)) == [(inf, 0), (inf, 4), (1.0, 2), (-inf, 1)]    # +-Inf are ordinary values
    assert sm((71 * T + 5, 6)) == [(-inf, 1), (-inf, 5), (1.0, 2), (inf, 0)] and int(e[(71 * T + 5, 6)]["nans"]) == 1
    assert lg((71 * T + 8, 1)) == [] and int(e[(71 * T + 8, 1)]["nans"]) == 1
    assert lg((65535, 2)) == [(30.0, 0), (30.0, 1)]                            # across sample 65536
    for c in (0, 1, 2, 3):  # windows of 0 .. 3 samples with k = 4
        w = e[(2 * T, c)]
        assert int(w["count"]) == c and len(lg((2 * T, c))) == c == len(sm((2 * T, c)))
        assert np.all(w["largest"]["at"][c:] == NONE) and np.all(np.isnan(w["smallest"]["value"][c:]))
    assert lg((2 * T, 3))[0] == (50.0, 0) and sm((2 * T, 3))[2] == (50.0, 0)   # one sample in both lists
    # two overlapping windows share mid tiles 32 .. 35; the third one's head tile, 33, is one of them
    assert lg((33 * T + 10, 2 * T + 77))[0][0] < 1.0 and sm((33 * T, T))[0] == (-9.0, 1033)
    assert sm((30 * T + 5, 6 * T))[:4] == [(-9.0, t * T + 1000 + t - 30 * T - 5) for t in (30, 31, 32, 33)]
    assert sm((31 * T + 700, 6 * T))[:4] == [(-9.0, t * T + 1000 + t - 31 * T - 700) for t in (31, 32, 33, 34)]


def test_64_and_66_tiles_in_one_window(A, ctx, torch):
    """64 partials fill one combine group exactly, 65 and 66 need a second pass: windows of 64 and 66 tiles (135168
    samples) and their neighbours, on tile multiples and on odd slots, under the default budget and under the least one,
    whose pieces of 32 tiles cut every one of them"""
    nan = float("nan")
    n = 35 * 4096
    rng = np.random.default_rng(644)
    # decoding rounds to the fifth decimal, so the samples are placed on it; a sum of these depends on its order
    x = np.round(rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 7, n), 5)
    x[rng.integers(0, n, 300)] = nan
    x[rng.integers(0, n, 500)] = 9.0e7   # the largest value many times over, in most tiles: the earliest win
    x[rng.integers(0, n, 500)] = -9.0e7
    recs = b"".join(_idw_record(x[k:k + 4096].tolist()) for k in range(0, n, 4096))
    full = ctx.decompress_host(recs)
    assert np.array_equal(np.isnan(full), np.isnan(x)) and np.array_equal(full[~np.isnan(x)], x[~np.isnan(x)])
    wins = [(2 * T, 64 * T), (2 * T - 1, 64 * T + 2), (T, 66 * T), (2 * T + 1, 66 * T - 1), (2 * T, 64 * T - 1),
            (2 * T + 1, 64 * T), (0, n), (T + 7, 65 * T), (3 * T, 64 * T), (2 * T, 65 * T), (5, 64 * T)]
    try:
        for budget in (0, 1):
            ctx.set_aggregate_scratch(budget)
            for k in (1, 4, 16):
                got = _host(ctx, recs, wins, k)
                _check(full, wins, got, k, "64 tiles, budget %d" % budget)
                assert _equal(_dev(A, ctx, torch, recs, wins, k), got), (budget, k)
    finally:
        ctx.set_aggregate_scratch(0)


def test_k_at_the_edges(A, ctx, torch, placed):
    recs, full = placed
    wins = [(14 * T - 100, T + 200), (0, len(full)), (27 * T + 100, 8), (16 * T, T), (25 * T + 10, 10), (3, 0)]
    want = M.windows_extremes(full, wins, 16)
    for k in (1, 2, 15, 16):
        got = _host(ctx, recs, wins, k)
        _check(full, wins, got, k, "edges", want=M.head_of(want, k))
        assert _equal(_dev(A, ctx, torch, recs, wins, k), got), k
    assert _entries(want[2], "largest")[:3] == [(0.5, 6), (0.0, 0), (-0.0, 1)] and len(_entries(want[2], "largest")) == 8


@pytest.mark.parametrize("which", ["mixed", "large"])
def test_pieces(A, ctx, torch, decoded, which):
    """the least budget: pieces of 65536 samples.  The default budget's records bit for bit, by the host call and
    repeatedly on one plan"""
    recs, full = decoded[which]
    total = len(full)
    rng = np.random.default_rng(31)
    wins = [(1000, 200000), (PIECE, 70000), (PIECE, 1), (PIECE, 2), (PIECE - 10, 10), (0, PIECE), (PIECE - 1, 2),
            (PIECE - 1, 1), (PIECE - 2, 2), (PIECE - 1, PIECE + 2), (2 * PIECE - 1, 2), (2 * PIECE - T, 2 * T),
            (2 * PIECE, T), (PIECE + 1, 5), (0, total), (5, 0), (3 * PIECE - 1, 3), (PIECE - T - 1, 2 * T + 2)]
    wins += [(int(b), int(rng.integers(0, 150000))) for b in rng.integers(0, total - 150000, 10)]
    wins += [(int(b), 60) for b in rng.integers(PIECE - 100, PIECE + 100, 10)]
    for k in (4, 16):
        alone = _host(ctx, recs, wins, k)
        _check(full, wins, alone, k, which)
        dp = A.DPlan(ctx, recs)
        try:
            for budget in (1, 1 << 20):  # 65536 and 131072 samples a piece
                ctx.set_aggregate_scratch(budget)
                assert _equal(_host(ctx, recs, wins, k), alone), budget
                assert _equal(_dev(A, ctx, torch, recs, wins, k, dp), alone), budget
                assert _equal(_dev(A, ctx, torch, recs, wins[:1], k, dp), alone[:1]), budget  # the tables reused
                assert _equal(_dev(A, ctx, torch, recs, wins[6:9], k, dp), alone[6:9]), budget
                assert _equal(_dev(A, ctx, torch, recs, wins[14:15], 1, dp), M.head_of(alone[14:15], 1)), budget
        finally:
            ctx.set_aggregate_scratch(0)
        assert _equal(_dev(A, ctx, torch, recs, wins, k, dp), alone)
        assert len(_dev(A, ctx, torch, recs, [], k, dp)) == 0
        dp.close()


def test_placed_patterns_under_the_least_budget(A, ctx, torch, placed):
    recs, full = placed
    wins = [(0, len(full)), (65535, 2), (65536 - 100, 200), (0, 71 * T), (30 * T + 5, 6 * T), (31 * T + 700, 6 * T)]
    alone = _host(ctx, recs, wins, 4)
    _check(full, wins, alone, 4, "placed")
    try:
        ctx.set_aggregate_scratch(1)
        assert _equal(_host(ctx, recs, wins, 4), alone)
        assert _equal(_dev(A, ctx, torch, recs, wins, 4), alone)
    finally:
        ctx.set_aggregate_scratch(0)


def test_validation(A, ctx, torch):
    n, nf = 256, 8
    x = H.synth_series(1909, n * nf, klass=2)
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
    _check(good, outside, _host(ctx, bad, outside, K), K, "outside")
    lib = A.capi.lib()
    bb = np.frombuffer(bad, dtype=np.uint8)
    gb = np.frombuffer(recs, dtype=np.uint8)
    p = C.POINTER(C.c_uint64)
    FILL = 0x0707070707070707

    def raw(buf, wins, k=K):
        out = np.full(max(len(wins), 1) * (2 + 4 * 17), FILL, dtype=np.uint64)
        b = np.array([w[0] for w in wins], dtype=np.uint64)
        c = np.array([w[1] for w in wins], dtype=np.uint64)
        rc = lib.atsc_extremes_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(wins),
                                       b.ctypes.data_as(p), c.ctypes.data_as(p), k, C.c_void_p(out.ctypes.data))
        return rc, out

    for wins in ([(3 * n, 1)], [(0, nf * n)], [(0, 10), (3 * n - 1, 2)], [(4 * n - 1, 1), (6 * n, 5)]):
        rc, out = raw(bb, wins)
        assert rc == A.capi.E_FORMAT and np.all(out == FILL), (wins, rc)
    for wins in ([(nf * n - 2, 4)], [(0, 5), (nf * n + 1, 0)], [(2 ** 63, 2 ** 63)]):
        rc, out = raw(gb, wins)
        assert rc == A.capi.E_INVALID and np.all(out == FILL), (wins, rc)
    for k in (0, 17, 2 ** 32 - 1):
        for wins in ([(0, 5)], [(0, 0)], []):
            rc, out = raw(gb, wins, k)
            assert rc == A.capi.E_INVALID and np.all(out == FILL), (k, wins)
    rc, _ = raw(gb, [])
    assert rc == 0
    e = _host(ctx, recs, [(5, 0), (nf * n, 0)], K)
    assert _equal(e, M.windows_extremes(good, [(5, 0), (nf * n, 0)], K)) and np.all(e["largest"]["at"] == NONE)
    assert len(_host(ctx, recs, [], K)) == 0
    for k in (0, 17):
        with pytest.raises(A.AtscError):
            _host(ctx, recs, [(0, 5)], k)
    # the device call: a bad k, a window beyond the plan, a misaligned or null result, a null plan -- nothing enqueued
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(gb.copy()).to("cuda")
    d_out = torch.full((2 * (2 + 4 * 17) + 1,), -1, dtype=torch.int64, device="cuda")
    one = np.array([0], dtype=np.uint64)
    cnt = np.array([nf * n + 1], dtype=np.uint64)

    def dev(h_dp, d_body, nw, b, c, ptr, k=K):
        return lib.atsc_extremes_windows_dev(ctx._h, h_dp, C.c_void_p(d_body), nw, b.ctypes.data_as(p), c.ctypes.data_as(p),
                                             k, C.c_void_p(ptr), None)

    assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    cnt[0] = 10
    assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr() + 4) == A.capi.E_INVALID
    assert dev(dp._h, body.data_ptr(), 1, one, cnt, 0) == A.capi.E_INVALID
    assert dev(None, body.data_ptr(), 1, one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    for k in (0, 17):
        assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr(), k) == A.capi.E_INVALID
        assert dev(dp._h, body.data_ptr(), 0, one, cnt, d_out.data_ptr(), k) == A.capi.E_INVALID
    assert dev(dp._h, body.data_ptr(), 0, one, cnt, d_out.data_ptr()) == 0  # n_windows == 0
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())
    for k in (1, 16):  # the edges of k are valid; a result that is only 8-byte aligned
        assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr() + 8, k) == 0
        torch.cuda.synchronize()
        h = d_out.cpu().numpy()
        got = h[1:1 + 2 + 4 * k].copy().view(A.window_extremes_dtype(k))
        assert _equal(got, M.windows_extremes(good, [(0, 10)], k)) and h[0] == -1 and np.all(h[1 + 2 + 4 * k:] == -1)
        d_out.fill_(-1)
    dp.close()


def test_interleaved_with_aggregates_and_runs(A, ctx, torch, decoded):
    """aggregate, runs and extremes calls on one plan, enqueued back to back and three times over: the aggregate and runs
    results are the bytes of plans that never saw an extremes call, the extremes results those of a plan of their own"""
    recs, full = decoded["mixed"]
    total = len(full)
    rng = np.random.default_rng(59)
    wa = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, total - 100000, 30)] + [(0, total)]
    we = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, total - 100000, 40)] + [(7, total - 7)]
    lim = float(np.median(full))
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(method, words, wins, *params):
        d = torch.full((len(wins) * words,), -1, dtype=torch.int64, device="cuda")
        method(body, [w[0] for w in wins], [w[1] for w in wins], *params, d, s)
        return d

    def alone(name, words, wins, *params):
        dp = A.DPlan(ctx, recs)
        d = call(getattr(dp, name), words, wins, *params)
        torch.cuda.synchronize()
        out = d.cpu().numpy().tobytes()
        dp.close()
        return out

    a_alone, r_alone = alone("aggregate_windows", 6, wa), alone("runs_windows", 10, wa, RM.GT, lim)
    e_alone = _dev(A, ctx, torch, recs, we, 5)
    _check(full, we, e_alone, 5, "alone")
    dp = A.DPlan(ctx, recs)
    outs = []
    for _ in range(3):
        outs.append((call(dp.aggregate_windows, 6, wa), call(dp.extremes_windows, 22, we, 5),
                     call(dp.runs_windows, 10, wa, RM.GT, lim), call(dp.extremes_windows, 66, wa, 16),
                     call(dp.aggregate_windows, 6, we[:5]), call(dp.extremes_windows, 6, we, 1)))
    torch.cuda.synchronize()
    want16 = M.windows_extremes(full, wa, 16)
    for a, e, r, e2, _, e3 in outs:
        assert a.cpu().numpy().tobytes() == a_alone
        assert r.cpu().numpy().tobytes() == r_alone
        assert _equal(e.cpu().numpy().view(M.dtype(5)), e_alone)
        assert _equal(e2.cpu().numpy().view(M.dtype(16)), want16)
        assert _equal(e3.cpu().numpy().view(M.dtype(1)), M.head_of(e_alone, 1))
    dp.close()


def test_entry_points_agree(A, ctx, torch, oracle, golden_dir):
    rng = np.random.default_rng(61)
    for name in ("go_gc_heap_goal_bytes", "uptime"):
        x = H.read_wbro(os.path.join(golden_dir, "wbros", name + ".wbro"))
        for comp, err in ((oracle.AUTO, 3), (oracle.FFT, 1), (oracle.NOOP, 0)):
            bro = oracle.compress_data(x, comp, err)
            full = A.decompress_data(ctx, bro)
            _, frames = H.parse_bro(bro)
            wins = _windows(len(full), rng, n_random=15, longest=len(full))
            b = [w[0] for w in wins]
            c = [w[1] for w in wins]
            for k in (2, 16):
                via_bro = A.extremes_data_windows(ctx, bro, b, c, k)
                _check(full, wins, via_bro, k, name)
                records = bro[9:]  # with the frame-count varint
                assert _equal(ctx.extremes_windows_host(records, b, c, k, has_count=True), via_bro), (name, comp)
                s = A.CompressedStream.from_bytes(ctx, bro)
                assert _equal(s.extremes_windows(b, c, k), via_bro), (name, comp)
                n0, p0 = H.varint_decode(bro, 9)
                assert n0 == len(frames)
                assert _equal(_dev(A, ctx, torch, bro[p0:], wins, k), via_bro), (name, comp)
                # the buckets of a range fold into the range's own record: all words
                for (b0, c0), bucket in (((0, len(full)), 60), ((0, len(full)), 2048), ((37, len(full) - 100), 1000)):
                    bb, bc = A.bucket_windows(b0, c0, bucket)
                    parts = A.extremes_data_windows(ctx, bro, bb, bc, k)
                    whole = A.extremes_data_windows(ctx, bro, [b0], [c0], k)
                    folded = A.extremes_merge(parts, k)
                    assert np.array_equal(M.words(folded), M.words(whole)), (name, comp, b0, c0, bucket, k)
    s = A.CompressedStream(ctx)  # a stream without a frame holds only empty windows at 0
    e = s.extremes_windows([0, 0], [0, 0], 3)
    assert len(e) == 2 and _equal(e, M.windows_extremes(np.zeros(0), [(0, 0), (0, 0)], 3))
    with pytest.raises(A.AtscError):
        s.extremes_windows([0], [1], 3)
    for k in (0, 17):
        with pytest.raises(A.AtscError):
            s.extremes_windows([0], [0], k)


def _cols(k):
    return ",nans" + "".join(",%s%d,%s%d_at" % (e, j, e, j) for e in ("max", "min") for j in range(1, k + 1))


def _got_cols(rows, k):
    """the 1 + 4 k new columns: nans, then per entry the value's bits and the place; an empty entry as (None, None)"""
    out = []
    for r in rows:
        cells = r[-(1 + 4 * k):]
        row = [int(cells[0])]
        for j in range(2 * k):
            v, at = cells[1 + 2 * j], cells[2 + 2 * j]
            row += [_bit1(float(v)) if v else None, int(at) if at else None]
        out.append(row)
    return out


def _want_cols(d, place=int):
    out = []
    for r in d:
        row = [int(r["nans"])]
        for name in ("largest", "smallest"):
            for e in r[name]:
                if int(e["at"]) == NONE:
                    row += [None, None]
                else:
                    row += [_bit1(e["value"]), place(int(e["at"]))]
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
    seen = set()
    for extra, (b0, c0), nb, more, k in (
            ((), (0, len(full)), 60, (), 3),
            (("--samples", "100:50"), (100, 50), 7, ("--runs", "gt:0.5", "--deltas", "--moments"), 16),
            ((), (0, len(full)), len(full) + 1, ("--deltas",), 1)):
        _run(atsc, "-u", "--buckets", nb, *extra, *more, tmp_path / "uptime.bro")
        plain = open(tmp_path / "uptime.agg.csv").read()
        _run(atsc, "-u", "--buckets", nb, "--extremes", k, *extra, *more, tmp_path / "uptime.bro")
        text = open(tmp_path / "uptime.agg.csv").read()
        head, rows = _rows(tmp_path / "uptime.agg.csv")
        cols = _cols(k)
        # without the flag the file is what it was: the new columns come after all the others
        assert head.endswith(cols) and head[: -len(cols)] == plain.split("\n")[0]
        assert [",".join(r[:-(1 + 4 * k)]) for r in rows] == [l for l in plain.split("\n")[1:] if l], (extra, nb)
        assert text.endswith("\n")
        bb, bc = A.bucket_windows(b0, c0, nb)
        assert [int(r[0]) for r in rows] == bb.tolist()
        d = A.extremes_data_windows(ctx, bro, bb, bc, k)
        _check(full, list(zip(bb.tolist(), bc.tolist())), d, k, "atsc")
        assert _got_cols(rows, k) == _want_cols(d), (extra, nb)
        seen |= {v is None for r in _got_cols(rows, k) for v in r[1:]}
    assert seen == {True, False}  # empty entries and filled ones were both written
    # csv-compressor -u --from --to --step --extremes on the reference's cpu_utilization values and times
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
    for t0, t1, step, more, k in ((times[0], times[-1], 600, (), 2),
                                  (times[10] + 1, times[50] - 1, 60, ("--runs", "le:%r" % lim, "--deltas", "--moments"), 5)):
        for f in tmp_path.glob("win*"):
            f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, *more, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        plain = open(tmp_path / "win.agg.csv").read()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "--extremes", k, *more, "-o", tmp_path / "win",
             tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.agg.csv"]
        head, got = _rows(tmp_path / "win.agg.csv")
        cols = _cols(k)
        assert head == plain.split("\n")[0] + cols
        assert [",".join(r[:-(1 + 4 * k)]) for r in got] == [l for l in plain.split("\n")[1:] if l]
        wb, wc = index.step_windows(int(t0), int(t1), int(step))
        d = A.extremes_data_windows(ctx, cbro, wb, wc, k)
        _check(all_vals, list(zip(wb.tolist(), wc.tolist())), d, k, "csv-compressor")
        want = []
        for r, b in zip(d, wb.tolist()):  # every place as the indexed time of its sample
            want += _want_cols([r], place=lambda o: int(index.get_time(b + o)))
        assert _got_cols(got, k) == want, (t0, t1, step)
        assert (d["count"] - d["nans"] >= 1).any()
