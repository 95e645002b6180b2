"""Windowed runs on the GPU: every window of every case against the NumPy model of the contract (tests/runs_model.py)
applied to the GPU's own full decode -- all ten fields bit for bit, any NaN equal to any NaN, no tolerance, no window
left out.  The streams, seam windows and piece windows are tests/test_gpu_delta.py's; on top of them runs placed by hand
(through IDW records with f64 points) at the tile, ballot-word, combine-group and piece seams, ties between equal runs,
NaN, signed zeros and +-Inf; the least budget; validation and malformed payloads; aggregate, delta and runs calls
interleaved on one plan; the dev, host, stream and .bro entry points, atsc_runs_merge over buckets, and both command
lines.

The placed-pattern stream is 17 x 4096 samples (34 tiles); a run of exactly 64 tiles does not fit it, so that one case
has a stream of its own of 35 x 4096 samples."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import runs_model as M
from tests.test_gpu_delta import (LARGE, PIECE, SMALL, A, _idw_record, _rec, _rows, _run, _seam_windows,  # noqa: F401
                                  _windows, ctx, decoded, large, mixed, torch)

pytestmark = pytest.mark.gpu

T = M.TILE
inf, nan = float("inf"), float("nan")
NONE = M.NONE


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _equal(got, want):
    """the nine integers equal, excess bit for bit; any NaN equals any NaN"""
    if len(got) != len(want):
        return False
    for k in M.FIELDS[:9]:
        if not np.array_equal(got[k], want[k]):
            return False
    g, w = np.ascontiguousarray(got["excess"]), np.ascontiguousarray(want["excess"])
    return bool(np.all((_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))))


def _check(full, wins, got, op, limit, label=""):
    """every window against the model on the full decode"""
    assert len(got) == len(wins), label
    want = M.windows_runs(full, wins, op, limit)
    for i, (b, c) in enumerate(wins):
        assert _equal(got[i:i + 1], want[i:i + 1]), (label, op, limit, b, c, got[i], want[i])
    return want


def _dev(A, ctx, torch, recs, wins, op, limit, dp=None):
    own = dp is None
    if own:
        dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    d_out = torch.full((max(len(wins), 1) * 10,), -1, dtype=torch.int64, device="cuda")
    dp.runs_windows(body, [w[0] for w in wins], [w[1] for w in wins], op, limit, d_out,
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(A.WINDOW_RUNS)[: len(wins)].copy()
    if own:
        dp.close()
    return out


def _host(ctx, recs, wins, op, limit):
    return ctx.runs_windows_host(recs, [w[0] for w in wins], [w[1] for w in wins], op, limit)


def _ints(r):
    return tuple(int(r[k]) for k in M.FIELDS[:9])


@pytest.mark.parametrize("limits", ["median", "exact", "infinite"])
@pytest.mark.parametrize("which", ["mixed", "large"])
def test_parity_with_full_decode(A, ctx, torch, decoded, which, limits):
    recs, full = decoded[which]
    total = len(full)
    assert total == (sum(SMALL) * 35 if which == "mixed" else sum(LARGE))
    assert not np.isnan(full).any()
    wins = _windows(total, np.random.default_rng(23))
    b, c = [w[0] for w in wins], [w[1] for w in wins]
    if limits == "median":
        conds = [(op, float(np.median(full))) for op in M.OPS]
    elif limits == "exact":
        # a value that samples hold exactly (in `mixed`: one of the Noop part, the last fifth, a counter with resets)
        at = total - sum(SMALL) * 7 + 4321 if which == "mixed" else total // 2
        v = float(full[at])
        assert (full == v).sum() >= 1
        conds = [(op, v) for op in (M.GT, M.GE, M.EQ, M.NE)]
    else:
        conds = [(M.GT, -inf), (M.GT, inf)]
    res = {}
    for op, limit in conds:
        got = _host(ctx, recs, wins, op, limit)
        res[op] = _check(full, wins, got, op, limit, which)
        assert _equal(_dev(A, ctx, torch, recs, wins, op, limit), got), (op, limit)
    if limits == "median":
        assert (res[M.GT]["runs"] > 1).sum() > 20 and (res[M.GT]["runs"] == 0).sum() > 2
        st = ctx.aggregate_windows_host(recs, b, c)
        assert np.array_equal(res[M.GT]["inside"] + res[M.LE]["inside"], st["count"])
        assert np.array_equal(res[M.EQ]["inside"] + res[M.NE]["inside"], res[M.EQ]["samples"])
        assert np.array_equal(res[M.GE]["inside"] + res[M.LT]["inside"], np.array(c, dtype=np.uint64))
    elif limits == "exact":
        whole = wins.index((0, total))
        assert res[M.EQ]["inside"][whole] >= 1
        assert res[M.GE]["inside"][whole] == res[M.GT]["inside"][whole] + res[M.EQ]["inside"][whole]
        assert np.array_equal(res[M.EQ]["inside"] + res[M.NE]["inside"], res[M.NE]["samples"])
    else:
        # every finite sample is over -Inf: the whole stream is one run, over 153 / 115 tiles -- more than one combine
        # group of 64 partials, hence two passes; nothing is over +Inf
        whole = wins.index((0, total))
        assert _ints(res[M.GT][whole]) == (total, 0, 0, 0, NONE, NONE, NONE, 0, 0)  # (the last call: GT +Inf)
        allin = _host(ctx, recs, [(0, total), (5, total - 5)], M.GT, -inf)
        assert _ints(allin[0]) == (total, total, 1, total, 0, 0, total - 1, total, total) and allin[0]["excess"] == inf
        assert _ints(allin[1]) == (total - 5, total - 5, 1, total - 5, 0, 0, total - 6, total - 5, total - 5)
        assert total > 64 * T


def _placed():
    """17 x 4096 samples of 0 / 1 (and a few special values) with runs of ones at the places the kernels can go wrong"""
    n = 17 * 4096
    x = np.zeros(n)
    x[T + 2040:2 * T] = 1           # ends at slot 2047
    x[3 * T:3 * T + 5] = 1          # starts at slot 0 (slot 2048 of the stream's second record)
    x[4 * T + 100:4 * T + 107] = 1  # 7 long: as long as the next one, which joins across a tile boundary
    x[5 * T - 3:5 * T + 4] = 1      # straddles 2047 / 2048: 3 + 4
    x[5 * T + 300:5 * T + 307] = 1  # 7 long again, later
    x[7 * T:8 * T] = 1              # exactly one tile
    x[9 * T + 40:9 * T + 64] = 1    # ends at bit 63 of a ballot word
    x[10 * T + 64:10 * T + 100] = 1  # starts at bit 64
    x[10 * T + 120:10 * T + 128] = 1  # ends at bit 127: the end of a load step's 128 slots
    x[11 * T + 128:11 * T + 160] = 1  # starts at bit 128
    x[11 * T + 60:11 * T + 70] = 1  # straddles 63 / 64
    x[12 * T + 120:12 * T + 136] = 1  # straddles 127 / 128
    x[12 * T + 1000:12 * T + 1064] = 1  # 64 long across three words, none of them full
    x[12 * T + 1280:12 * T + 1408] = 1  # two full words
    x[13 * T + 200:13 * T + 230] = 1  # 30 long in a window's head tile ...
    x[15 * T + 500:15 * T + 530] = 1  # ... and 30 long in a shared mid tile
    x[65536 - 5:65536 + 6] = 1      # straddles sample 65536, a piece boundary under the least budget
    x[20 * T + 10:20 * T + 21] = 1
    x[20 * T + 15] = nan            # a NaN in the middle splits the run
    x[22 * T:22 * T + 5] = [-0.0, 0.0, -0.0, 1.0, -0.0]
    x[24 * T:24 * T + 6] = [inf, 1.0, -inf, inf, inf, 0.0]
    x[33 * T + 2000:34 * T] = 1     # reaches the stream's end
    return x


def test_placed_patterns(A, ctx, torch):
    x = _placed()
    n = len(x)
    recs = b"".join(_idw_record(x[k:k + 4096].tolist()) for k in range(0, n, 4096))
    full = ctx.decompress_host(recs)
    assert np.array_equal(np.isnan(full), np.isnan(x)) and np.array_equal(_bits(full[~np.isnan(x)]), _bits(x[~np.isnan(x)]))
    rng = np.random.default_rng(53)
    wins = _seam_windows(n)
    wins += [(T + 2040, 8), (T + 2039, 10), (T + 2040, 9), (3 * T, 5), (3 * T - 1, 7), (3 * T, 4), (4 * T, 2 * T), (5 * T - 10, T),
             (5 * T - 3, 7), (5 * T - 3, 3), (5 * T, 4), (4 * T + 100, T), (7 * T, T), (7 * T - 1, T + 2), (7 * T + 1, T - 1),
             (6 * T, 3 * T), (9 * T, T), (9 * T + 63, 2), (9 * T + 40, 24), (10 * T, T), (10 * T + 64, 64), (10 * T + 127, 2),
             (11 * T, T), (11 * T + 60, 10), (11 * T + 63, 2), (11 * T + 128, 32), (12 * T, T), (12 * T + 127, 2),
             (12 * T + 1000, 64), (12 * T + 1280, 128), (12 * T + 999, 500), (13 * T + 100, 5 * T), (14 * T + 5, 4 * T),
             (13 * T + 200, 30), (13 * T, 3 * T), (65536 - 5, 11), (65536 - 6, 13), (65535, 2), (65536, 6), (65000, 1000),
             (20 * T, 100), (20 * T + 10, 11), (20 * T + 15, 1), (20 * T + 14, 3), (22 * T, 5), (22 * T, 3), (24 * T, 6),
             (24 * T, 1), (24 * T + 2, 3), (33 * T, T), (33 * T + 2000, 48), (n - 1, 1), (0, n), (9 * T, 4 * T)]
    for at in (T + 2047, 3 * T, 5 * T - 1, 7 * T, 65535, 20 * T + 14):  # counts 0 .. 3 on, at the edge of and off a run
        wins += [(at, c) for c in (0, 1, 2, 3)] + [(at - 1, c) for c in (1, 2, 3)] + [(at + 1, c) for c in (1, 2)]
    wins += [(int(b), int(rng.integers(0, 9000))) for b in rng.integers(0, n - 9000, 40)]
    conds = [(M.EQ, 1.0), (M.NE, 1.0), (M.GT, 0.0), (M.GE, 0.0), (M.EQ, 0.0), (M.GT, 0.5), (M.GT, inf), (M.GE, inf),
             (M.LT, inf), (M.LE, -inf), (M.GT, -inf), (M.EQ, -inf)]
    r, first = {}, {}
    try:
        for budget in (0, 1):  # the default, then pieces of 65536 samples: the same records
            ctx.set_aggregate_scratch(budget)
            for op, limit in conds:
                got = _host(ctx, recs, wins, op, limit)
                if budget == 0:
                    _check(full, wins, got, op, limit, "placed")
                    first[(op, limit)] = got
                    r[(op, limit)] = dict(zip(wins, got))
                assert _equal(got, first[(op, limit)]), (budget, op, limit)
                assert _equal(_dev(A, ctx, torch, recs, wins, op, limit), got), (budget, op, limit)
    finally:
        ctx.set_aggregate_scratch(0)
    e = r[(M.EQ, 1.0)]

    def rec(w):
        return _ints(e[w]) + (float(e[w]["excess"]),)

    assert rec((T + 2039, 10)) == (10, 8, 1, 8, 1, 1, 8, 0, 0, 0.0)           # ends at slot 2047, the next tile's slot 0 off
    assert rec((3 * T - 1, 7)) == (7, 5, 1, 5, 1, 1, 5, 0, 0, 0.0)            # starts at slot 0 of a tile
    assert rec((5 * T - 3, 7)) == (7, 7, 1, 7, 0, 0, 6, 7, 7, 0.0)            # joined across the tile boundary
    assert rec((4 * T, 2 * T)) == (2 * T, 21, 3, 7, 100, 100, T + 306, 0, 0, 0.0)  # the joined 7 ties with the earlier 7
    assert rec((5 * T - 10, T)) == (T, 14, 2, 7, 7, 7, 316, 0, 0, 0.0)        # ... and with the later 7: the earliest
    assert rec((7 * T, T)) == (T, T, 1, T, 0, 0, T - 1, T, T, 0.0)            # exactly one tile
    assert rec((7 * T - 1, T + 2)) == (T + 2, T, 1, T, 1, 1, T, 0, 0, 0.0)
    assert rec((11 * T, T)) == (T, 42, 2, 32, 128, 60, 159, 0, 0, 0.0)
    assert rec((12 * T, T)) == (T, 208, 3, 128, 1280, 120, 1407, 0, 0, 0.0)
    assert rec((13 * T + 100, 5 * T)) == (5 * T, 60, 2, 30, 100, 100, 2 * T + 429, 0, 0, 0.0)  # head tile before mid tile
    assert rec((14 * T + 5, 4 * T))[:6] == (4 * T, 30, 1, 30, T + 495, T + 495)  # the mid tile's, shared
    assert rec((65536 - 6, 13)) == (13, 11, 1, 11, 1, 1, 11, 0, 0, 0.0)       # across sample 65536
    assert rec((20 * T + 10, 11)) == (11, 10, 2, 5, 0, 0, 10, 5, 5, 0.0)      # the NaN splits it; of 5 and 5 the earliest
    assert rec((33 * T, T)) == (T, 48, 1, 48, 2000, 2000, T - 1, 0, 48, 0.0)
    assert rec((65535, 0)) == M.EMPTY and rec((65535, 1)) == (1, 1, 1, 1, 0, 0, 0, 1, 1, 0.0)
    assert rec((65535, 2)) == (2, 2, 1, 2, 0, 0, 1, 2, 2, 0.0) and rec((65536, 6)) == (6, 6, 1, 6, 0, 0, 5, 6, 6, 0.0)
    z = (22 * T, 5)  # -0.0 +0.0 -0.0 1.0 -0.0 against 0.0: the zeros are equal to it whatever their sign
    assert _ints(r[(M.GT, 0.0)][z]) == (5, 1, 1, 1, 3, 3, 3, 0, 0) and r[(M.GT, 0.0)][z]["excess"] == 1.0
    assert _ints(r[(M.GE, 0.0)][z]) == (5, 5, 1, 5, 0, 0, 4, 5, 5)
    assert _ints(r[(M.EQ, 0.0)][z]) == (5, 4, 2, 3, 0, 0, 4, 3, 1) and _bits(r[(M.EQ, 0.0)][z]["excess"]) == 0
    w = (24 * T, 6)  # Inf 1 -Inf Inf Inf 0
    assert _ints(r[(M.GT, 0.5)][w]) == (6, 4, 2, 2, 0, 0, 4, 2, 0) and r[(M.GT, 0.5)][w]["excess"] == inf
    assert _ints(r[(M.GT, inf)][w]) == (6, 0, 0, 0, NONE, NONE, NONE, 0, 0) and _bits(r[(M.GT, inf)][w]["excess"]) == 0
    assert _ints(r[(M.GE, inf)][w]) == (6, 3, 2, 2, 3, 0, 4, 1, 0) and np.isnan(r[(M.GE, inf)][w]["excess"])
    assert _ints(r[(M.LT, inf)][w]) == (6, 3, 2, 2, 1, 1, 5, 0, 1) and r[(M.LT, inf)][w]["excess"] == inf
    assert _ints(r[(M.LE, -inf)][w]) == (6, 1, 1, 1, 2, 2, 2, 0, 0) and np.isnan(r[(M.LE, -inf)][w]["excess"])
    assert _ints(r[(M.GT, -inf)][w]) == (6, 5, 2, 3, 3, 0, 5, 2, 3)
    assert _ints(r[(M.NE, 1.0)][(20 * T + 14, 3)]) == (3, 0, 0, 0, NONE, NONE, NONE, 0, 0)  # 1 NaN 1: NaN is not inside


def test_a_run_of_exactly_64_tiles(A, ctx, torch):
    """64 partials fill one combine group exactly; 65 and 66 need a second pass"""
    n = 35 * 4096
    x = np.zeros(n)
    x[2 * T:66 * T] = 1
    x[67 * T + 3] = 1
    recs = b"".join(_idw_record(x[k:k + 4096].tolist()) for k in range(0, n, 4096))
    full = ctx.decompress_host(recs)
    assert np.array_equal(full, x)
    wins = [(2 * T, 64 * T), (2 * T - 1, 64 * T + 2), (T, 66 * T), (2 * T, 64 * T - 1), (2 * T + 1, 64 * T), (0, n),
            (T + 7, 65 * T), (3 * T, 64 * T), (2 * T, 65 * T), (5, 64 * T)]
    got = _host(ctx, recs, wins, M.EQ, 1.0)
    _check(full, wins, got, M.EQ, 1.0, "64 tiles")
    assert _equal(_dev(A, ctx, torch, recs, wins, M.EQ, 1.0), got)
    L = 64 * T
    assert _ints(got[0]) == (L, L, 1, L, 0, 0, L - 1, L, L)
    assert _ints(got[1]) == (L + 2, L, 1, L, 1, 1, L, 0, 0)
    assert _ints(got[5]) == (n, L + 1, 2, L, 2 * T, 2 * T, 67 * T + 3, 0, 0)


@pytest.mark.parametrize("which", ["mixed", "large"])
def test_pieces(A, ctx, torch, decoded, which):
    """the least budget: pieces of 65536 samples.  The window list of the delta test; under GT -Inf the whole-stream window
    crosses every piece boundary with one run.  The default budget's records bit for bit, by the host call and repeatedly
    on one plan"""
    recs, full = decoded[which]
    total = len(full)
    rng = np.random.default_rng(31)
    wins = [(1000, 200000), (PIECE, 70000), (PIECE, 1), (PIECE, 2), (PIECE - 10, 10), (0, PIECE), (PIECE - 1, 2),
            (PIECE - 1, 1), (PIECE - 2, 2), (PIECE - 1, PIECE + 2), (2 * PIECE - 1, 2), (2 * PIECE - T, 2 * T),
            (2 * PIECE, T), (PIECE + 1, 5), (0, total), (5, 0), (3 * PIECE - 1, 3), (PIECE - T - 1, 2 * T + 2)]
    wins += [(int(b), int(rng.integers(0, 150000))) for b in rng.integers(0, total - 150000, 10)]
    wins += [(int(b), 60) for b in rng.integers(PIECE - 100, PIECE + 100, 10)]
    for op, limit in ((M.GT, -inf), (M.GT, float(np.median(full)))):
        alone = _host(ctx, recs, wins, op, limit)
        _check(full, wins, alone, op, limit, which)
        dp = A.DPlan(ctx, recs)
        try:
            for budget in (1, 1 << 20):  # 65536 and 131072 samples a piece
                ctx.set_aggregate_scratch(budget)
                assert _equal(_host(ctx, recs, wins, op, limit), alone), budget
                assert _equal(_dev(A, ctx, torch, recs, wins, op, limit, dp), alone), budget
                assert _equal(_dev(A, ctx, torch, recs, wins[:1], op, limit, dp), alone[:1]), budget  # the tables reused
                assert _equal(_dev(A, ctx, torch, recs, wins[6:9], op, limit, dp), alone[6:9]), budget
        finally:
            ctx.set_aggregate_scratch(0)
        assert _equal(_dev(A, ctx, torch, recs, wins, op, limit, dp), alone)
        assert len(_dev(A, ctx, torch, recs, [], op, limit, dp)) == 0
        dp.close()
        if limit == -inf:
            assert _ints(alone[14]) == (total, total, 1, total, 0, 0, total - 1, total, total)
            assert _ints(alone[0])[:4] == (200000, 200000, 1, 200000)


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
    lim = float(np.median(good))
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 10, 10), (5 * n + 3, 100), (0, 0), (3 * n + 5, 0)]
    _check(good, outside, _host(ctx, bad, outside, M.GT, lim), M.GT, lim, "outside")
    lib = A.capi.lib()
    bb = np.frombuffer(bad, dtype=np.uint8)
    gb = np.frombuffer(recs, dtype=np.uint8)
    p = C.POINTER(C.c_uint64)

    def raw(buf, wins, op=M.GT, limit=lim):
        out = np.full(max(len(wins), 1), 0, dtype=A.WINDOW_RUNS)
        out["excess"] = 7.0
        b = np.array([w[0] for w in wins], dtype=np.uint64)
        c = np.array([w[1] for w in wins], dtype=np.uint64)
        rc = lib.atsc_runs_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(wins),
                                   b.ctypes.data_as(p), c.ctypes.data_as(p), op, limit, C.c_void_p(out.ctypes.data))
        return rc, out

    for wins in ([(3 * n, 1)], [(0, nf * n)], [(0, 10), (3 * n - 1, 2)], [(4 * n - 1, 1), (6 * n, 5)]):
        rc, out = raw(bb, wins)
        assert rc == A.capi.E_FORMAT and np.all(out["excess"] == 7.0) and np.all(out["samples"] == 0), (wins, rc)
    for wins in ([(nf * n - 2, 4)], [(0, 5), (nf * n + 1, 0)], [(2 ** 63, 2 ** 63)]):
        rc, out = raw(gb, wins)
        assert rc == A.capi.E_INVALID and np.all(out["excess"] == 7.0), (wins, rc)
    for op, limit in ((6, lim), (-1, lim), (M.GT, nan), (M.NE, -nan), (99, nan)):
        for wins in ([(0, 5)], [(0, 0)], []):
            rc, out = raw(gb, wins, op, limit)
            assert rc == A.capi.E_INVALID and np.all(out["excess"] == 7.0), (op, limit, wins)
    rc, _ = raw(gb, [])
    assert rc == 0
    e = _host(ctx, recs, [(5, 0), (nf * n, 0)], M.GT, lim)
    for r in e:
        assert _ints(r) == M.EMPTY[:9] and _bits(r["excess"]) == 0
    assert len(_host(ctx, recs, [], M.GT, lim)) == 0
    with pytest.raises(A.AtscError):
        _host(ctx, recs, [(0, 5)], 6, lim)
    # the device call: a bad condition, a window beyond the plan, a misaligned result, a null argument -- nothing enqueued
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(gb.copy()).to("cuda")
    d_out = torch.full((21,), -1, dtype=torch.int64, device="cuda")
    one = np.array([0], dtype=np.uint64)
    cnt = np.array([nf * n + 1], dtype=np.uint64)

    def dev(h_dp, d_body, nw, b, c, ptr, op=M.GT, limit=lim):
        return lib.atsc_runs_windows_dev(ctx._h, h_dp, C.c_void_p(d_body), nw, b.ctypes.data_as(p), c.ctypes.data_as(p),
                                         op, limit, C.c_void_p(ptr), None)

    assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    cnt[0] = 10
    assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr() + 4) == A.capi.E_INVALID
    assert dev(dp._h, body.data_ptr(), 1, one, cnt, 0) == A.capi.E_INVALID
    assert dev(None, body.data_ptr(), 1, one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    for op, limit in ((6, lim), (-1, lim), (M.GT, nan)):
        assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr(), op, limit) == A.capi.E_INVALID
        assert dev(dp._h, body.data_ptr(), 0, one, cnt, d_out.data_ptr(), op, limit) == A.capi.E_INVALID
    assert dev(dp._h, body.data_ptr(), 0, one, cnt, d_out.data_ptr()) == 0  # n_windows == 0
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())
    for op, limit in ((M.LE, inf), (M.GE, -inf)):  # an infinite limit is valid
        assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr(), op, limit) == 0
        torch.cuda.synchronize()
        assert d_out.cpu().numpy()[:9].tolist() == [10, 10, 1, 10, 0, 0, 9, 10, 10]
    dp.close()


def test_interleaved_with_aggregates_and_deltas(A, ctx, torch, decoded):
    """aggregate, delta and runs calls on one plan, enqueued back to back and three times over: the aggregate and delta
    results are the bytes of plans that never saw a runs call, the runs results those of a plan of their own"""
    recs, full = decoded["mixed"]
    total = len(full)
    rng = np.random.default_rng(59)
    wa = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, total - 100000, 30)] + [(0, total)]
    wr = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, total - 100000, 40)] + [(7, total - 7)]
    lim = float(np.median(full))
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(method, words, wins, *cond):
        d = torch.full((len(wins) * words,), -1, dtype=torch.int64, device="cuda")
        method(body, [w[0] for w in wins], [w[1] for w in wins], *cond, d, s)
        return d

    def alone(name, words, wins):
        dp = A.DPlan(ctx, recs)
        d = call(getattr(dp, name), words, wins)
        torch.cuda.synchronize()
        out = d.cpu().numpy().tobytes()
        dp.close()
        return out

    a_alone, d_alone = alone("aggregate_windows", 6, wa), alone("delta_windows", 8, wa)
    r_alone = _dev(A, ctx, torch, recs, wr, M.GT, lim)
    _check(full, wr, r_alone, M.GT, lim, "alone")
    dp = A.DPlan(ctx, recs)
    outs = []
    for _ in range(3):
        outs.append((call(dp.aggregate_windows, 6, wa), call(dp.runs_windows, 10, wr, M.GT, lim),
                     call(dp.delta_windows, 8, wa), call(dp.runs_windows, 10, wa, M.LE, lim),
                     call(dp.aggregate_windows, 6, wr[:5])))
    torch.cuda.synchronize()
    for a, r, d, r2, _ in outs:
        assert a.cpu().numpy().tobytes() == a_alone
        assert d.cpu().numpy().tobytes() == d_alone
        assert _equal(r.cpu().numpy().view(A.WINDOW_RUNS), r_alone)
        _check(full, wa, r2.cpu().numpy().view(A.WINDOW_RUNS), M.LE, lim, "second")
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
            for op, limit in ((M.GT, float(np.median(full))), (M.LE, float(full[len(full) // 3]))):
                via_bro = A.runs_data_windows(ctx, bro, b, c, op, limit)
                _check(full, wins, via_bro, op, limit, name)
                records = bro[9:]  # with the frame-count varint
                assert _equal(ctx.runs_windows_host(records, b, c, op, limit, has_count=True), via_bro), (name, comp)
                s = A.CompressedStream.from_bytes(ctx, bro)
                assert _equal(s.runs_windows(b, c, op, limit), via_bro), (name, comp)
                n0, p0 = H.varint_decode(bro, 9)
                assert n0 == len(frames)
                assert _equal(_dev(A, ctx, torch, bro[p0:], wins, op, limit), via_bro), (name, comp)
            # the buckets of a range fold into the range's own record: the nine integers exactly
            op, limit = M.GT, float(np.median(full))
            for (b0, c0), bucket in (((0, len(full)), 60), ((0, len(full)), 2048), ((37, len(full) - 100), 1000)):
                bb, bc = A.bucket_windows(b0, c0, bucket)
                parts = A.runs_data_windows(ctx, bro, bb, bc, op, limit)
                whole = A.runs_data_windows(ctx, bro, [b0], [c0], op, limit)[0]
                folded = A.runs_merge(parts)
                assert _ints(folded) == _ints(whole), (name, comp, b0, c0, bucket)
                assert _ints(folded) == M.merge_all([tuple(p) for p in parts])[:9]
    s = A.CompressedStream(ctx)  # a stream without a frame holds only empty windows at 0
    e = s.runs_windows([0, 0], [0, 0], M.GT, 1.0)
    assert all(_ints(r) == M.EMPTY[:9] and _bits(r["excess"]) == 0 for r in e) and len(e) == 2
    with pytest.raises(A.AtscError):
        s.runs_windows([0], [1], M.GT, 1.0)
    with pytest.raises(A.AtscError):
        s.runs_windows([0], [0], 6, 1.0)
    with pytest.raises(A.AtscError):
        s.runs_windows([0], [0], M.GT, nan)


COLS = ",inside,runs,longest,longest_at,first_at,last_at,head,tail,excess"


def _got_cols(rows):
    """the nine new columns: integers (an empty position as None), excess as bits"""
    return [[int(v) if v else None for v in r[-9:-1]] + [int(_bits(float(r[-1])))] for r in rows]


def _want_cols(d, place=int):
    out = []
    for r in d:
        pos = [None if int(r[k]) == NONE else place(int(r[k])) for k in ("longest_at", "first_at", "last_at")]
        e = np.float64(r["excess"])
        out.append([int(r["inside"]), int(r["runs"]), int(r["longest"])] + pos + [int(r["head"]), int(r["tail"]),
                   int(_bits(np.nan if np.isnan(e) else e))])
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
    # (uptime is 1 while the process is up: over 0.5 nearly everywhere, under it nearly nowhere)
    for extra, (b0, c0), nb, more, flag, op, lim in (
            ((), (0, len(full)), 60, (), "gt:0.5", M.GT, 0.5),
            (("--samples", "100:1500"), (100, 1500), 1000, ("--deltas", "--moments"), "lt:0.5", M.LT, 0.5),
            ((), (0, len(full)), len(full) + 1, ("--deltas",), "ne:%r" % float(full[7]), M.NE, float(full[7]))):
        _run(atsc, "-u", "--buckets", nb, *extra, *more, tmp_path / "uptime.bro")
        plain = open(tmp_path / "uptime.agg.csv").read()
        _run(atsc, "-u", "--buckets", nb, "--runs", flag, *extra, *more, tmp_path / "uptime.bro")
        text = open(tmp_path / "uptime.agg.csv").read()
        head, rows = _rows(tmp_path / "uptime.agg.csv")
        # without the flag the file is what it was: the new columns come after all the others
        assert head.endswith(COLS) and head[: -len(COLS)] == plain.split("\n")[0]
        assert [",".join(r[:-9]) for r in rows] == [l for l in plain.split("\n")[1:] if l], (extra, nb)
        assert text.endswith("\n")
        bb, bc = A.bucket_windows(b0, c0, nb)
        assert [int(r[0]) for r in rows] == bb.tolist()
        d = A.runs_data_windows(ctx, bro, bb, bc, op, lim)
        _check(full, list(zip(bb.tolist(), bc.tolist())), d, op, lim, "atsc")
        assert _got_cols(rows) == _want_cols(d), (extra, nb)
        seen |= {v is None for r in _got_cols(rows) for v in r[3:6]}
    assert seen == {True, False}  # empty positions and filled ones were both written
    # csv-compressor -u --from --to --step --runs on the reference's cpu_utilization values and times
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
    for t0, t1, step, more in ((times[0], times[-1], 600, ()), (times[10] + 1, times[50] - 1, 60, ("--deltas",))):
        for f in tmp_path.glob("win*"):
            f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, *more, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        plain = open(tmp_path / "win.agg.csv").read()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "--runs", "le:%r" % lim, *more, "-o", tmp_path / "win",
             tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.agg.csv"]
        head, got = _rows(tmp_path / "win.agg.csv")
        assert head == plain.split("\n")[0] + COLS
        assert [",".join(r[:-9]) for r in got] == [l for l in plain.split("\n")[1:] if l]
        wb, wc = index.step_windows(int(t0), int(t1), int(step))
        d = A.runs_data_windows(ctx, cbro, wb, wc, M.LE, lim)
        _check(all_vals, list(zip(wb.tolist(), wc.tolist())), d, M.LE, lim, "csv-compressor")
        want = []
        for r, b in zip(d, wb.tolist()):  # the three positions as the indexed times of their samples
            want += _want_cols([r], place=lambda o: int(index.get_time(b + o)))
        assert _got_cols(got) == want, (t0, t1, step)
        assert (d["runs"] >= 1).any()
