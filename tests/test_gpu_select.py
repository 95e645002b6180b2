"""Windowed select on the GPU: every call against the NumPy model of the contract (tests/select_model.py) applied to the
GPU's own full decode -- offsets equal, entry values by their uint64 bits, `at` equal, no tolerance, no window left
out.  The streams, seam windows and piece length are tests/test_gpu_delta.py's; on top of them hits placed by hand
(through IDW records with f64 points) at the task and load-step seams, NaN, signed zeros and +-Inf; truncation by `cap`
with a guard behind the block; the least budget; enough tasks for several blocks of the scan; validation and malformed
payloads; select, runs and aggregate calls interleaved on one plan; the dev, host, stream and .bro entry points and both
command lines."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import select_model as M
from tests.test_gpu_delta import (LARGE, PIECE, SMALL, A, _idw_record, _rec, _run, _seam_windows,  # noqa: F401
                                  _windows, ctx, decoded, large, mixed, torch)
from tests.test_gpu_histogram import GAP_WINS, gaps  # noqa: F401  (windows that leave gaps, and their stream)

pytestmark = pytest.mark.gpu

TASK = 2048  # SEL_TASK: samples of a task, counted from the window's begin (or from a piece's start inside the window)
inf, nan = float("inf"), float("nan")
SENT = -0x0123456789ABCDF  # the guard words behind a device block


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _equal(got, want):
    """offsets equal, the entries' values bit for bit, their positions equal"""
    return (np.array_equal(got[0], want[0]) and len(got[1]) == len(want[1]) and
            np.array_equal(_bits(got[1]["value"]), _bits(want[1]["value"])) and np.array_equal(got[1]["at"], want[1]["at"]))


def _check(full, wins, got, op, limit, cap, label=""):
    """a call against the model on the full decode, window by window"""
    want = M.windows_select(full, wins, op, limit, cap)
    assert np.array_equal(got[0], want[0]), (label, op, limit, cap)
    assert len(got[1]) == len(want[1]) == min(int(want[0][-1]), cap), (label, op, limit, cap)
    if not _equal(got, want):
        for i, (b, c) in enumerate(wins):  # name the first window that differs
            lo, hi = int(want[0][i]), min(int(want[0][i + 1]), cap)
            assert _equal((want[0], got[1][lo:hi]), (want[0], want[1][lo:hi])), (label, op, limit, cap, i, b, c)
    return want


def _dev(A, ctx, torch, recs, wins, op, limit, cap, dp=None, body=None):
    """the device call into a block with eight guard words behind it, which must stay as they were"""
    own = dp is None
    if own:
        dp = A.DPlan(ctx, recs)
    if body is None:
        body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    n, words = len(wins), A.select_bytes(len(wins), cap) // 8
    d = torch.full((words + 8,), SENT, dtype=torch.int64, device="cuda")
    dp.select_windows(body, [w[0] for w in wins], [w[1] for w in wins], op, limit, cap, d,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    if own:
        dp.close()
    assert (h[words:] == SENT).all(), "written behind the block"
    if n == 0:
        assert (h == SENT).all()
        return np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=A.SELECTED)
    off = h[: n + 1].view(np.uint64).copy()
    m = min(int(off[n]), cap)
    return off, h[n + 1: n + 1 + 2 * m].copy().view(A.SELECTED)


def _host(ctx, recs, wins, op, limit, cap=None):
    return ctx.select_windows_host(recs, [w[0] for w in wins], [w[1] for w in wins], op, limit, cap)


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
        at = total - sum(SMALL) * 7 + 4321 if which == "mixed" else total // 2
        v = float(full[at])
        assert (full == v).sum() >= 1
        conds = [(op, v) for op in (M.GT, M.GE, M.EQ, M.NE)]
    else:
        conds = [(M.GT, -inf), (M.GT, inf)]
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    for op, limit in conds:
        got = _host(ctx, recs, wins, op, limit)
        want = _check(full, wins, got, op, limit, 2 ** 62, which)
        n_sel = int(want[0][-1])
        assert _equal(_dev(A, ctx, torch, recs, wins, op, limit, n_sel, dp, body), got), (op, limit)
        runs = ctx.runs_windows_host(recs, b, c, op, limit)
        off, ent = got
        inside = np.diff(off)
        assert np.array_equal(inside, runs["inside"])
        some = inside > 0
        assert np.array_equal(ent["at"][off[:-1][some].astype(np.int64)], runs["first_at"][some])
        assert np.array_equal(ent["at"][(off[1:][some] - 1).astype(np.int64)], runs["last_at"][some])
        if limit == -inf:  # every sample of a NaN-free stream: a window's entries are its decoded samples
            assert np.array_equal(inside, np.array(c, dtype=np.uint64)) and n_sel == sum(c)
            for i, (wb, wc) in enumerate(wins):
                e = ent[int(off[i]):int(off[i + 1])]
                assert np.array_equal(_bits(e["value"]), _bits(full[wb:wb + wc])), (wb, wc)
                assert np.array_equal(e["at"], np.arange(wc, dtype=np.uint64)), (wb, wc)
        if limit == inf:
            assert n_sel == 0 and len(ent) == 0
    dp.close()


def _placed():
    """17 x 4096 samples of 0 / 1 (and a few special values) with hits at the places the kernels can go wrong"""
    n = 17 * 4096
    x = np.zeros(n)
    for k in range(3):  # around the seams of a load step (63/64, 127/128) and of a task (2047/2048), from even and odd begins
        for s in (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 2046, 2047):
            x[k * TASK + s] = 1
    x[3 * TASK:4 * TASK] = 1          # a task where every sample hits
    #   4 TASK .. 5 TASK                one where none does
    x[5 * TASK:6 * TASK:2] = 1        # alternating
    x[6 * TASK + 1:7 * TASK:2] = 1    # alternating, the other lanes' halves
    x[7 * TASK + 10:7 * TASK + 21] = 1
    x[7 * TASK + 15] = nan            # a NaN next to hits
    x[8 * TASK:8 * TASK + 5] = [-0.0, 0.0, -0.0, 1.0, -0.0]
    x[9 * TASK:9 * TASK + 6] = [inf, 1.0, -inf, inf, inf, 0.0]
    x[PIECE - 5:PIECE + 6] = 1        # on both sides of sample 65536, a piece boundary under the least budget
    x[n - 48:] = 1                    # reaches the stream's end
    return x


@pytest.fixture(scope="module")
def placed(ctx):
    x = _placed()
    recs = b"".join(_idw_record(x[k:k + 4096].tolist()) for k in range(0, len(x), 4096))
    full = ctx.decompress_host(recs)
    assert np.array_equal(np.isnan(full), np.isnan(x)) and np.array_equal(_bits(full[~np.isnan(x)]), _bits(x[~np.isnan(x)]))
    return recs, full


def test_placed_patterns(A, ctx, torch, placed):
    recs, full = placed
    n = len(full)
    T = TASK
    rng = np.random.default_rng(53)
    wins = _seam_windows(n)
    # windows from even and odd begins whose tasks begin or end on a hit, and whose load steps cut between two hits
    wins += [(0, 3 * T), (1, 3 * T), (63, 2 * T), (64, 2 * T), (62, T + 3), (65, 2 * T - 2), (127, 2), (128, T), (129, T),
             (2047, 2), (2047, T + 2), (2046, T), (1, T), (0, T), (3 * T, T), (3 * T - 1, T + 2), (3 * T + 1, T - 1),
             (3 * T + 1, T), (4 * T, T), (4 * T + 1, T - 2), (5 * T, T), (5 * T + 1, T), (5 * T, 2 * T), (5 * T + 1, 2 * T - 1),
             (6 * T, 127), (6 * T + 1, 128), (7 * T, 100), (7 * T + 10, 11), (7 * T + 15, 1), (7 * T + 14, 3),
             (8 * T, 5), (8 * T + 1, 4), (8 * T, 3), (9 * T, 6), (9 * T + 1, 5), (9 * T, 1), (9 * T + 2, 3),
             (PIECE - 5, 11), (PIECE - 6, 13), (PIECE - 1, 2), (PIECE, 6), (n - 48, 48), (n - 100, 100), (n - 1, 1), (0, n),
             (3, n - 3), (2 * T + 5, 6 * T)]
    wins += [(int(b), int(rng.integers(0, 9000))) for b in rng.integers(0, n - 9000, 40)]
    conds = [(M.EQ, 1.0), (M.NE, 1.0), (M.GT, 0.0), (M.GE, 0.0), (M.EQ, 0.0), (M.NE, 0.0), (M.GT, 0.5), (M.GT, inf),
             (M.GE, inf), (M.LT, inf), (M.LE, -inf), (M.GT, -inf), (M.EQ, -inf), (M.LT, 0.5)]
    dp = A.DPlan(ctx, recs)
    r = {}
    for op, limit in conds:
        got = _host(ctx, recs, wins, op, limit)
        want = _check(full, wins, got, op, limit, 2 ** 62, "placed")
        assert _equal(_dev(A, ctx, torch, recs, wins, op, limit, int(want[0][-1]), dp), got), (op, limit)
        r[(op, limit)] = {w: got[1][int(got[0][i]):int(got[0][i + 1])] for i, w in enumerate(wins)}
    dp.close()

    def at(cond, w):
        return r[cond][w]["at"].tolist()

    e = (M.EQ, 1.0)
    assert at(e, (3 * T, T)) == list(range(T)) and at(e, (4 * T, T)) == [] and at(e, (5 * T, T)) == list(range(0, T, 2))
    assert at(e, (5 * T + 1, T)) == list(range(1, T - 1, 2)) and at(e, (5 * T + 1, 2 * T - 1))[-2:] == [2 * T - 4, 2 * T - 2]
    assert at(e, (63, 2 * T))[:6] == [0, 1, 2, 63, 64, 65]            # the task's first sample, and the 126/127/128 seam
    assert at(e, (2047, T + 2)) == [0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 130, 2047, 2048, 2049]  # ... and its last
    assert at(e, (127, 2)) == [0, 1] and at(e, (2047, 2)) == [0, 1] and at(e, (62, T + 3))[-4:] == [1987, 2048, 2049, 2050]
    assert at(e, (7 * T + 10, 11)) == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]  # the NaN is left out
    assert at((M.NE, 1.0), (7 * T + 14, 3)) == [] and at((M.NE, 0.0), (7 * T + 14, 3)) == [0, 2]  # 1 NaN 1
    z = (8 * T, 5)  # -0.0 +0.0 -0.0 1.0 -0.0 against 0.0: the zeros are equal to it whatever their sign, and keep it
    assert at((M.EQ, 0.0), z) == [0, 1, 2, 4]
    assert _bits(r[(M.EQ, 0.0)][z]["value"]).tolist() == [1 << 63, 0, 1 << 63, 1 << 63]
    assert at((M.NE, 0.0), z) == [3] and at((M.GE, 0.0), z) == [0, 1, 2, 3, 4] and at((M.GT, 0.0), z) == [3]
    w = (9 * T, 6)  # Inf 1 -Inf Inf Inf 0
    assert at((M.GT, 0.5), w) == [0, 1, 3, 4] and at((M.GT, inf), w) == [] and at((M.GE, inf), w) == [0, 3, 4]
    assert at((M.LT, inf), w) == [1, 2, 5] and at((M.LE, -inf), w) == [2] and at((M.EQ, -inf), w) == [2]
    assert at((M.GT, -inf), w) == [0, 1, 3, 4, 5]
    assert r[(M.GE, inf)][w]["value"].tolist() == [inf, inf, inf] and r[(M.LE, -inf)][w]["value"].tolist() == [-inf]
    assert at(e, (PIECE - 6, 13)) == list(range(1, 12)) and at(e, (n - 100, 100)) == list(range(52, 100))


def test_truncation(A, ctx, torch, decoded):
    """one call's windows under caps from 0 to past the total: the offsets never change, the entries below cap never do,
    and the words behind ATSC_SELECT_BYTES(n, cap) stay untouched (_dev's guard)"""
    recs, full = decoded["mixed"]
    total = len(full)
    rng = np.random.default_rng(71)
    wins = [(int(b), int(rng.integers(0, 6000))) for b in rng.integers(0, total - 6000, 30)] + [(5, 0), (1000, 5000)]
    op, limit = M.GT, float(np.quantile(full, 0.9))
    whole = _host(ctx, recs, wins, op, limit)
    off, ent = _check(full, wins, whole, op, limit, 2 ** 62, "whole")
    n_sel = int(off[-1])
    i = int(np.flatnonzero(np.diff(off) >= 3)[1])  # a window with three entries or more, with entries before and behind
    assert 0 < int(off[i + 1]) < n_sel
    caps = [0, 1, int(off[i]) + 1, int(off[i + 1]), n_sel - 1, n_sel, n_sel + 5]
    assert len(set(caps)) == 7 and n_sel > 100
    dp = A.DPlan(ctx, recs)
    for cap in caps:
        for got in (_dev(A, ctx, torch, recs, wins, op, limit, cap, dp), _host(ctx, recs, wins, op, limit, cap)):
            assert np.array_equal(got[0], off), cap
            assert _equal(got, (off, ent[:cap])), cap
    dp.close()


@pytest.mark.parametrize("which", ["mixed", "large", "placed", "gaps"])
def test_pieces(A, ctx, torch, decoded, placed, gaps, which):
    """the least budget: pieces of 65536 samples, counted from the first covered sample (0: the whole stream is one of
    the windows, but for "gaps", where they are counted from the first sample of every run of windows).  The write step
    decodes every piece again; the default budget's result bit for bit, by the host call and repeatedly on one plan"""
    recs, full = placed if which == "placed" else gaps if which == "gaps" else decoded[which]
    total = len(full)
    rng = np.random.default_rng(31)
    wins = [(0, total), (PIECE, 1), (PIECE, 2), (PIECE - 10, 10), (0, PIECE), (PIECE - 1, 2), (PIECE - 1, 1), (PIECE - 2, 2),
            (PIECE - 6, 13), (5, 0), (PIECE - TASK - 1, 2 * TASK + 2), (PIECE + 1, 5)]
    if total > 3 * PIECE:
        wins += [(1000, 200000), (PIECE, 70000), (PIECE - 1, PIECE + 2), (2 * PIECE - 1, 2), (2 * PIECE - TASK, 2 * TASK),
                 (3 * PIECE - 1, 3)]
        wins += [(int(b), int(rng.integers(0, 150000))) for b in rng.integers(0, total - 150000, 6)]
    wins += [(int(b), 60) for b in rng.integers(PIECE - 100, PIECE + 100, 10)]
    if which == "gaps":
        wins = GAP_WINS
    conds = [(M.EQ, 1.0), (M.GT, -inf)] if which == "placed" else [(M.GT, float(np.median(full))), (M.GT, -inf)]
    for op, limit in conds:
        alone = _host(ctx, recs, wins, op, limit)
        _check(full, wins, alone, op, limit, 2 ** 62, which)
        n_sel = int(alone[0][-1])
        dp = A.DPlan(ctx, recs)
        try:
            for budget in (1, 1 << 20):  # 65536 and 131072 samples a piece
                ctx.set_aggregate_scratch(budget)
                assert _equal(_host(ctx, recs, wins, op, limit), alone), budget
                assert _equal(_dev(A, ctx, torch, recs, wins, op, limit, n_sel, dp), alone), budget
                one = _dev(A, ctx, torch, recs, wins[:1], op, limit, n_sel, dp)  # the tables reused
                _check(full, wins[:1], one, op, limit, n_sel, which)
                cut = _dev(A, ctx, torch, recs, wins, op, limit, n_sel // 2, dp)
                assert _equal(cut, (alone[0], alone[1][: n_sel // 2])), budget
        finally:
            ctx.set_aggregate_scratch(0)
        assert _equal(_dev(A, ctx, torch, recs, wins, op, limit, n_sel, dp), alone)
        dp.close()
        if which == "placed" and op == M.EQ:  # the hits on both sides of the piece boundary, in order
            k = wins.index((PIECE - 6, 13))
            assert alone[1]["at"][int(alone[0][k]):int(alone[0][k + 1])].tolist() == list(range(1, 12))


def test_many_tasks(A, ctx, torch, decoded):
    """20000 short windows at random places and in random order: about 19500 tasks, one per non-empty window.  The scan
    takes SEL_SCAN_BLOCK = 2048 counts per workgroup, so this is ten blocks and a second level over their sums.  The same
    windows permuted give every window the same entries"""
    recs, full = decoded["mixed"]
    total = len(full)
    rng = np.random.default_rng(83)
    wins = [(int(b), int(c)) for b, c in zip(rng.integers(0, total - 40, 20000), rng.integers(0, 41, 20000))]
    assert sum(1 for _, c in wins if c) > 4 * 2048
    op, limit = M.GT, float(np.median(full))
    got = _host(ctx, recs, wins, op, limit)
    want = _check(full, wins, got, op, limit, 2 ** 62, "many")
    n_sel = int(want[0][-1])
    dp = A.DPlan(ctx, recs)
    assert _equal(_dev(A, ctx, torch, recs, wins, op, limit, n_sel, dp), got)
    perm = rng.permutation(len(wins))
    wins2 = [wins[k] for k in perm]
    got2 = _dev(A, ctx, torch, recs, wins2, op, limit, n_sel, dp)
    dp.close()
    _check(full, wins2, got2, op, limit, n_sel, "permuted")
    for j in (0, 1, 77, 9999, 19999):  # (the model has checked every window; spelled out for a few)
        k = int(perm[j])
        a = got[1][int(got[0][k]):int(got[0][k + 1])]
        b = got2[1][int(got2[0][j]):int(got2[0][j + 1])]
        assert np.array_equal(a, b)


def test_three_scan_levels(A, ctx, torch, decoded):
    """2048 * 2048 + 4097 one-sample windows: more counts than two levels of the scan hold, so a third level runs.  The
    expected block is read off the full decode directly: a window's entry is its sample at offset 0"""
    recs, full = decoded["mixed"]
    rng = np.random.default_rng(89)
    n = 2048 * 2048 + 4097
    b = rng.integers(0, len(full), n).astype(np.uint64)
    c = np.ones(n, dtype=np.uint64)
    c[::1000] = 0
    limit = float(np.quantile(full, 0.99))
    hit = (full[b.astype(np.int64)] > limit) & (c > 0)
    off = np.concatenate([[0], np.cumsum(hit)]).astype(np.uint64)
    n_sel = int(off[-1])
    assert 10000 < n_sel < n // 50
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    words = A.select_bytes(n, n_sel) // 8
    d = torch.full((words + 8,), SENT, dtype=torch.int64, device="cuda")
    dp.select_windows(body, b, c, M.GT, limit, n_sel, d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    dp.close()
    assert (h[words:] == SENT).all()
    assert np.array_equal(h[: n + 1].view(np.uint64), off)
    ent = h[n + 1: words].view(A.SELECTED)
    assert np.array_equal(_bits(ent["value"]), _bits(full[b[hit].astype(np.int64)])) and not ent["at"].any()


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
    _check(good, outside, _host(ctx, bad, outside, M.GT, lim), M.GT, lim, 2 ** 62, "outside")  # the damage is not seen
    lib = A.capi.lib()
    bb = np.frombuffer(bad, dtype=np.uint8)
    gb = np.frombuffer(recs, dtype=np.uint8)
    p = C.POINTER(C.c_uint64)
    CAP = 64

    def raw(buf, wins, op=M.GT, limit=lim, cap=CAP):
        out = np.full(A.select_bytes(len(wins), CAP) // 8, 7, dtype=np.uint64)
        b = np.array([w[0] for w in wins], dtype=np.uint64)
        c = np.array([w[1] for w in wins], dtype=np.uint64)
        rc = lib.atsc_select_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(wins),
                                     b.ctypes.data_as(p), c.ctypes.data_as(p), op, limit, cap, C.c_void_p(out.ctypes.data))
        return rc, out

    for wins in ([(3 * n, 1)], [(0, nf * n)], [(0, 10), (3 * n - 1, 2)], [(4 * n - 1, 1), (6 * n, 5)]):
        for cap in (CAP, 0):
            rc, out = raw(bb, wins, cap=cap)
            assert rc == A.capi.E_FORMAT and np.all(out == 7), (wins, rc)
    for wins in ([(nf * n - 2, 4)], [(0, 5), (nf * n + 1, 0)], [(2 ** 63, 2 ** 63)]):
        rc, out = raw(gb, wins)
        assert rc == A.capi.E_INVALID and np.all(out == 7), (wins, rc)
    for op, limit in ((6, lim), (-1, lim), (M.GT, nan), (M.NE, -nan), (99, nan)):
        for wins in ([(0, 5)], [(0, 0)], []):
            rc, out = raw(gb, wins, op, limit)
            assert rc == A.capi.E_INVALID and np.all(out == 7), (op, limit, wins)
    rc, out = raw(gb, [])
    assert rc == 0 and np.all(out == 7)  # n_windows == 0 writes nothing
    rc, out = raw(gb, [(5, 0), (nf * n, 0), (0, 0)])
    assert rc == 0 and out[:4].tolist() == [0, 0, 0, 0] and np.all(out[4:] == 7)  # only empty windows: the offsets
    rc, out = raw(gb, [(0, 40), (7, 0), (40, 40)], cap=3)  # a small cap is no error: a correct prefix
    want = M.windows_select(good, [(0, 40), (7, 0), (40, 40)], M.GT, lim, 3)
    assert rc == 0 and np.array_equal(out[:4], want[0]) and int(want[0][-1]) > 3
    assert _equal((want[0], out[4:10].view(A.SELECTED)), want)
    off, ent = _host(ctx, recs, [], M.GT, lim)
    assert off.tolist() == [0] and len(ent) == 0
    with pytest.raises(A.AtscError):
        _host(ctx, recs, [(0, 5)], 6, lim)
    # the device call: a bad condition, a window beyond the plan, a misaligned result, a null argument -- nothing enqueued
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(gb.copy()).to("cuda")
    d_out = torch.full((64,), -1, dtype=torch.int64, device="cuda")
    one = np.array([0], dtype=np.uint64)
    cnt = np.array([nf * n + 1], dtype=np.uint64)

    def dev(h_dp, d_body, nw, b, c, ptr, op=M.GT, limit=lim, cap=16):
        return lib.atsc_select_windows_dev(ctx._h, h_dp, C.c_void_p(d_body), nw, b.ctypes.data_as(p), c.ctypes.data_as(p),
                                           op, limit, cap, C.c_void_p(ptr), None)

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
    for op, limit in ((M.LE, inf), (M.GE, -inf)):  # an infinite limit is valid; an entries' base that is 8-byte aligned only
        assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr() + 8, op, limit) == 0
        torch.cuda.synchronize()
        h = d_out.cpu().numpy()
        assert h[0] == -1 and h[1:3].tolist() == [0, 10] and (h[35:] == -1).all()  # the block: words 1 .. 34
        e = h[3:23].view(A.SELECTED)
        assert np.array_equal(_bits(e["value"]), _bits(good[:10])) and e["at"].tolist() == list(range(10))
    dp.close()


def test_one_plan(A, ctx, torch, decoded):
    """two select calls with different conditions back to back on one plan, without waiting in between, and select
    interleaved with runs and aggregate calls: every result is that of a plan of its own"""
    recs, full = decoded["mixed"]
    total = len(full)
    rng = np.random.default_rng(59)
    wa = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, total - 100000, 30)] + [(0, total)]
    ws = [(int(b), int(rng.integers(0, 20000))) for b in rng.integers(0, total - 20000, 40)] + [(7, 30000)]
    lo, hi = float(np.quantile(full, 0.05)), float(np.quantile(full, 0.95))
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    s = torch.cuda.current_stream().cuda_stream
    want_hi = M.windows_select(full, ws, M.GT, hi, 2 ** 62)
    want_lo = M.windows_select(full, ws, M.LE, lo, 2 ** 62)
    cap_hi, cap_lo = int(want_hi[0][-1]), int(want_lo[0][-1])

    def call(method, words, wins, *mid):
        d = torch.full((words,), -1, dtype=torch.int64, device="cuda")
        method(body, [w[0] for w in wins], [w[1] for w in wins], *mid, d, s)
        return d

    def alone(name, words, wins, *mid):
        dp = A.DPlan(ctx, recs)
        d = call(getattr(dp, name), words, wins, *mid)
        torch.cuda.synchronize()
        out = d.cpu().numpy().tobytes()
        dp.close()
        return out

    a_alone = alone("aggregate_windows", 6 * len(wa), wa)
    r_alone = alone("runs_windows", 10 * len(wa), wa, M.GT, hi)

    def block(d, cap):
        h = d.cpu().numpy()
        n = len(ws)
        off = h[: n + 1].view(np.uint64)
        return off, h[n + 1: n + 1 + 2 * min(int(off[n]), cap)].view(A.SELECTED)

    dp = A.DPlan(ctx, recs)
    outs = []
    for _ in range(3):
        outs.append((call(dp.select_windows, A.select_bytes(len(ws), cap_hi) // 8, ws, M.GT, hi, cap_hi),
                     call(dp.select_windows, A.select_bytes(len(ws), cap_lo) // 8, ws, M.LE, lo, cap_lo),
                     call(dp.aggregate_windows, 6 * len(wa), wa),
                     call(dp.select_windows, A.select_bytes(len(ws), 5) // 8, ws, M.GT, hi, 5),
                     call(dp.runs_windows, 10 * len(wa), wa, M.GT, hi),
                     call(dp.select_windows, A.select_bytes(len(ws), cap_lo) // 8, ws, M.LE, lo, cap_lo)))
    torch.cuda.synchronize()
    for s_hi, s_lo, a, s_cut, r, s_lo2 in outs:
        assert _equal(block(s_hi, cap_hi), want_hi) and _equal(block(s_lo, cap_lo), want_lo)
        assert _equal(block(s_lo2, cap_lo), want_lo)
        assert _equal(block(s_cut, 5), (want_hi[0], want_hi[1][:5]))
        assert a.cpu().numpy().tobytes() == a_alone and r.cpu().numpy().tobytes() == r_alone
    dp.close()
    assert cap_hi > 1000 and cap_lo > 1000


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
                via_bro = A.select_data_windows(ctx, bro, b, c, op, limit)
                want = _check(full, wins, via_bro, op, limit, 2 ** 62, name)
                n_sel = int(want[0][-1])
                records = bro[9:]  # with the frame-count varint
                assert _equal(ctx.select_windows_host(records, b, c, op, limit, has_count=True), via_bro), (name, comp)
                s = A.CompressedStream.from_bytes(ctx, bro)
                assert _equal(s.select_windows(b, c, op, limit), via_bro), (name, comp)
                assert _equal(s.select_windows(b, c, op, limit, cap=3), (want[0], want[1][:3])), (name, comp)
                assert _equal(A.select_data_windows(ctx, bro, b, c, op, limit, cap=n_sel + 9), via_bro), (name, comp)
                n0, p0 = H.varint_decode(bro, 9)
                assert n0 == len(frames)
                assert _equal(_dev(A, ctx, torch, bro[p0:], wins, op, limit, n_sel), via_bro), (name, comp)
    s = A.CompressedStream(ctx)  # a stream without a frame holds only empty windows at 0
    off, ent = s.select_windows([0, 0], [0, 0], M.GT, 1.0)
    assert off.tolist() == [0, 0, 0] and len(ent) == 0
    with pytest.raises(A.AtscError):
        s.select_windows([0], [1], M.GT, 1.0)
    with pytest.raises(A.AtscError):
        s.select_windows([0], [0], 6, 1.0)
    with pytest.raises(A.AtscError):
        s.select_windows([0], [0], M.GT, nan)


def _sel_rows(path, first):
    lines = open(path).read().split("\n")
    assert lines[0] == first + ",value" and lines[-1] == ""
    return [(int(l.split(",")[0]), int(_bits(float(l.split(",")[1]))[0])) for l in lines[1:-1]]


def test_command_lines(A, ctx, golden_dir, tmp_path):
    from oracle import vsri_oracle as VO

    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    src = tmp_path / "heap.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "go_gc_heap_goal_bytes.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    src.unlink()
    bro = (tmp_path / "heap.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    med = float(np.median(full))
    seen = 0
    for (b0, c0), flag, op, lim in (((0, len(full)), "gt:%r" % med, M.GT, med), ((100, 1500), "le:%r" % med, M.LE, med),
                                    ((37, 900), "ne:%r" % float(full[40]), M.NE, float(full[40])),
                                    ((5, 0), "gt:0", M.GT, 0.0), ((10, 50), "gt:inf", M.GT, inf)):
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--where", flag, tmp_path / "heap.bro")
        assert sorted(p.name for p in tmp_path.glob("heap*")) == ["heap.bro", "heap.sel.csv"]  # no .wbro
        _, ent = M.windows_select(full, [(b0, c0)], op, lim, c0)
        want = [(b0 + int(a), int(v)) for a, v in zip(ent["at"], _bits(ent["value"]))]
        assert _sel_rows(tmp_path / "heap.sel.csv", "sample") == want, (b0, c0, flag)
        seen += len(want)
        (tmp_path / "heap.sel.csv").unlink()
    assert seen > 500
    # csv-compressor -u --from --to --where on the reference's cpu_utilization values and times
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
    times = np.array([int(r.split(",")[0]) for r in all_rows])  # the index's time of every sample
    index = A.Vsri.load(str(tmp_path / "cpu.vsri"))
    lim = float(np.median(all_vals))
    for t0, t1, flag, op in ((times[0], times[-1], "le:%r" % lim, M.LE), (times[10] + 1, times[50] - 1, "gt:%r" % lim, M.GT),
                             (times[-1] + 1, times[-1] + 5, "gt:0", M.GT)):
        for f in tmp_path.glob("win*"):
            f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--where", flag, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.sel.csv"]
        b0, c0 = index.sample_window(int(t0), int(t1))
        _, ent = M.windows_select(all_vals, [(b0, c0)], op, lim if flag != "gt:0" else 0.0, c0)
        want = [(int(times[b0 + int(a)]), int(v)) for a, v in zip(ent["at"], _bits(ent["value"]))]
        assert _sel_rows(tmp_path / "win.sel.csv", "timestamp") == want, (t0, t1, flag)
        assert all(int(index.get_time(b0 + int(a))) == int(times[b0 + int(a)]) for a in ent["at"][:20])
        assert len(want) > 5 or c0 == 0
