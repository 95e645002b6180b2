"""Windowed pair matrix on the GPU: every record against atsc_pair_windows_dev of its two streams and against the NumPy
model (tests/pair_matrix_model.py: the pair moments' model per pair) on the GPU's own full decodes -- all six fields bit
for bit, any NaN equal to any NaN, no tolerance.  Lists of 1, 2, 3 and 7 streams of different framings, codecs and
tiers (131072-sample frames in one stream only); windows inside a tile, across tile and frame boundaries, of lengths 0, 1
and 2, overlapping, unsorted; 64 and 66 tiles in one window and shared mid tiles; NaN and Inf; 64 streams; budgets that
cut a window into pieces; a stream listed twice and a permuted list; plans reused and shared with other queries; every
validation case with the result untouched; a malformed payload; the device, host, stream and Python surfaces and the
command line."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import pair_matrix_model as PM

pytestmark = pytest.mark.gpu

T = PM.TILE
N = 131072 + 40000  # samples of the main streams
SENT = -1  # every result is prefilled with it


@pytest.fixture(scope="module")
def A():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a MI355X"  # (torch's runtime first, as the other GPU suites)
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


@pytest.fixture(scope="module")
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def _v(x):
    if x < 251:
        return bytes([x])
    if x < 1 << 16:
        return b"\xfb" + struct.pack("<H", x)
    return b"\xfc" + struct.pack("<I", x)


def _rec(n, tag, payload):
    return _v(41) + _v(n) + _v(tag) + _v(len(payload)) + payload


def _idw_stream(x, frame):
    """hand-built IDW records whose points are the samples themselves (f64 points, point step 1, min -Inf, max +Inf):
    every sample decodes to its point, NaN and +-Inf included"""
    out = []
    for k in range(0, len(x), frame):
        v = np.ascontiguousarray(x[k:k + frame], dtype="<f8")
        out.append(_rec(len(v), 2, _v(1) + _v(0) + _v(len(v)) + v.tobytes() + struct.pack("<dd", -np.inf, np.inf) + bytes([1])))
    return b"".join(out)


def _exact(ctx, recs, x):
    """the decode of a hand-built stream is its samples"""
    f = ctx.decompress_host(recs)
    assert np.array_equal(np.isnan(f), np.isnan(x)) and np.array_equal(f[~np.isnan(x)], x[~np.isnan(x)])
    return f


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _equal(got, want):
    """the count and the five doubles bit for bit; any NaN equals any NaN"""
    if got.shape != want.shape or not np.array_equal(got["count"], want["count"]):
        return False
    for k in PM.FIELDS[1:]:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if not np.all((_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))):
            return False
    return True


class _Plans:
    """the decode plans and device bytes of a list of record streams, made once"""

    def __init__(self, A, ctx, torch, recs):
        self.A, self.torch = A, torch
        self.dp = [A.DPlan(ctx, r) for r in recs]
        self.body = [torch.from_numpy(np.frombuffer(r, dtype=np.uint8).copy()).to("cuda") for r in recs]
        self.stream = torch.cuda.current_stream().cuda_stream

    def close(self):
        for d in self.dp:
            d.close()

    def matrix(self, wins, order=None):
        """the device call over the streams `order` (default: all of them) -> (W, P) records"""
        order = list(range(len(self.dp))) if order is None else order
        p = PM.records(len(order))
        d_out = self.torch.full((max(len(wins) * p, 1) * 6,), SENT, dtype=self.torch.int64, device="cuda")
        view = self.dp[order[0]].pair_matrix_windows(self.body[order[0]], [self.dp[k] for k in order[1:]],
                                                     [self.body[k] for k in order[1:]], [w[0] for w in wins],
                                                     [w[1] for w in wins], d_out, self.stream)
        self.torch.cuda.synchronize()
        assert tuple(view.shape) == (len(wins), p, 48)
        return d_out.cpu().numpy().view(self.A.WINDOW_PAIR)[: len(wins) * p].reshape(len(wins), p).copy()

    def pairs(self, wins, order=None, only=None):
        """atsc_pair_windows_dev of every pair (only: of those) of the streams `order` -> (W, P) records"""
        order = list(range(len(self.dp))) if order is None else order
        n, w = len(order), len(wins)
        d_out = self.torch.full((PM.records(n), max(w, 1) * 6), SENT, dtype=self.torch.int64, device="cuda")
        b, c = [x[0] for x in wins], [x[1] for x in wins]
        todo = PM.pairs(n) if only is None else only
        for i, j in todo:
            self.dp[order[i]].pair_windows(self.body[order[i]], self.dp[order[j]], self.body[order[j]], b, c,
                                           d_out[PM.index(n, i, j)], self.stream)
        self.torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(self.A.WINDOW_PAIR)[:, :w]
        return np.ascontiguousarray(out.T)


def _check_pairs(pl, wins, got, order=None, label=""):
    want = pl.pairs(wins, order)
    n = len(pl.dp) if order is None else len(order)
    for i, j in PM.pairs(n):
        p = PM.index(n, i, j)
        assert _equal(got[:, p], want[:, p]), (label, i, j, got[:, p], want[:, p])


def _check_model(fulls, wins, got, only=None, label=""):
    n = len(fulls)
    want = PM.windows_pair_matrix(fulls, wins, only)
    for i, j in (PM.pairs(n) if only is None else only):
        p = PM.index(n, i, j)
        for w in range(len(wins)):
            assert _equal(got[w:w + 1, p], want[w:w + 1, p]), (label, i, j, wins[w], got[w, p], want[w, p])


def _tile_tasks(wins):
    """the tile tasks of a call: the shared full tiles, merged over the windows, and every window's first and last tile"""
    mids, ends = set(), 0
    for b, c in wins:
        if not c:
            continue
        kb, ke = b // T, (b + c - 1) // T
        ends += 1 if ke == kb else 2
        mids.update(range(kb + 1, ke))
    return len(mids) + ends


WINS = [(0, N), (0, 0), (N, 0), (N - 1, 1), (0, 1), (0, 2), (N - 2, 2), (77, 0), (131071, 1), (131072, 1), (131071, 2),
        (131067, 11), (80000 - 1, 2), (80000 - 5, 11), (4096 - 1, 2), (4096, 1), (3000, 1000), (5 * T, T), (5 * T, 2 * T),
        (9 * T, 5 * T), (7 * T - 1, 2), (7 * T + 1, T - 2), (11 * T + T - 1, T + 2), (20 * T + 100, 1500), (20 * T + 7, 2),
        (30 * T, 1), (30 * T + T - 2, 2), (10 * T + 5, 60000), (131072 - 3 * T - 9, 7 * T), (100000, N - 100000), (12345, 0), (40 * T + 3, 5)]


@pytest.fixture(scope="module")
def streams(A, ctx):
    """seven streams of N samples.  X: 4096-sample frames under auto; Y: frames of 1000 (polynomial) and 3000 (idw); YL: a
    131072-sample frame and one of 40000 (fft: the large tier's launch sequence and spill slots in this region only); S3
    .. S6: hand-built records of 700, 2048, 5000 and 1234 samples with NaN at different slots of each.
    -> list of (records, full decode)"""
    e = float(np.float32(0.03))
    x = ctx.compress_host(H.synth_series(3100, N, block=20000), H.frame_offsets(N, 4096), A.AUTO, True, e, 0)[0]
    h = 80000
    y = ctx.compress_host(H.synth_series(3101, h, klass=2), H.frame_offsets(h, 1000), A.POLYNOMIAL, True, e, 0)[0]
    y += ctx.compress_host(H.synth_series(3102, N - h, klass=0), H.frame_offsets(N - h, 3000), A.IDW, True, e, 0)[0]
    yl = ctx.compress_host(H.synth_series(3103, N, klass=1), np.array([0, 131072, N], dtype=np.uint64), A.FFT, True,
                           float(np.float32(0.01)), 0)[0]
    out = [(r, ctx.decompress_host(r)) for r in (x, y, yl)]
    rng = np.random.default_rng(3104)
    for k, frame in enumerate((700, 2048, 5000, 1234)):
        v = np.round(rng.normal(k, 10.0 ** k, N), 5)
        v[rng.random(N) < 0.01 * (k + 1)] = np.nan
        v[(5 + k) * T + 128 * k:(5 + k) * T + 128 * k + 128] = np.nan  # an aligned stretch of 128 slots, elsewhere in each
        r = _idw_stream(v, frame)
        out.append((r, _exact(ctx, r, v)))
    assert all(len(f) == N for _, f in out)
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_parity_with_pairs_and_full_decodes(A, ctx, torch, streams, n):
    rng = np.random.default_rng(3110 + n)
    wins = [WINS[i] for i in rng.permutation(len(WINS))]
    assert _tile_tasks(wins) % 4 != 0  # the last workgroup of the tile launch is not full
    pl = _Plans(A, ctx, torch, [r for r, _ in streams[:n]])
    try:
        got = pl.matrix(wins)
        assert got.shape == (len(wins), PM.records(n))
        _check_pairs(pl, wins, got, label="n = %d" % n)
        _check_model([f for _, f in streams[:n]], wins, got, label="n = %d" % n)
        for w, (b, c) in enumerate(wins):
            if c == 0:
                assert np.all(got[w]["count"] == 0) and all(np.all(np.isnan(got[w][k])) for k in PM.FIELDS[1:])
    finally:
        pl.close()


@pytest.fixture(scope="module")
def long3(ctx):
    """three hand-built streams of 72 tiles whose merges depend on their order, with NaN holes"""
    n = 72 * T
    rng = np.random.default_rng(3120)
    x = np.round(rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 7, n), 5)
    y = np.round(0.5 * x + rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 5, n), 5)
    z = np.round(rng.normal(1e9, 1e-3, n), 5)
    for v in (x, y, z):
        v[rng.integers(0, n, 300)] = np.nan
    recs = [_idw_stream(x, 4096), _idw_stream(y, 2560), _idw_stream(z, 3000)]
    return recs, [_exact(ctx, r, v) for r, v in zip(recs, (x, y, z))]


LONG_WINS = [(2 * T + 1, 64 * T), (T + 7, 66 * T), (2 * T, 64 * T), (T, 66 * T), (2 * T - 1, 64 * T + 2), (5, 65 * T),
             (0, 72 * T), (3 * T + 9, 20 * T), (10 * T, 30 * T)]


def test_64_and_66_tiles_and_shared_mid_tiles(A, ctx, torch, long3):
    """64 partials fill one combine group exactly, 66 need a second pass; the overlapping windows share their mid tiles'
    partials"""
    recs, fulls = long3
    pl = _Plans(A, ctx, torch, recs)
    try:
        got = pl.matrix(LONG_WINS)
        _check_pairs(pl, LONG_WINS, got, label="long")
        _check_model(fulls, LONG_WINS, got, label="long")
    finally:
        pl.close()


def test_nan_and_inf(A, ctx, torch):
    """NaN at different slots per stream, stream 2 all NaN inside one window, +-Inf: the pairs with stream 2 count nothing
    there, the other pairs are what they are without it; tile 3 has no NaN in any stream (the equal-count path) and the
    others have some (the general path)"""
    nan, inf = float("nan"), float("inf")
    n = 5 * T
    rng = np.random.default_rng(3130)
    s = [np.round(rng.normal(k, 3.0 + k, n), 5) for k in range(5)]
    for k in range(5):
        hole = rng.random(n) < 0.02 * (k + 1)
        hole[3 * T:4 * T] = False
        s[k][hole] = nan
    s[2][T:2 * T] = nan  # a whole tile
    s[0][2 * T + 256:2 * T + 384] = nan  # aligned stretches of 128 slots
    s[4][2 * T + 1280:2 * T + 1408] = nan
    s[3][4 * T + 5] = inf
    s[4][4 * T + 9] = -inf
    s[3][4 * T + 300] = -inf
    s[4][4 * T + 300] = inf
    recs = [_idw_stream(v, f) for v, f in zip(s, (4096, 1000, 2048, 3000, 777))]
    fulls = [_exact(ctx, r, v) for r, v in zip(recs, s)]
    wins = [(0, n), (T, T), (T + 10, 100), (T - 5, T + 10), (3 * T, T), (3 * T + 1, T - 2), (2 * T, T), (2 * T + 256, 128),
            (4 * T, T), (4 * T, 8), (4 * T + 300, 1), (4 * T + 299, 3), (5, 4 * T), (T + 55, 0)]
    pl = _Plans(A, ctx, torch, recs)
    try:
        got = pl.matrix(wins)
        _check_pairs(pl, wins, got, label="nonfinite")
        _check_model(fulls, wins, got, label="nonfinite")
        for w in (1, 2):  # windows inside stream 2's tile of NaN
            for i, j in PM.pairs(5):
                r = got[w, PM.index(5, i, j)]
                if 2 in (i, j):
                    assert int(r["count"]) == 0 and all(np.isnan(r[k]) for k in PM.FIELDS[1:]), (w, i, j)
                else:
                    assert int(r["count"]) > 0 and not np.isnan(r["c_xy"]), (w, i, j)
        # without stream 2 in the list the other pairs' records are the same bits
        four = pl.matrix(wins, order=[0, 1, 3, 4])
        for a, i in enumerate((0, 1, 3, 4)):
            for b, j in list(enumerate((0, 1, 3, 4)))[a:]:
                assert _equal(four[:, PM.index(4, a, b)], got[:, PM.index(5, i, j)]), (i, j)
        assert all(int(got[4, p]["count"]) == T for p in range(PM.records(5)))  # tile 3: every slot of every pair
        assert int(got[7, PM.index(5, 0, 1)]["count"]) == 0 and int(got[7, PM.index(5, 1, 3)]["count"]) > 0
    finally:
        pl.close()


def _many(ctx, n_streams, n, seed):
    """n_streams distinct hand-built streams of n samples in frames of different lengths, a few NaN in every third"""
    rng = np.random.default_rng(seed)
    base = rng.normal(0, 1, n)
    recs, fulls = [], []
    for k in range(n_streams):
        v = np.round((k % 7 - 3) * 0.3 * base + rng.normal(k, 1 + k % 5, n) * 10.0 ** (k % 4), 5)
        if k % 3 == 0:
            v[rng.integers(0, n, 20)] = np.nan
        recs.append(_idw_stream(v, 500 + 37 * k))
        fulls.append(v)
    return recs, fulls


def test_64_streams(A, ctx, torch):
    """all 2080 records of every window against atsc_pair_windows_dev of their pair; 24 pairs against the model"""
    n = 3 * T + 100
    recs, vals = _many(ctx, 64, n, 3140)
    fulls = [_exact(ctx, recs[k], vals[k]) for k in (0, 31, 63)]
    assert len(fulls) == 3
    wins = [(n - 1, 1), (T + 100, 700), (T - 50, 100), (0, n), (17, 0), (2 * T - 1, T + 50)]
    pl = _Plans(A, ctx, torch, recs)
    try:
        got = pl.matrix(wins)
        assert got.shape == (len(wins), 2080)
        _check_pairs(pl, wins, got, label="64")
        rng = np.random.default_rng(3141)
        only = {(0, 0), (0, 63), (63, 63)}
        while len(only) < 24:
            i, j = sorted(int(v) for v in rng.integers(0, 64, 2))
            only.add((i, j))
        _check_model(vals, wins, got, only=sorted(only), label="64, model")
    finally:
        pl.close()


def test_pieces_under_the_least_budget(A, ctx, torch, long3):
    """the least budget gives every region 32 tiles: a 70-tile window of three streams in three pieces, a 40-tile window
    of 64 streams in two -- the default budget's bits"""
    recs3, fulls3 = long3
    wins3 = [(T + 5, 70 * T), (0, 72 * T), (40 * T, 100), (31 * T + 2000, 100)]
    n = 41 * T
    recs64, vals64 = _many(ctx, 64, n, 3150)
    wins64 = [(T // 2, 40 * T), (33 * T, 5)]
    pl3, pl64 = _Plans(A, ctx, torch, recs3), _Plans(A, ctx, torch, recs64)
    try:
        whole3, whole64 = pl3.matrix(wins3), pl64.matrix(wins64)
        _check_model(fulls3, wins3, whole3, label="70 tiles")
        only = [(0, 0), (0, 63), (63, 63), (5, 40), (31, 32)]
        want = pl64.pairs(wins64, only=only)
        for i, j in only:
            assert _equal(whole64[:, PM.index(64, i, j)], want[:, PM.index(64, i, j)]), (i, j)
        try:
            ctx.set_aggregate_scratch(1)
            assert _equal(pl3.matrix(wins3), whole3)
            assert _equal(pl64.matrix(wins64), whole64)
            assert _equal(ctx.pair_matrix_windows_host(recs3, [w[0] for w in wins3], [w[1] for w in wins3]), whole3)
        finally:
            ctx.set_aggregate_scratch(0)
    finally:
        pl3.close()
        pl64.close()


def test_listed_twice_and_permuted(A, ctx, torch, streams):
    wins = [WINS[i] for i in (0, 3, 8, 10, 17, 19, 23, 27, 1)]
    pl = _Plans(A, ctx, torch, [r for r, _ in streams[:4]])
    try:
        base = pl.matrix(wins, order=[0, 1, 2])
        twice = pl.matrix(wins, order=[0, 1, 0])
        _check_pairs(pl, wins, twice, order=[0, 1, 0], label="twice")
        assert _equal(twice[:, PM.index(3, 0, 2)], base[:, PM.index(3, 0, 0)])  # off the diagonal, its own diagonal record
        assert _equal(twice[:, PM.index(3, 2, 2)], base[:, PM.index(3, 0, 0)])
        perm = pl.matrix(wins, order=[2, 0, 3, 1])
        _check_pairs(pl, wins, perm, order=[2, 0, 3, 1], label="permuted")
        assert _equal(perm[:, PM.index(4, 1, 3)], base[:, PM.index(3, 0, 1)])  # (X, Y) wherever they stand
        sw = perm[:, PM.index(4, 0, 1)]  # (YL, X): base's (X, YL) with the fields swapped
        bw = base[:, PM.index(3, 0, 2)]
        for k, kb in zip(("count", "mean_x", "m2_x", "mean_y", "m2_y", "c_xy"), ("count", "mean_y", "m2_y", "mean_x", "m2_x", "c_xy")):
            g, w = np.ascontiguousarray(sw[k]), np.ascontiguousarray(bw[kb])
            assert np.array_equal(g, w) if k == "count" else np.all((_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))), k
    finally:
        pl.close()


def test_plan_reuse_and_other_queries(A, ctx, torch, streams):
    """two calls on one dp[0] with different N, then pair_windows and an across call on the same plans: every result is
    that of fresh plans"""
    recs = [r for r, _ in streams]
    wa = [WINS[i] for i in (0, 9, 18, 20, 28)]
    wb = [WINS[i] for i in (27, 2, 19, 11)]
    fresh = _Plans(A, ctx, torch, recs)
    try:
        want7, want2, want3 = fresh.matrix(wa), fresh.matrix(wb, order=[0, 1]), fresh.matrix(wa, order=[0, 1, 2])
    finally:
        fresh.close()
    pl = _Plans(A, ctx, torch, recs)
    try:
        assert _equal(pl.matrix(wa, order=[0, 1, 2]), want3)
        assert _equal(pl.matrix(wb, order=[0, 1]), want2)
        assert _equal(pl.matrix(wa), want7)
        assert pl.matrix([]).shape == (0, 28)
        assert _equal(pl.matrix(wa, order=[0, 1, 2]), want3)
        pair = pl.pairs(wa, order=[0, 1], only=[(0, 1)])[:, PM.index(2, 0, 1)]
        assert _equal(pair, want3[:, PM.index(3, 0, 1)])
        d = torch.full((4 * 64,), SENT, dtype=torch.int64, device="cuda")
        pl.dp[0].across_windows(pl.body[0], pl.dp[1:3], pl.body[1:3], [131040], [64], d, 1, pl.stream)
        torch.cuda.synchronize()
        acr = d.cpu().numpy().view(A.ACROSS_RECORD)
        stack = np.stack([f[131040:131104] for _, f in streams[:3]])
        assert np.array_equal(acr["count"], np.full(64, 3)) and np.array_equal(acr["min"], stack.min(axis=0))
        assert _equal(pl.matrix(wb, order=[0, 1]), want2)
    finally:
        pl.close()


def test_validation(A, ctx, torch):
    n, nf = 256, 8
    off = np.arange(nf + 1, dtype=np.uint64) * n
    e = float(np.float32(0.05))
    recs = [ctx.compress_host(H.synth_series(3160 + k, n * nf, klass=2), off, A.FFT, True, e, 0)[0] for k in range(2)]
    short = ctx.compress_host(H.synth_series(3163, n * 5, klass=2), off[:6], A.FFT, True, e, 0)[0]
    lst = recs + [short]
    fulls = [ctx.decompress_host(r) for r in lst]
    lib = A.capi.lib()
    p64 = C.POINTER(C.c_uint64)
    P3 = PM.records(3)

    def arr(v):
        return np.array(v, dtype=np.uint64)

    def host(bodies, wins, n_streams=None, null_list=False):
        out = np.full(max(len(wins), 1) * P3, 0, dtype=A.WINDOW_PAIR)
        out["mean_x"] = 7.0
        bufs = [np.frombuffer(b, dtype=np.uint8) if b is not None else None for b in bodies]
        ptrs = (C.c_void_p * max(len(bufs), 1))(*[b.ctypes.data if b is not None else None for b in bufs])
        lens = arr([len(b) if b is not None else 0 for b in bufs] or [0])
        flags = np.zeros(max(len(bufs), 1), dtype=np.int32)
        b, c = arr([w[0] for w in wins] or [0]), arr([w[1] for w in wins] or [0])
        rc = lib.atsc_pair_matrix_windows(ctx._h, len(bufs) if n_streams is None else n_streams, None if null_list else ptrs,
                                          lens.ctypes.data_as(p64), flags.ctypes.data_as(C.POINTER(C.c_int32)), len(wins),
                                          b.ctypes.data_as(p64), c.ctypes.data_as(p64), C.c_void_p(out.ctypes.data))
        return rc, out

    def untouched(out):
        return bool(np.all(out["mean_x"] == 7.0) and np.all(out["count"] == 0))

    # the host call: the list, a window beyond the end of ANY stream
    for bodies, wins, kw in ((lst, [(0, 5)], {"n_streams": 0}), (lst, [(0, 5)], {"n_streams": 65}), (lst, [(0, 5)], {"null_list": True}),
                             ([recs[0], None, short], [(0, 5)], {}), (lst, [(5 * n - 2, 4)], {}), (lst, [(0, 5), (5 * n + 1, 0)], {}),
                             ([short] + recs, [(0, 5 * n + 1)], {}), (lst, [(2 ** 63, 2 ** 63)], {})):
        rc, out = host(bodies, wins, **kw)
        assert rc == A.capi.E_INVALID and untouched(out), (wins, kw, rc)
        assert b"pair_matrix_windows" in lib.atsc_ctx_last_error(ctx._h), (wins, kw)
    rc, out = host(lst, [(0, 5 * n), (5 * n, 0), (5 * n - 1, 1)])
    assert rc == 0
    _check_model(fulls, [(0, 5 * n), (5 * n, 0), (5 * n - 1, 1)], out[: 3 * P3].reshape(3, P3), label="shorter stream")
    rc, out = host(lst, [])
    assert rc == 0 and untouched(out)
    # the device call: nothing enqueued, nothing written
    dps = [A.DPlan(ctx, r) for r in lst]
    bodies = [torch.from_numpy(np.frombuffer(r, dtype=np.uint8).copy()).to("cuda") for r in lst]
    ctx2 = A.Context(0)
    dp2 = A.DPlan(ctx2, recs[1])
    d_out = torch.full((6 * P3 + 1,), SENT, dtype=torch.int64, device="cuda")
    one, cnt = arr([0]), arr([10])
    many = 0xfffffffe // 2080 + 1  # with 64 streams W * P is more than 2^32 - 2 records
    zb = np.zeros(many, dtype=np.uint64)

    def dev(plans, bods, ptr, n_streams=None, n_windows=1, b=one, c=cnt, null=()):
        hp = (C.c_void_p * 65)(*[d._h.value if d is not None else None for d in plans])
        hb = (C.c_void_p * 65)(*[t.data_ptr() if t is not None else None for t in bods])
        return lib.atsc_pair_matrix_windows_dev(ctx._h, len(plans) if n_streams is None else n_streams,
                                                None if "dp" in null else hp, None if "body" in null else hb, n_windows,
                                                b.ctypes.data_as(p64), c.ctypes.data_as(p64), C.c_void_p(ptr), None)

    inv = A.capi.E_INVALID
    assert dev(dps, bodies, d_out.data_ptr(), n_streams=0) == inv
    assert dev(dps, bodies, d_out.data_ptr(), n_streams=65) == inv
    assert dev(dps, bodies, d_out.data_ptr(), null=("dp",)) == inv
    assert dev(dps, bodies, d_out.data_ptr(), null=("body",)) == inv
    assert dev([dps[0], None, dps[2]], bodies, d_out.data_ptr()) == inv
    assert dev(dps, [bodies[0], bodies[1], None], d_out.data_ptr()) == inv
    assert dev([dps[0], dp2, dps[2]], bodies, d_out.data_ptr()) == inv  # plans of different contexts
    assert dev(dps, bodies, d_out.data_ptr(), c=arr([5 * n + 1])) == inv  # beyond the third stream only
    assert dev(dps[::-1], bodies[::-1], d_out.data_ptr(), c=arr([5 * n + 1])) == inv
    assert dev(dps, bodies, d_out.data_ptr() + 4) == inv
    assert dev(dps, bodies, 0) == inv
    assert dev([dps[0]] * 64, [bodies[0]] * 64, d_out.data_ptr(), n_windows=many, b=zb, c=zb) == inv
    assert b"pair_matrix_windows: more than 2^32 - 2 records" in lib.atsc_ctx_last_error(ctx._h)
    torch.cuda.synchronize()
    assert bool((d_out == SENT).all())
    assert dev(dps, bodies, d_out.data_ptr(), n_windows=0) == 0
    torch.cuda.synchronize()
    assert bool((d_out == SENT).all())
    assert dev(dps, bodies, d_out.data_ptr()) == 0
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert got[6 * P3] == SENT
    _check_model(fulls, [(0, 10)], got[: 6 * P3].view(A.WINDOW_PAIR).reshape(1, P3), label="device")
    for d in dps + [dp2]:
        d.close()
    ctx2.close()


def test_malformed_payload_in_stream_2(A, ctx, torch):
    n, nf = 256, 8
    off = np.arange(nf + 1, dtype=np.uint64) * n
    e = float(np.float32(0.05))
    recs = [ctx.compress_host(H.synth_series(3170 + k, n * nf, klass=2), off, A.FFT, True, e, 0)[0] for k in range(3)]
    fulls = [ctx.decompress_host(r) for r in recs]
    frames = H.parse_bro_body(recs[2], with_count=False)
    pos = sum(len(_rec(f[1], f[2], f[3])) for f in frames[:3])
    pay = pos + len(_rec(frames[3][1], frames[3][2], frames[3][3])) - len(frames[3][3])
    assert recs[2][pay] == 15 and recs[2][pay + 1] < 200
    bad = bytearray(recs[2])
    bad[pay + 1] = 250  # stream 2, frame 3: more stored bins than the transform has; the record walk stays valid
    lst = [recs[0], recs[1], bytes(bad)]
    for wins in ([(3 * n, 1)], [(0, nf * n)], [(0, 10), (3 * n - 1, 2)], [(4 * n - 1, 1), (6 * n, 5)]):
        with pytest.raises(A.AtscError) as ei:
            ctx.pair_matrix_windows_host(lst, [w[0] for w in wins], [w[1] for w in wins])
        assert ei.value.rc == A.capi.E_FORMAT, wins
        # the status word is that plan's only: the same windows over the two good streams give their records
        ok = ctx.pair_matrix_windows_host(lst[:2], [w[0] for w in wins], [w[1] for w in wins])
        _check_model(fulls[:2], wins, ok, label="good streams")
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 10, 10), (3 * n + 5, 0)]
    _check_model(fulls, outside, ctx.pair_matrix_windows_host(lst, [w[0] for w in outside], [w[1] for w in outside]), label="outside")
    # the device call returns ATSC_OK, finishes and writes every record; the windows beside the bad frame are right
    pl = _Plans(A, ctx, torch, lst)
    try:
        wins = [(0, 3 * n), (3 * n + 7, 20), (4 * n, 100)]
        got = pl.matrix(wins)
        assert not np.any(got["count"].view(np.int64) == SENT)
        _check_model(fulls, [wins[0], wins[2]], got[[0, 2]], label="device, beside the bad frame")
        _check_model(fulls[:2], wins, np.ascontiguousarray(got[:, [PM.index(3, 0, 0), PM.index(3, 0, 1), PM.index(3, 1, 1)]]),
                     label="device, the good streams")
    finally:
        pl.close()


def _run(*args, code=0):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == code, (args, r.stdout, r.stderr)
    return r


def test_surfaces_and_command_line(A, ctx, torch, tmp_path):
    """the device call, the host call with and without the frame count in front, the stream call and the image call give
    the same records; atsc --pair-matrix writes what pair_fit reads off them; the misuse messages"""
    n = 30000
    e = float(np.float32(0.03))
    vals = [H.synth_series(3180, n, block=5000), None, H.synth_series(3182, n, klass=1)]
    vals[1] = 0.3 * vals[0] + H.synth_series(3181, n, klass=2)
    offs = [H.frame_offsets(n, 1024), H.frame_offsets(n - 2000, 700), H.frame_offsets(n, 4096)]
    recs = [ctx.compress_host(vals[0], offs[0], A.AUTO, True, e, 0)[0],
            ctx.compress_host(vals[1][: n - 2000], offs[1], A.FFT, True, float(np.float32(0.01)), 0)[0],  # the shorter one
            ctx.compress_host(vals[2], offs[2], A.POLYNOMIAL, True, e, 0)[0]]
    fulls = [ctx.decompress_host(r) for r in recs]
    m = len(fulls[1])
    wins = [(0, m), (0, 0), (m, 0), (m - 1, 1), (700 - 1, 2), (1024 - 3, 7), (4096, 1), (2 * T - 5, T + 11), (5, 3 * T), (12000, 9000)]
    b, c = [w[0] for w in wins], [w[1] for w in wins]
    host = ctx.pair_matrix_windows_host(recs, b, c)
    assert host.shape == (len(wins), 6) and host.dtype == A.WINDOW_PAIR
    _check_model([f[:m] for f in fulls], wins, host, label="host")
    pl = _Plans(A, ctx, torch, recs)
    try:
        assert _equal(pl.matrix(wins), host)
    finally:
        pl.close()
    bros = [A.bro_prefix(len(o) - 1) + r for o, r in zip(offs, recs)]
    assert _equal(ctx.pair_matrix_windows_host([x[9:] for x in bros], b, c, has_count=True), host)
    assert _equal(A.pair_matrix_data_windows(ctx, bros, b, c), host)
    ss = [A.CompressedStream.from_bytes(ctx, x) for x in bros]
    assert _equal(ss[0].pair_matrix_windows(ss[1:], b, c), host)
    one = ss[1].pair_matrix_windows([], b, c)
    assert one.shape == (len(wins), 1) and _equal(one[:, 0], host[:, PM.index(3, 1, 1)])
    corr = A.pair_matrix_correlation(host, 3)
    assert corr.shape == (len(wins), 3, 3) and corr[0, 0, 1] == corr[0, 1, 0] and abs(corr[0, 0, 1]) <= 1.0
    with pytest.raises(A.AtscError) as ei:
        ss[0].pair_matrix_windows(ss[1:], [m - 1], [2])
    assert ei.value.rc == A.capi.E_INVALID
    s0 = A.CompressedStream(ctx)  # a stream without a frame admits only empty windows at 0
    e0 = ss[0].pair_matrix_windows([s0], [0, 0], [0, 0])
    assert e0.shape == (2, 3) and np.all(e0["count"] == 0) and np.all(np.isnan(e0["c_xy"]))
    with pytest.raises(A.AtscError):
        ss[0].pair_matrix_windows([s0], [0], [1])
    # the command line
    atsc = os.path.join(os.path.dirname(A.__file__), "bin", "atsc")
    names = ("x.bro", "y.bro", "z.bro")
    for name, x in zip(names, bros):
        (tmp_path / name).write_bytes(x)
    others = "%s,%s" % (tmp_path / "y.bro", tmp_path / "z.bro")
    for extra, (b0, c0) in ((("--samples", "0:%d" % m), (0, m)), (("--samples", "100:1500"), (100, 1500))):
        for nb in (1000, m + 1):
            _run(atsc, "-u", "--buckets", nb, *extra, tmp_path / "x.bro")
            plain = open(tmp_path / "x.agg.csv").read()
            _run(atsc, "-u", "--buckets", nb, *extra, "--pair-matrix", others, tmp_path / "x.bro")
            assert open(tmp_path / "x.agg.csv").read() == plain  # the .agg.csv is what it was
            lines = open(tmp_path / "x.pairs.csv").read().split("\n")
            assert lines[0] == "bucket,begin,count,i,j,pair_count,mean_i,mean_j,covariance,correlation,slope,intercept" and lines[-1] == ""
            rows = [l.split(",") for l in lines[1:] if l]
            bb, bc = A.bucket_windows(b0, c0, nb)
            want = ctx.pair_matrix_windows_host(recs, bb, bc)
            fit = A.pair_fit(want.reshape(-1)).reshape(want.shape)
            assert len(rows) == len(bb) * 6
            k = 0
            for w in range(len(bb)):
                for i, j in PM.pairs(3):
                    r, rec, f = rows[k], want[w, PM.index(3, i, j)], fit[w, PM.index(3, i, j)]
                    assert [int(v) for v in r[:6]] == [w, int(bb[w]), int(bc[w]), i, j, int(rec["count"])], (extra, nb, r)
                    cells = np.array([rec["mean_x"], rec["mean_y"], f["covariance"], f["correlation"], f["slope"], f["intercept"]])
                    cells[np.isnan(cells)] = np.nan  # the text form keeps no NaN payload
                    assert _bits([float(v) for v in r[6:]]).tolist() == _bits(cells).tolist(), (extra, nb, r)
                    k += 1
    # a listed file shorter than the bucketed range: a runtime error with the library's message
    r = _run(atsc, "-u", "--buckets", 1000, "--pair-matrix", others, tmp_path / "x.bro", code=1)
    assert "window beyond the stream" in r.stderr
    # misuse
    r = _run(atsc, "-u", "--samples", "0:100", "--pair-matrix", others, tmp_path / "x.bro", code=2)
    assert "error: '--pair-matrix' needs '--buckets'" in r.stderr
    r = _run(atsc, "-u", "--buckets", 100, "--pair", tmp_path / "y.bro", "--pair-matrix", others, tmp_path / "x.bro", code=2)
    assert "error: '--pair-matrix' cannot be used with '--pair'" in r.stderr
    for v in ("", "%s,,%s" % (tmp_path / "y.bro", tmp_path / "z.bro"), ",".join(["y.bro"] * 64)):
        r = _run(atsc, "-u", "--buckets", 100, "--pair-matrix", v, tmp_path / "x.bro", code=2)
        assert "for '--pair-matrix': expected 1..=63 paths of .bro files, comma separated" in r.stderr, v
    cc = os.path.join(os.path.dirname(A.__file__), "bin", "csv-compressor")
    r = _run(cc, "--pair-matrix", others, tmp_path / "x.bro", code=2)
    assert "unexpected argument '--pair-matrix'" in r.stderr
