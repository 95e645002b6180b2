"""Windowed pair moments on the GPU: every window of every case against the NumPy model of the documented merge tree
(tests/pair_model.py) applied to the GPU's own full decodes of the two streams -- all six fields bit for bit, any NaN
equal to any NaN, no tolerance.  X holds every frame-length tier below the large one and every codec, Y the same samples'
count in other frame lengths and codecs, once with 131072-sample frames (the large tier's launch sequence and spill
slots on one input only); windows inside a tile, across tile and frame boundaries of either stream, of lengths 0, 1 and
2, overlapping, unsorted; 64 and 66 tiles in one window; budgets that cut a window into pieces; NaN and Inf in either
input; the two identities of the contract; a plan reused and shared with other queries; validation and a malformed
payload; the device, host, stream and Python surfaces and the command line."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import pair_model as P

pytestmark = pytest.mark.gpu

T = P.TILE
N = 2 * 131072 + 40000  # samples of the two main streams
LENS = [1, 7, 64, 128, 256, 300, 512, 513, 1024, 2048, 4096]


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


def _fft_record(rng, n, k):
    """a hand-built FFT record of n samples with k stored bins (positions below n / 2)"""
    p = bytes([15]) + bytes([k])
    for pos in rng.choice(np.arange(1, n // 2), size=k, replace=False):
        pos = int(pos)
        p += (bytes([pos]) if pos < 251 else b"\xfb" + struct.pack("<H", pos))
        p += struct.pack("<ff", *rng.normal(0, 50 * n, 2).astype(np.float32))
    p += struct.pack("<ff", 400.0, -400.0)
    return _rec(n, 1, p)


def _const_record(A, ctx, value, n):
    """a Constant record of n samples of `value` as it is (NaN, +-Inf included): the library's own 64-bit Constant
    record of a stand-in, with the stored double replaced"""
    r, _, _, _ = ctx.compress_host(np.full(n, 1.5), np.array([0, n], dtype=np.uint64), A.CONSTANT, False, 0.0, 0)
    assert r.endswith(struct.pack("<d", 1.5))
    return r[:-8] + struct.pack("<d", value)


def _idw_record(values):
    """a hand-built IDW record whose points are the samples themselves (f64 points, point step 1, min -Inf, max +Inf):
    every sample decodes to its point, NaN and +-Inf included"""
    n = len(values)
    p = _v(1) + _v(0) + _v(n) + struct.pack("<%dd" % n, *values) + struct.pack("<dd", -np.inf, np.inf) + bytes([1])
    return _rec(n, 2, p)


def _idw_stream(x, frame):
    return b"".join(_idw_record(x[k:k + frame].tolist()) for k in range(0, len(x), frame))


def _frame_lens(recs):
    return [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in H.parse_bro_body(recs, with_count=False)]


@pytest.fixture(scope="module")
def streams(A, ctx):
    """X: every frame length of LENS (every tier below the large one) under auto at e = 5 / 1 / 0 % and forced fft,
    polynomial, idw, rle, constant, noop, hand-built FFT records with 15 and 16 bins, then 4096-sample frames under auto
    up to N samples.  Y: N samples in frames of 1000 (polynomial) and 3000 (idw).  YL: N samples in two 131072-sample
    frames and one of 40000 (fft).  -> dict of name -> (records, full decode, frame lengths)"""
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.uint64)
    modes = [(A.AUTO, True, 0.05), (A.AUTO, True, 0.01), (A.AUTO, True, 0.0), (A.FFT, True, 0.05),
             (A.POLYNOMIAL, True, 0.05), (A.IDW, True, 0.05), (A.RLE, False, 0.0), (A.CONSTANT, False, 0.0),
             (A.NOOP, False, 0.0)]
    x = b""
    for m, (comp, bounded, me) in enumerate(modes):
        v = H.synth_series(2700 + m, int(off[-1]), block=3000)
        if comp == A.RLE:
            v = np.round(v / 8.0) * 8.0
        x += ctx.compress_host(v, off, comp, bounded, float(np.float32(me)), 0)[0]
    rng = np.random.default_rng(7)
    for n in (128, 256, 1024, 2048, 4096):
        for k in (15, 16):
            x += _fft_record(rng, n, k)
    rest = N - sum(_frame_lens(x))
    x += ctx.compress_host(H.synth_series(2750, rest, block=20000), H.frame_offsets(rest, 4096), A.AUTO, True,
                           float(np.float32(0.05)), 0)[0]
    h = 150000
    y = ctx.compress_host(H.synth_series(2760, h, klass=2), H.frame_offsets(h, 1000), A.POLYNOMIAL, True,
                          float(np.float32(0.03)), 0)[0]
    y += ctx.compress_host(H.synth_series(2761, N - h, klass=0), H.frame_offsets(N - h, 3000), A.IDW, True,
                           float(np.float32(0.03)), 0)[0]
    loff = np.array([0, 131072, 262144, N], dtype=np.uint64)
    yl = ctx.compress_host(H.synth_series(2770, N, klass=1), loff, A.FFT, True, float(np.float32(0.01)), 0)[0]
    out = {}
    for name, r in (("X", x), ("Y", y), ("YL", yl)):
        full = ctx.decompress_host(r)
        lens = _frame_lens(r)
        assert len(full) == N == sum(lens), name
        out[name] = (r, full, lens)
    assert max(out["X"][2]) == 4096 and max(out["Y"][2]) == 3000 and out["YL"][2] == [131072, 131072, 40000]
    return out


def _windows(lens_x, lens_y, total, rng, n_random=25):
    """the whole stream, empty windows, lengths 1 and 2, every frame boundary of either stream and its neighbours, tile
    multiples and their neighbours, windows inside one tile, a few random ones up to 150000 samples -- unsorted, overlaps
    included"""
    w = {(0, total), (0, 0), (total, 0), (total - 1, 1), (0, 1), (0, 2), (total - 2, 2), (77, 0)}
    for s in set(np.cumsum(lens_x)[:-1].tolist()) | set(np.cumsum(lens_y)[:-1].tolist()):
        s = int(s)
        w.add((s - 1, 1))
        w.add((s, 1))
        w.add((s - 1, 2))
        w.add((max(s - 5, 0), min(11, total - max(s - 5, 0))))
    for k in rng.integers(1, total // T - 5, 12):
        k = int(k)
        for b, c in ((k * T, T), (k * T, 2 * T), (k * T, 5 * T), (k * T - 1, 2), (k * T + 1, T - 2), (k * T + T - 1, T + 2),
                     (k * T + 100, 1500), (k * T + 7, 2), (k * T, 1), (k * T + T - 2, 2)):
            w.add((b, c))
    for _ in range(n_random):
        b = int(rng.integers(0, total))
        w.add((b, int(rng.integers(0, min(total - b, 150000) + 1))))
    w = sorted(w)
    return [w[i] for i in rng.permutation(len(w))]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _equal(got, want, fields=P.FIELDS, want_fields=None):
    """the count and the five doubles bit for bit; any NaN equals any NaN"""
    want_fields = want_fields or fields
    if len(got) != len(want) or not np.array_equal(got[fields[0]], want[want_fields[0]]):
        return False
    for k, kw in zip(fields[1:], want_fields[1:]):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[kw])
        if not np.all((_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))):
            return False
    return True


def _check(fx, fy, wins, got, label=""):
    """every window against the model on the two full decodes"""
    assert len(got) == len(wins), label
    want = P.windows_pair(fx, fy, wins)
    for i, (b, c) in enumerate(wins):
        assert _equal(got[i:i + 1], want[i:i + 1]), (label, b, c, got[i], want[i])


def _to_dev(torch, recs):
    return torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")


def _dev(A, ctx, torch, rx, ry, wins, dpx=None, dpy=None):
    own_x, own_y = dpx is None, dpy is None
    if own_x:
        dpx = A.DPlan(ctx, rx)
    if own_y:
        dpy = A.DPlan(ctx, ry)
    bx, by = _to_dev(torch, rx), _to_dev(torch, ry)
    d_out = torch.full((max(len(wins), 1) * 6,), -1, dtype=torch.int64, device="cuda")
    dpx.pair_windows(bx, dpy, by, [w[0] for w in wins], [w[1] for w in wins], d_out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(A.WINDOW_PAIR)[: len(wins)].copy()
    if own_y:
        dpy.close()
    if own_x:
        dpx.close()
    return out


def _host(ctx, rx, ry, wins):
    return ctx.pair_windows_host(rx, ry, [w[0] for w in wins], [w[1] for w in wins])


@pytest.mark.parametrize("other", ["Y", "YL"])
def test_parity_with_full_decodes(A, ctx, torch, streams, other):
    (rx, fx, lx), (ry, fy, ly) = streams["X"], streams[other]
    wins = _windows(lx, ly, N, np.random.default_rng(223))
    got = _host(ctx, rx, ry, wins)
    _check(fx, fy, wins, got, other)
    assert _equal(_dev(A, ctx, torch, rx, ry, wins), got)


def test_64_and_66_tiles_in_one_window(A, ctx, torch):
    """64 partials fill one combine group exactly, 66 need a second pass: windows of 64 and 66 tiles (131072 and 135168
    samples) that do not start on a tile boundary, and neighbours on tile multiples, under the default budget and under
    the least one, whose pieces of 32 tiles cut every one of them"""
    n = 35 * 4096
    rng = np.random.default_rng(1642)
    # decoding rounds to the fifth decimal, so the samples are placed on it; a merge of these depends on its order
    x = np.round(rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 7, n), 5)
    y = np.round(0.5 * x + rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 5, n), 5)
    x[rng.integers(0, n, 300)] = np.nan
    y[rng.integers(0, n, 300)] = np.nan
    rx, ry = _idw_stream(x, 4096), _idw_stream(y, 2560)
    fx, fy = ctx.decompress_host(rx), ctx.decompress_host(ry)
    assert np.array_equal(np.isnan(fx), np.isnan(x)) and np.array_equal(fx[~np.isnan(x)], x[~np.isnan(x)])
    assert np.array_equal(np.isnan(fy), np.isnan(y)) and np.array_equal(fy[~np.isnan(y)], y[~np.isnan(y)])
    wins = [(2 * T + 1, 64 * T), (T + 7, 66 * T), (2 * T, 64 * T), (T, 66 * T), (2 * T - 1, 64 * T + 2), (5, 65 * T), (0, n)]
    try:
        for budget in (0, 1):
            ctx.set_aggregate_scratch(budget)
            got = _host(ctx, rx, ry, wins)
            _check(fx, fy, wins, got, "64 tiles, budget %d" % budget)
            assert _equal(_dev(A, ctx, torch, rx, ry, wins), got), budget
    finally:
        ctx.set_aggregate_scratch(0)


def test_budgets_pieces_and_plan_reuse(A, ctx, torch, streams):
    """one window of about 300000 samples in five and in three pieces and whole: the same bits; the batch around a
    window and repeated calls never change a bit; one pair of plans serves changing window lists; dp_x == dp_y"""
    (rx, fx, _), (ry, fy, _), (rl, fl, _) = streams["X"], streams["Y"], streams["YL"]
    rng = np.random.default_rng(231)
    probe = [(1000, 300000), (0, N), (5, 2043), (131071, 2), (N - 4097, 4097), (10, 0), (3 * T, 40 * T)]
    alone = _host(ctx, rx, ry, probe)
    _check(fx, fy, probe, alone, "probe")
    alone_l = _host(ctx, rx, rl, probe)
    _check(fx, fl, probe, alone_l, "probe, large")
    others = []
    for _ in range(200):
        c = int(rng.choice([1, 2, 60, 2048, 5000]))
        others.append((int(rng.integers(0, N - c + 1)), c))
    batch = probe + others
    order = rng.permutation(len(batch))
    got = _host(ctx, rx, ry, [batch[i] for i in order])
    back = np.empty_like(got)
    back[order] = got
    assert _equal(back[: len(probe)], alone)
    _check(fx, fy, others[:60], back[len(probe): len(probe) + 60], "others")
    dpx, dpy, dpl = A.DPlan(ctx, rx), A.DPlan(ctx, ry), A.DPlan(ctx, rl)
    try:
        # both regions inside the budget: 1 byte and 2 MiB give pieces of 65536 and 131072 samples per input, the window
        # (1000, 300000) in five and in three; with the large frames' spill slots the least piece holds under either
        for budget in (1, 2 << 20):
            ctx.set_aggregate_scratch(budget)
            assert _equal(_dev(A, ctx, torch, rx, ry, probe, dpx, dpy), alone), budget
            assert _equal(_dev(A, ctx, torch, rx, ry, probe[:1], dpx, dpy), alone[:1]), budget
            assert _equal(_dev(A, ctx, torch, rx, rl, probe, dpx, dpl), alone_l), budget
            assert _equal(_host(ctx, rx, rl, probe[:2]), alone_l[:2]), budget
    finally:
        ctx.set_aggregate_scratch(0)
    # the same plans, other windows, fewer and more than before, and again the first list
    assert _equal(_dev(A, ctx, torch, rx, ry, probe[:3], dpx, dpy), alone[:3])
    _check(fx, fy, others[:80], _dev(A, ctx, torch, rx, ry, others[:80], dpx, dpy), "reuse")
    assert len(_dev(A, ctx, torch, rx, ry, [], dpx, dpy)) == 0
    assert _equal(_dev(A, ctx, torch, rx, ry, probe, dpx, dpy), alone)
    # the same plan on both sides
    same = _dev(A, ctx, torch, rx, rx, probe, dpx, dpx)
    _check(fx, fx, probe, same, "dp_x == dp_y")
    for dp in (dpx, dpy, dpl):
        dp.close()


def test_nan_and_inf(A, ctx, torch):
    """NaN in X only, in Y only and in both; a whole tile of NaN in one input and aligned stretches of 128 slots of it
    (the equal-count fast path then holds in some of a wavefront's passes and not in others); +-Inf"""
    nan, inf = float("nan"), float("inf")
    n = 8 * T
    rng = np.random.default_rng(241)
    x = np.round(rng.normal(0, 100, n), 5)
    y = np.round(rng.normal(5, 3, n), 5)
    x[rng.random(n) < 0.02] = nan  # scattered: tiles 0 .. 7 of X
    y[T + np.flatnonzero(rng.random(T) < 0.1)] = nan  # tile 1 of Y
    x[T + 40:T + 60] = nan
    y[T + 50:T + 70] = nan  # both
    x[2 * T:3 * T] = np.round(rng.normal(0, 1, T), 5)
    y[2 * T:3 * T] = nan  # a whole tile of NaN in Y only
    x[3 * T:4 * T] = np.round(rng.normal(0, 1, T), 5)  # tile 3: no NaN but in aligned stretches of 128 slots
    y[3 * T + 512:3 * T + 640] = nan
    x[3 * T + 1280:3 * T + 1408] = nan
    x[4 * T:6 * T] = np.round(rng.normal(1e9, 1e-3, 2 * T), 5)  # tiles 4, 5 without NaN: every merge of equal counts
    x[6 * T + 5] = inf
    y[6 * T + 9] = -inf
    x[6 * T + 300] = -inf
    y[6 * T + 300] = inf
    rx = _idw_stream(x, 4096)
    ry = _const_record(A, ctx, 2.5, T) + _idw_stream(y[T:2 * T], 1000) + _const_record(A, ctx, nan, T) + _idw_stream(y[3 * T:], 3000)
    y[:T] = 2.5
    fx, fy = ctx.decompress_host(rx), ctx.decompress_host(ry)
    for f, v in ((fx, x), (fy, y)):
        assert np.array_equal(np.isnan(f), np.isnan(v)) and np.array_equal(f[~np.isnan(v)], v[~np.isnan(v)])
    wins = [(0, n), (0, T), (T, T), (2 * T, T), (2 * T, 1), (3 * T, T), (4 * T, 2 * T), (4 * T + 1, 2 * T - 2), (6 * T, T),
            (6 * T, 8), (6 * T, 10), (6 * T + 300, 1), (6 * T + 299, 3), (T + 30, 50), (T + 45, 10), (T + 55, 10),
            (T + 55, 0), (2 * T - 3, T + 6), (3 * T + 500, 200), (3 * T + 512, 128), (T, 3 * T), (5, 7 * T), (7 * T, T)]
    got = _host(ctx, rx, ry, wins)
    _check(fx, fy, wins, got, "nonfinite")
    assert _equal(_dev(A, ctx, torch, rx, ry, wins), got)
    r = dict(zip(wins, got))
    for w in ((2 * T, T), (2 * T, 1), (T + 55, 0), (3 * T + 512, 128), (T + 55, 10)):  # nothing counts: five NaN
        assert int(r[w]["count"]) == 0 and all(np.isnan(r[w][k]) for k in P.FIELDS[1:]), w
    ok = ~(np.isnan(x) | np.isnan(y))
    assert int(r[(0, n)]["count"]) == int(ok.sum()) and int(r[(3 * T, T)]["count"]) == T - 256
    assert int(r[(4 * T, 2 * T)]["count"]) == 2 * T and int(r[(T + 45, 10)]["count"]) == 0
    assert r[(0, T)]["m2_y"] == 0.0 and r[(0, T)]["c_xy"] == 0.0 and r[(0, T)]["mean_y"] == 2.5  # a constant input
    assert int(r[(6 * T, 8)]["count"]) == 8 - int((~ok[6 * T:6 * T + 8]).sum())
    w = r[(4 * T, 2 * T)]  # 1e9 +- 1e-3: the spread survives
    assert abs(w["m2_x"] / w["count"] - np.var(fx[4 * T:6 * T])) < 1e-8


def test_identities(A, ctx, torch, streams):
    """X and Y swapped: the x and y fields swapped, bit for bit; Y the same stream as X: the moments' mean and m2"""
    (rx, fx, lx), (ry, fy, ly) = streams["X"], streams["YL"]
    wins = _windows(lx[:40], ly, N, np.random.default_rng(251), n_random=10)
    xy, yx = _host(ctx, rx, ry, wins), _host(ctx, ry, rx, wins)
    assert _equal(yx, xy, ("count", "mean_y", "m2_y", "mean_x", "m2_x", "c_xy"), P.FIELDS)
    xx = _dev(A, ctx, torch, rx, rx, wins)
    mom = ctx.moments_windows_host(rx, [w[0] for w in wins], [w[1] for w in wins])
    assert np.array_equal(xx["count"], mom["count"])
    for k, km in (("mean_x", "mean"), ("mean_y", "mean"), ("m2_x", "m2"), ("m2_y", "m2"), ("c_xy", "m2")):
        g, w = np.ascontiguousarray(xx[k]), np.ascontiguousarray(mom[km])
        assert np.all((_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))), k
    _check(fx, fx, wins[:40], xx[:40], "X, X")


def test_interleaved_with_moments_and_aggregates(A, ctx, torch, streams):
    """pair, moments and aggregate calls enqueued back to back on the same two plans: every result is that of plans
    that never saw another kind of call"""
    (rx, fx, _), (ry, fy, _) = streams["X"], streams["YL"]
    rng = np.random.default_rng(257)
    wp = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, N - 100000, 20)] + [(7, N - 7)]
    wo = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, N - 100000, 25)] + [(0, N)]
    bx, by = _to_dev(torch, rx), _to_dev(torch, ry)
    s = torch.cuda.current_stream().cuda_stream

    def call(fn, wins):
        d = torch.full((len(wins) * 6,), -1, dtype=torch.int64, device="cuda")
        fn([w[0] for w in wins], [w[1] for w in wins], d, s)
        return d

    def alone(rec, body, what, wins):
        dp = A.DPlan(ctx, rec)
        d = call(lambda b, c, d, s: getattr(dp, what)(body, b, c, d, s), wins)
        torch.cuda.synchronize()
        out = d.cpu().numpy().tobytes()
        dp.close()
        return out

    p_alone = _dev(A, ctx, torch, rx, ry, wp)
    mx_alone, ay_alone = alone(rx, bx, "moments_windows", wo), alone(ry, by, "aggregate_windows", wo)
    my_alone, ax_alone = alone(ry, by, "moments_windows", wp), alone(rx, bx, "aggregate_windows", wp)
    dpx, dpy = A.DPlan(ctx, rx), A.DPlan(ctx, ry)
    outs = []
    for _ in range(2):  # no synchronisation between the kinds
        outs.append((call(lambda b, c, d, s: dpx.pair_windows(bx, dpy, by, b, c, d, s), wp),
                     call(lambda b, c, d, s: dpx.moments_windows(bx, b, c, d, s), wo),
                     call(lambda b, c, d, s: dpy.aggregate_windows(by, b, c, d, s), wo),
                     call(lambda b, c, d, s: dpy.pair_windows(by, dpx, bx, b, c, d, s), wp),
                     call(lambda b, c, d, s: dpy.moments_windows(by, b, c, d, s), wp),
                     call(lambda b, c, d, s: dpx.aggregate_windows(bx, b, c, d, s), wp)))
    torch.cuda.synchronize()
    for p, mx, ay, q, my, ax in outs:
        assert _equal(p.cpu().numpy().view(A.WINDOW_PAIR), p_alone)
        assert _equal(q.cpu().numpy().view(A.WINDOW_PAIR), p_alone, ("count", "mean_y", "m2_y", "mean_x", "m2_x", "c_xy"), P.FIELDS)
        assert mx.cpu().numpy().tobytes() == mx_alone and ay.cpu().numpy().tobytes() == ay_alone
        assert my.cpu().numpy().tobytes() == my_alone and ax.cpu().numpy().tobytes() == ax_alone
    dpx.close()
    dpy.close()
    _check(fx, fy, wp[:8], p_alone[:8], "interleaved")


def test_validation(A, ctx, torch):
    n, nf = 256, 8
    x = H.synth_series(2909, n * nf, klass=2)
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.05)), 0)
    short = ctx.compress_host(x[: 5 * n], off[:6], A.FFT, True, float(np.float32(0.05)), 0)[0]
    good, good_short = ctx.decompress_host(recs), ctx.decompress_host(short)
    frames = H.parse_bro_body(recs, with_count=False)
    pos = sum(len(_rec(f[1], f[2], f[3])) for f in frames[:3])
    rec3 = _rec(frames[3][1], frames[3][2], frames[3][3])
    pay = pos + len(rec3) - len(frames[3][3])
    assert recs[pay] == 15 and recs[pay + 1] < 200
    bad = bytearray(recs)
    bad[pay + 1] = 250  # frame 3: more stored bins than the transform has, which the decoder refuses; the walk stays valid
    bad = bytes(bad)
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 10, 10), (5 * n + 3, 100), (0, 0), (3 * n + 5, 0)]
    _check(good, good, outside, _host(ctx, recs, bad, outside), "outside")
    lib = A.capi.lib()
    p = C.POINTER(C.c_uint64)
    u8 = C.POINTER(C.c_uint8)

    def raw(bx, by, wins):
        out = np.full(max(len(wins), 1), 0, dtype=A.WINDOW_PAIR)
        out["mean_x"] = 7.0
        b = np.array([w[0] for w in wins], dtype=np.uint64)
        c = np.array([w[1] for w in wins], dtype=np.uint64)
        ax, ay = np.frombuffer(bx, dtype=np.uint8), np.frombuffer(by, dtype=np.uint8)
        rc = lib.atsc_pair_windows(ctx._h, ax.ctypes.data_as(u8), len(ax), 0, ay.ctypes.data_as(u8), len(ay), 0, len(wins),
                                   b.ctypes.data_as(p), c.ctypes.data_as(p), C.c_void_p(out.ctypes.data))
        return rc, out

    # a corrupted payload in Y only (and in X only): ATSC_E_FORMAT, out untouched
    for wins in ([(3 * n, 1)], [(0, nf * n)], [(0, 10), (3 * n - 1, 2)], [(4 * n - 1, 1), (6 * n, 5)]):
        for bx, by in ((recs, bad), (bad, recs)):
            rc, out = raw(bx, by, wins)
            assert rc == A.capi.E_FORMAT and np.all(out["mean_x"] == 7.0), (wins, rc)
    # a window beyond the end of either stream
    for bx, by, wins in ((recs, recs, [(nf * n - 2, 4)]), (recs, recs, [(0, 5), (nf * n + 1, 0)]), (recs, recs, [(2 ** 63, 2 ** 63)]),
                         (recs, short, [(5 * n - 2, 4)]), (short, recs, [(0, 5 * n + 1)]), (recs, short, [(0, 5), (5 * n + 1, 0)])):
        rc, out = raw(bx, by, wins)
        assert rc == A.capi.E_INVALID and np.all(out["mean_x"] == 7.0), (wins, rc)
    rc, out = raw(recs, short, [(0, 5 * n), (5 * n, 0), (5 * n - 1, 1)])
    assert rc == 0 and int(out["count"][0]) == 5 * n
    _check(good, good_short, [(0, 5 * n), (5 * n, 0), (5 * n - 1, 1)], out, "shorter y")
    rc, _ = raw(recs, short, [])
    assert rc == 0
    e = _host(ctx, recs, short, [(5, 0), (5 * n, 0)])
    assert np.all(e["count"] == 0) and all(np.all(np.isnan(e[k])) for k in P.FIELDS[1:])
    # the device call: a window beyond the shorter plan, a misaligned result, null arguments, plans of two contexts --
    # nothing enqueued
    dpx, dps = A.DPlan(ctx, recs), A.DPlan(ctx, short)
    ctx2 = A.Context(0)
    dp2 = A.DPlan(ctx2, recs)
    body, sbody = _to_dev(torch, recs), _to_dev(torch, short)
    d_out = torch.full((13,), -1, dtype=torch.int64, device="cuda")
    one = np.array([0], dtype=np.uint64)
    cnt = np.array([5 * n + 1], dtype=np.uint64)

    def dev(hx, d_bx, hy, d_by, ptr):
        return lib.atsc_pair_windows_dev(ctx._h, hx, C.c_void_p(d_bx), hy, C.c_void_p(d_by), 1, one.ctypes.data_as(p),
                                         cnt.ctypes.data_as(p), C.c_void_p(ptr), None)

    assert dev(dpx._h, body.data_ptr(), dps._h, sbody.data_ptr(), d_out.data_ptr()) == A.capi.E_INVALID
    assert dev(dps._h, sbody.data_ptr(), dpx._h, body.data_ptr(), d_out.data_ptr()) == A.capi.E_INVALID
    cnt[0] = 10
    assert dev(dpx._h, body.data_ptr(), dps._h, sbody.data_ptr(), d_out.data_ptr() + 4) == A.capi.E_INVALID
    assert dev(dpx._h, body.data_ptr(), dps._h, sbody.data_ptr(), 0) == A.capi.E_INVALID
    assert dev(None, body.data_ptr(), dps._h, sbody.data_ptr(), d_out.data_ptr()) == A.capi.E_INVALID
    assert dev(dpx._h, body.data_ptr(), None, sbody.data_ptr(), d_out.data_ptr()) == A.capi.E_INVALID
    assert dev(dpx._h, body.data_ptr(), dps._h, 0, d_out.data_ptr()) == A.capi.E_INVALID
    assert dev(dpx._h, body.data_ptr(), dp2._h, body.data_ptr(), d_out.data_ptr()) == A.capi.E_INVALID
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())
    assert dev(dpx._h, body.data_ptr(), dps._h, sbody.data_ptr(), d_out.data_ptr()) == 0
    torch.cuda.synchronize()
    _check(good, good_short, [(0, 10)], d_out.cpu().numpy()[:6].view(A.WINDOW_PAIR), "device, shorter y")
    for dp in (dpx, dps, dp2):
        dp.close()
    ctx2.close()


def _run(*args, code=0):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == code, (args, r.stdout, r.stderr)
    return r


def test_surfaces_and_command_line(A, ctx, torch, tmp_path):
    """the device call, the host call, the stream call and the Python stream object give the same records, with and
    without the frame count in front; atsc --pair writes the fit of those records bit for bit"""
    rng = np.random.default_rng(263)
    n = 30000
    vx = H.synth_series(2801, n, block=5000)
    vy = 0.3 * vx + H.synth_series(2802, n, klass=2)
    ox, oy = H.frame_offsets(n, 1024), H.frame_offsets(n - 2000, 700)
    rx = ctx.compress_host(vx, ox, A.AUTO, True, float(np.float32(0.03)), 0)[0]
    ry = ctx.compress_host(vy[: n - 2000], oy, A.FFT, True, float(np.float32(0.01)), 0)[0]  # the shorter one
    fx, fy = ctx.decompress_host(rx), ctx.decompress_host(ry)
    m = len(fy)
    wins = _windows(np.diff(ox.astype(np.int64)).tolist()[:-2], np.diff(oy.astype(np.int64)).tolist(), m, rng, n_random=10)
    b, c = [w[0] for w in wins], [w[1] for w in wins]
    host = ctx.pair_windows_host(rx, ry, b, c)
    _check(fx[:m], fy, wins, host, "host")
    assert _equal(_dev(A, ctx, torch, rx, ry, wins), host)
    brx, bry = A.bro_prefix(len(ox) - 1) + rx, A.bro_prefix(len(oy) - 1) + ry
    assert np.array_equal(A.decompress_data(ctx, brx), fx) and np.array_equal(A.decompress_data(ctx, bry), fy)
    assert _equal(ctx.pair_windows_host(brx[9:], bry[9:], b, c, has_count=True), host)
    sx, sy = A.CompressedStream.from_bytes(ctx, brx), A.CompressedStream.from_bytes(ctx, bry)
    assert _equal(sx.pair_windows(sy, b, c), host)
    assert _equal(sy.pair_windows(sx, b, c), host, ("count", "mean_y", "m2_y", "mean_x", "m2_x", "c_xy"), P.FIELDS)
    with pytest.raises(A.AtscError) as ei:
        sx.pair_windows(sy, [m - 1], [2])
    assert ei.value.rc == A.capi.E_INVALID
    s0 = A.CompressedStream(ctx)  # a stream without a frame admits only empty windows at 0
    e = sx.pair_windows(s0, [0, 0], [0, 0])
    assert np.all(e["count"] == 0) and np.all(np.isnan(e["c_xy"]))
    with pytest.raises(A.AtscError):
        sx.pair_windows(s0, [0], [1])
    ctx2 = A.Context(0)
    s2 = A.CompressedStream.from_bytes(ctx2, bry)
    with pytest.raises(A.AtscError) as ei:
        sx.pair_windows(s2, [0], [1])
    assert ei.value.rc == A.capi.E_INVALID
    del s2
    ctx2.close()
    # the command line
    atsc = os.path.join(os.path.dirname(A.__file__), "bin", "atsc")
    (tmp_path / "x.bro").write_bytes(brx)
    (tmp_path / "y.bro").write_bytes(bry)
    cols = ",pair_count,covariance,correlation,slope,intercept"
    for extra, (b0, c0) in ((("--samples", "0:%d" % m), (0, m)), (("--samples", "100:1500"), (100, 1500))):
        for nb in (60, 1000, m + 1):
            _run(atsc, "-u", "--buckets", nb, *extra, "--moments", tmp_path / "x.bro")
            plain = open(tmp_path / "x.agg.csv").read().split("\n")
            _run(atsc, "-u", "--buckets", nb, *extra, "--moments", "--pair", tmp_path / "y.bro", tmp_path / "x.bro")
            lines = open(tmp_path / "x.agg.csv").read().split("\n")
            assert lines[0] == plain[0] + cols and lines[-1] == ""
            rows = [l.split(",") for l in lines[1:] if l]
            # without the flag the file is what it was: the new columns come after all the others
            assert [",".join(r[:-5]) for r in rows] == [l for l in plain[1:] if l], (extra, nb)
            bb, bc = A.bucket_windows(b0, c0, nb)
            want = P.windows_pair(fx, np.concatenate([fy, np.zeros(n - m)]), list(zip(bb.tolist(), bc.tolist())))
            assert [int(r[-5]) for r in rows] == want["count"].tolist()
            for r, w in zip(rows, want):
                f = np.array(P.fit(*[w[k] for k in P.FIELDS]))[[0, 2, 3, 4]]
                f[np.isnan(f)] = np.nan  # the text form keeps no NaN payload
                assert _bits([float(v) for v in r[-4:]]).tolist() == _bits(f).tolist(), (extra, nb, r[0])
    # OTHER shorter than the bucketed range: a runtime error with the library's message
    r = _run(atsc, "-u", "--buckets", 1000, "--pair", tmp_path / "y.bro", tmp_path / "x.bro", code=1)
    assert "window beyond the stream" in r.stderr
