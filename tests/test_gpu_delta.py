"""Windowed deltas on the GPU: every window of every case against the NumPy model of the documented pairs, terms and
summation order (tests/delta_model.py) applied to the GPU's own full decode -- all eight fields bit for bit, any NaN
equal to any NaN, no tolerance, no window left out.  A mixed stream of small-tier records of every codec and one of
frames above 4096 samples; windows at the seams of the kernel's slot-to-lane mapping, across tiles, of lengths 0 .. 3,
overlapping and sharing mid tiles; the least budget, whose pieces of 65536 samples make the carried sample matter; NaN
and +-Inf at a tile's first and last slot and at the carried slot (Noop stores integers and cannot carry NaN or Inf:
those come through hand-built IDW records with f64 points); validation and malformed payloads; aggregate, moments and
delta calls interleaved on one plan; the dev, host, stream and .bro entry points and both command lines."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import delta_model as M

pytestmark = pytest.mark.gpu

T = M.TILE
PIECE = 65536  # samples of a piece of the scratch under the least budget
SMALL = [1, 7, 64, 128, 256, 300, 512, 513, 1024, 2048, 4096]
LARGE = [4097, 6500, 8192, 20000, 65536, 131072]


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


def _idw_record(values):
    """a hand-built IDW record whose points are the samples themselves (f64 points, point step 1, min -Inf, max +Inf):
    every sample decodes to its point, NaN and +-Inf included"""
    n = len(values)
    p = _v(1) + _v(0) + _v(n) + struct.pack("<%dd" % n, *values) + struct.pack("<dd", -np.inf, np.inf) + bytes([1])
    return _rec(n, 2, p)


def _counter(rng, n):
    """an integer counter with restarts: what Noop and RLE store as it is"""
    x = np.cumsum(rng.integers(0, 1000, n)).astype(np.float64)
    for at in rng.integers(1, n, max(n // 700, 1)):
        x[at:] -= x[at] - float(rng.integers(0, 50))
    return x


@pytest.fixture(scope="module")
def mixed(A, ctx):
    """small-tier records, 313215 samples: every frame length of SMALL, seven times over, under forced fft, constant,
    idw, rle and noop"""
    lens = SMALL * 7
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    recs = b""
    rng = np.random.default_rng(3)
    for m, (comp, bounded, me) in enumerate([(A.FFT, True, 0.05), (A.CONSTANT, False, 0.0), (A.IDW, True, 0.05),
                                             (A.RLE, False, 0.0), (A.NOOP, False, 0.0)]):
        x = H.synth_series(2100 + m, int(off[-1]), block=3000)
        if comp == A.RLE:
            x = np.round(x / 8.0) * 8.0
        if comp == A.NOOP:
            x = _counter(rng, int(off[-1]))
        r, _, _, _ = ctx.compress_host(x, off, comp, bounded, float(np.float32(me)), 0)
        recs += r
    return recs


@pytest.fixture(scope="module")
def large(A, ctx):
    """frames above 4096 samples (the large tier), 235397 samples: the pieces of the least budget cut two of them"""
    off = np.concatenate([[0], np.cumsum(LARGE)]).astype(np.uint64)
    x = H.synth_series(2208, int(off[-1]), klass=1)
    r, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.01)), 0)
    return r


@pytest.fixture(scope="module")
def decoded(ctx, mixed, large):
    """the full decodes, computed once"""
    return {"mixed": (mixed, ctx.decompress_host(mixed)), "large": (large, ctx.decompress_host(large))}


def _seam_windows(total):
    """the edges at which the kernel can go wrong: counts 0 .. 3; begins around a tile multiple; the pair that straddles
    a tile; starts and ends at the lane (127/128), k (511/512 of a quarter's lanes: slots 127/128 + 512 q) and quarter
    (511/512, 1023/1024) seams of the slot-to-lane mapping; overlapping windows that share mid tiles; the whole stream"""
    w = [(0, total), (0, 0), (total, 0), (total - 1, 1), (0, 1), (0, 2), (0, 3), (total - 2, 2), (total - 3, 3)]
    for b in (2047, 2048, 2049):
        w += [(b, c) for c in (0, 1, 2, 3, 100, T, 3 * T)]
    w.append((2047, 2))
    for k in (0, 3):
        for s in (127, 128, 129, 511, 512, 513, 639, 640, 1023, 1024, 1025, 1535, 1536, 2046, 2047):
            b = k * T + s
            w += [(b, 1), (b, 2), (b, 3), (b, T), (b, 2 * T + 5), (k * T, s), (k * T, s + 1), (k * T + 5, s),
                  (max(b - 3 * T, 0), b - max(b - 3 * T, 0)), (max(b - 3 * T, 0), b + 1 - max(b - 3 * T, 0))]
    w += [(T + 5, 9 * T), (2 * T + 700, 9 * T), (3 * T, 4 * T), (100, 20 * T)]  # shared mid tiles
    return [(b, c) for b, c in w if b + c <= total]


def _windows(total, rng, n_random=100, longest=120000):
    w = _seam_windows(total)
    for _ in range(n_random):
        b = int(rng.integers(0, total))
        c = int(rng.choice([60, 3000, longest]))
        w.append((b, int(rng.integers(0, min(total - b, c) + 1))))
    return [w[i] for i in rng.permutation(len(w))]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _equal(got, want):
    """the three counts equal, the five doubles bit for bit; any NaN equals any NaN"""
    if len(got) != len(want):
        return False
    for k in M.FIELDS[:3]:
        if not np.array_equal(got[k], want[k]):
            return False
    for k in M.FIELDS[3:]:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if not np.all((_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))):
            return False
    return True


def _check(full, wins, got, label=""):
    """every window against the model on the full decode"""
    assert len(got) == len(wins), label
    want = M.windows_delta(full, wins)
    for i, (b, c) in enumerate(wins):
        assert _equal(got[i:i + 1], want[i:i + 1]), (label, b, c, got[i], want[i])
    return want


def _dev(A, ctx, torch, recs, wins, dp=None):
    own = dp is None
    if own:
        dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    d_out = torch.full((max(len(wins), 1) * 8,), -1, dtype=torch.int64, device="cuda")
    dp.delta_windows(body, [w[0] for w in wins], [w[1] for w in wins], d_out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(A.WINDOW_DELTA)[: len(wins)].copy()
    if own:
        dp.close()
    return out


def _host(ctx, recs, wins):
    return ctx.delta_windows_host(recs, [w[0] for w in wins], [w[1] for w in wins])


@pytest.mark.parametrize("which", ["mixed", "large"])
def test_parity_with_full_decode(A, ctx, torch, decoded, which):
    recs, full = decoded[which]
    assert len(full) == (sum(SMALL) * 35 if which == "mixed" else sum(LARGE))
    wins = _windows(len(full), np.random.default_rng(23))
    got = _host(ctx, recs, wins)
    want = _check(full, wins, got, which)
    assert _equal(_dev(A, ctx, torch, recs, wins), got)
    assert want["rises"].sum() > 1000 and want["falls"].sum() > 1000  # the data moves both ways


@pytest.mark.parametrize("which", ["mixed", "large"])
def test_pieces_and_the_carried_sample(A, ctx, torch, decoded, which):
    """the least budget: pieces of 65536 samples.  A window across two piece boundaries, windows that begin and end at a
    boundary, the pair that straddles it, and ones that stay on one side: the default budget's records bit for bit, by
    the host call and twice on one plan"""
    recs, full = decoded[which]
    total = len(full)
    rng = np.random.default_rng(31)
    wins = [(1000, 200000), (PIECE, 70000), (PIECE, 1), (PIECE, 2), (PIECE - 10, 10), (0, PIECE), (PIECE - 1, 2),
            (PIECE - 1, 1), (PIECE - 2, 2), (PIECE - 1, PIECE + 2), (2 * PIECE - 1, 2), (2 * PIECE - T, 2 * T),
            (2 * PIECE, T), (PIECE + 1, 5), (0, total), (5, 0), (3 * PIECE - 1, 3), (PIECE - T - 1, 2 * T + 2)]
    wins += [(int(b), int(rng.integers(0, 150000))) for b in rng.integers(0, total - 150000, 10)]
    wins += [(int(b), 60) for b in rng.integers(PIECE - 100, PIECE + 100, 10)]
    alone = _host(ctx, recs, wins)
    _check(full, wins, alone, which)
    dp = A.DPlan(ctx, recs)
    try:
        for budget in (1, 1 << 20):  # 65536 and 131072 samples a piece
            ctx.set_aggregate_scratch(budget)
            assert _equal(_host(ctx, recs, wins), alone), budget
            assert _equal(_dev(A, ctx, torch, recs, wins, dp), alone), budget
            assert _equal(_dev(A, ctx, torch, recs, wins[:1], dp), alone[:1]), budget  # the plan's tables reused
            assert _equal(_dev(A, ctx, torch, recs, wins[6:9], dp), alone[6:9]), budget
    finally:
        ctx.set_aggregate_scratch(0)
    assert _equal(_dev(A, ctx, torch, recs, wins, dp), alone)
    assert len(_dev(A, ctx, torch, recs, [], dp)) == 0
    dp.close()


def test_64_and_66_tiles_in_one_window(A, ctx, torch):
    """64 partials fill one combine group exactly, 65 and 66 need a second pass: windows of 64 and 66 tiles (135168
    samples) and their neighbours, on tile multiples and on odd slots, under the default budget and under the least one,
    whose pieces of 32 tiles cut every one of them"""
    nan = float("nan")
    n = 35 * 4096
    rng = np.random.default_rng(643)
    # decoding rounds to the fifth decimal, so the samples are placed on it; a sum of these depends on its order
    x = np.round(rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 7, n), 5)
    x[rng.integers(0, n, 300)] = nan
    recs = b"".join(_idw_record(x[k:k + 4096].tolist()) for k in range(0, n, 4096))
    full = ctx.decompress_host(recs)
    assert np.array_equal(np.isnan(full), np.isnan(x)) and np.array_equal(full[~np.isnan(x)], x[~np.isnan(x)])
    wins = [(2 * T, 64 * T), (2 * T - 1, 64 * T + 2), (T, 66 * T), (2 * T + 1, 66 * T - 1), (2 * T, 64 * T - 1),
            (2 * T + 1, 64 * T), (0, n), (T + 7, 65 * T), (3 * T, 64 * T), (2 * T, 65 * T), (5, 64 * T)]
    try:
        for budget in (0, 1):
            ctx.set_aggregate_scratch(budget)
            got = _host(ctx, recs, wins)
            _check(full, wins, got, "64 tiles, budget %d" % budget)
            assert _equal(_dev(A, ctx, torch, recs, wins), got), budget
    finally:
        ctx.set_aggregate_scratch(0)


def test_non_finite_values(A, ctx, torch):
    """NaN at a tile's last slot, at its first slot, at both, and at slot 65535, the sample carried into the next piece;
    +-Inf next to finite values and next to each other: the counts are exact.  (Under the contract's rules no term is NaN
    -- a rise's b - a and a fall's a - b are positive or +Inf, and a fall's b is never +Inf -- so neither the model nor
    the GPU may return one: _check holds every field to the model's bits.)"""
    nan, inf = float("nan"), float("inf")
    n = 17 * 4096
    rng = np.random.default_rng(41)
    x = np.round(rng.normal(0, 100, n), 2)
    x[rng.random(n) < 0.02] = nan
    x[2040:2060] = np.arange(20.0)
    x[2047] = nan                       # a tile's last slot
    x[3 * T - 5:3 * T + 5] = np.arange(10.0)
    x[3 * T] = nan                      # a tile's first slot
    x[5 * T - 3:5 * T + 3] = [1.0, 2.0, nan, nan, 5.0, 4.0]  # both
    x[PIECE - 4:PIECE + 4] = [1.0, 3.0, 2.0, nan, 7.0, 6.0, 9.0, 9.0]  # the carried sample
    x[2 * T - 2:2 * T + 2] = [1.0, inf, inf, 2.0]            # Inf across a tile boundary, next to each other and to finite
    x[100:108] = [1.0, inf, -inf, -inf, inf, 0.0, -inf, 3.0]
    x[7 * T - 1:7 * T + 2] = [-inf, inf, 5.0]
    x[200:204] = [-0.0, 0.0, -0.0, 1.0]
    recs = b"".join(_idw_record(x[k:k + 4096].tolist()) for k in range(0, n, 4096))
    full = ctx.decompress_host(recs)
    assert np.array_equal(np.isnan(full), np.isnan(x)) and np.array_equal(full[~np.isnan(x)], x[~np.isnan(x)])
    wins = [(0, n), (2040, 20), (2046, 2), (2047, 2), (2046, 3), (2048, 5), (3 * T - 5, 10), (3 * T - 1, 2), (3 * T, 2),
            (3 * T, T), (2 * T, T + 1), (5 * T - 3, 6), (5 * T - 1, 2), (4 * T, 2 * T), (PIECE - 4, 8), (PIECE - 2, 2),
            (PIECE - 1, 2), (PIECE - 1, 3), (PIECE, 4), (PIECE - T, 2 * T), (1000, PIECE), (2 * T - 2, 4), (2 * T - 1, 2),
            (100, 8), (101, 2), (102, 2), (103, 2), (104, 3), (7 * T - 1, 3), (7 * T - 1, 2), (7 * T, 2), (200, 4),
            (200, 3), (0, 3 * T), (T, 8 * T)]
    wins += [(int(b), int(rng.integers(0, 9000))) for b in rng.integers(0, n - 9000, 40)]
    try:
        for budget in (1, 0):
            ctx.set_aggregate_scratch(budget)
            got = _host(ctx, recs, wins)
            want = _check(full, wins, got, "nonfinite")
            assert _equal(_dev(A, ctx, torch, recs, wins), got)
    finally:
        ctx.set_aggregate_scratch(0)
    r = dict(zip(wins, got))
    assert not any(np.isnan(got[k]).any() or np.isnan(want[k]).any() for k in M.FIELDS[3:])
    assert np.isinf(want["up"]).sum() > 2 and np.isinf(want["after_falls"]).sum() > 2
    assert tuple(r[(2040, 20)])[:3] == (17, 17, 0) and r[(2040, 20)]["up"] == 17.0  # 7 -> NaN -> 9 counts no pair
    assert tuple(r[(2046, 2)])[:3] == (0, 0, 0) and tuple(r[(2047, 2)])[:3] == (0, 0, 0)
    assert tuple(r[(3 * T - 1, 2)])[:3] == (0, 0, 0) and tuple(r[(3 * T, 2)])[:3] == (0, 0, 0)
    assert tuple(r[(3 * T - 5, 10)])[:3] == (7, 7, 0)
    assert tuple(r[(5 * T - 3, 6)])[:3] == (2, 1, 1) and r[(5 * T - 3, 6)]["after_falls"] == 4.0
    w = r[(PIECE - 4, 8)]  # 1 3 2 NaN | 7 6 9 9: nothing reaches across the carried NaN
    assert tuple(w)[:3] == (5, 2, 2) and (w["up"], w["down"], w["after_falls"]) == (5.0, 2.0, 8.0)
    assert tuple(r[(PIECE - 1, 2)])[:3] == (0, 0, 0) and tuple(r[(PIECE, 4)])[:3] == (3, 1, 1)
    w = r[(2 * T - 2, 4)]  # 1 Inf | Inf 2
    assert tuple(w)[:3] == (3, 1, 1) and w["up"] == inf and w["down"] == inf and w["after_falls"] == 2.0
    assert tuple(r[(2 * T - 1, 2)])[:3] == (1, 0, 0) and _bits(r[(2 * T - 1, 2)]["up"]) == 0
    w = r[(100, 8)]  # 1 Inf -Inf -Inf Inf 0 -Inf 3
    assert tuple(w)[:3] == (7, 3, 3) and w["up"] == inf and w["down"] == inf and w["after_falls"] == -inf
    assert w["max_rise"] == inf and w["max_fall"] == inf
    assert tuple(r[(200, 3)])[:3] == (2, 0, 0) and all(_bits(r[(200, 3)][k]) == 0 for k in M.FIELDS[3:])
    assert tuple(r[(200, 4)])[:3] == (3, 1, 0) and r[(200, 4)]["max_rise"] == 1.0


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
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 10, 10), (5 * n + 3, 100), (0, 0), (3 * n + 5, 0)]
    _check(good, outside, _host(ctx, bad, outside), "outside")
    lib = A.capi.lib()
    bb = np.frombuffer(bad, dtype=np.uint8)
    gb = np.frombuffer(recs, dtype=np.uint8)
    p = C.POINTER(C.c_uint64)

    def raw(buf, wins):
        out = np.full(max(len(wins), 1), 0, dtype=A.WINDOW_DELTA)
        out["up"] = 7.0
        b = np.array([w[0] for w in wins], dtype=np.uint64)
        c = np.array([w[1] for w in wins], dtype=np.uint64)
        rc = lib.atsc_delta_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(wins),
                                    b.ctypes.data_as(p), c.ctypes.data_as(p), C.c_void_p(out.ctypes.data))
        return rc, out

    for wins in ([(3 * n, 1)], [(0, nf * n)], [(0, 10), (3 * n - 1, 2)], [(4 * n - 1, 1), (6 * n, 5)]):
        rc, out = raw(bb, wins)
        assert rc == A.capi.E_FORMAT and np.all(out["up"] == 7.0), (wins, rc)
    for wins in ([(nf * n - 2, 4)], [(0, 5), (nf * n + 1, 0)], [(2 ** 63, 2 ** 63)]):
        rc, out = raw(gb, wins)
        assert rc == A.capi.E_INVALID and np.all(out["up"] == 7.0), (wins, rc)
    rc, _ = raw(gb, [])
    assert rc == 0
    e = _host(ctx, recs, [(5, 0), (nf * n, 0), (7, 1)])
    assert all(np.all(_bits(e[k]) == 0) for k in M.FIELDS[3:]) and all(np.all(e[k] == 0) for k in M.FIELDS[:3])
    assert len(_host(ctx, recs, [])) == 0
    # the device call: a window beyond the plan, a misaligned result, a null argument -- nothing enqueued
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(gb.copy()).to("cuda")
    d_out = torch.full((17,), -1, dtype=torch.int64, device="cuda")
    one = np.array([0], dtype=np.uint64)
    cnt = np.array([nf * n + 1], dtype=np.uint64)

    def dev(h_dp, d_body, nw, b, c, ptr):
        return lib.atsc_delta_windows_dev(ctx._h, h_dp, C.c_void_p(d_body), nw, b.ctypes.data_as(p), c.ctypes.data_as(p),
                                          C.c_void_p(ptr), None)

    assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    cnt[0] = 10
    assert dev(dp._h, body.data_ptr(), 1, one, cnt, d_out.data_ptr() + 4) == A.capi.E_INVALID
    assert dev(dp._h, body.data_ptr(), 1, one, cnt, 0) == A.capi.E_INVALID
    assert dev(None, body.data_ptr(), 1, one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    assert dev(dp._h, body.data_ptr(), 0, one, cnt, d_out.data_ptr()) == 0  # n_windows == 0
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())
    dp.close()


def test_interleaved_with_aggregates_and_moments(A, ctx, torch, decoded):
    """aggregate, moments and delta calls on one plan, enqueued back to back and repeatedly: each gives what it gives on
    a plan of its own"""
    recs, full = decoded["mixed"]
    total = len(full)
    rng = np.random.default_rng(43)
    wa = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, total - 100000, 30)] + [(0, total)]
    wd = [(int(b), int(rng.integers(0, 100000))) for b in rng.integers(0, total - 100000, 40)] + [(7, total - 7)]
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(method, words, wins):
        d = torch.full((len(wins) * words,), -1, dtype=torch.int64, device="cuda")
        method(body, [w[0] for w in wins], [w[1] for w in wins], d, s)
        return d

    def alone(name, words, wins):
        dp = A.DPlan(ctx, recs)
        d = call(getattr(dp, name), words, wins)
        torch.cuda.synchronize()
        out = d.cpu().numpy().tobytes()
        dp.close()
        return out

    a_alone, m_alone = alone("aggregate_windows", 6, wa), alone("moments_windows", 6, wa)
    d_alone = _dev(A, ctx, torch, recs, wd)
    _check(full, wd, d_alone, "alone")
    dp = A.DPlan(ctx, recs)
    outs = []
    for _ in range(3):
        outs.append((call(dp.aggregate_windows, 6, wa), call(dp.delta_windows, 8, wd), call(dp.moments_windows, 6, wa),
                     call(dp.delta_windows, 8, wa), call(dp.aggregate_windows, 6, wd[:5])))
    torch.cuda.synchronize()
    for a, d, m, _, _ in outs:
        assert a.cpu().numpy().tobytes() == a_alone
        assert m.cpu().numpy().tobytes() == m_alone
        assert _equal(d.cpu().numpy().view(A.WINDOW_DELTA), d_alone)
    dp.close()
    # NaN-free windows: every pair counts
    st = np.frombuffer(a_alone, dtype=A.WINDOW_STATS)
    dd = outs[0][3].cpu().numpy().view(A.WINDOW_DELTA)
    assert not np.isnan(full).any()
    assert np.array_equal(dd["pairs"], np.maximum(st["count"], 1) - 1)


def test_entry_points_agree(A, ctx, torch, oracle, golden_dir):
    rng = np.random.default_rng(47)
    for name in ("go_gc_heap_goal_bytes", "uptime"):
        x = H.read_wbro(os.path.join(golden_dir, "wbros", name + ".wbro"))
        for comp, err in ((oracle.AUTO, 3), (oracle.FFT, 1), (oracle.NOOP, 0)):
            bro = oracle.compress_data(x, comp, err)
            full = A.decompress_data(ctx, bro)
            _, frames = H.parse_bro(bro)
            wins = _windows(len(full), rng, n_random=15, longest=len(full))
            b = [w[0] for w in wins]
            c = [w[1] for w in wins]
            via_bro = A.delta_data_windows(ctx, bro, b, c)
            _check(full, wins, via_bro, name)
            records = bro[9:]  # with the frame-count varint
            assert _equal(ctx.delta_windows_host(records, b, c, has_count=True), via_bro), (name, comp)
            s = A.CompressedStream.from_bytes(ctx, bro)
            assert _equal(s.delta_windows(b, c), via_bro), (name, comp)
            n0, p0 = H.varint_decode(bro, 9)
            assert n0 == len(frames)
            assert _equal(_dev(A, ctx, torch, bro[p0:], wins), via_bro), (name, comp)
    s = A.CompressedStream(ctx)  # a stream without a frame holds only empty windows at 0
    e = s.delta_windows([0, 0], [0, 0])
    assert np.all(e["pairs"] == 0) and np.all(_bits(e["up"]) == 0)
    with pytest.raises(A.AtscError):
        s.delta_windows([0], [1])


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def _rows(path):
    lines = open(path).read().split("\n")
    return lines[0], [l.split(",") for l in lines[1:] if l]


COLS = ",pairs,rises,falls,up,down,increase,variation,max_rise,max_fall"


def _got_cols(rows):
    return [[int(v) for v in r[-9:-6]] + [int(b) for b in _bits([float(v) for v in r[-6:]])] for r in rows]


def _want_cols(A, d):
    f = A.delta_derive(d)
    out = []
    for r, g in zip(d, f):
        v = np.array([r["up"], r["down"], g["increase"], g["variation"], r["max_rise"], r["max_fall"]])
        v[np.isnan(v)] = np.nan  # the text form keeps no NaN payload
        out.append([int(r["pairs"]), int(r["rises"]), int(r["falls"])] + [int(b) for b in _bits(v)])
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
    for extra, (b0, c0), nb, more in (((), (0, len(full)), 60, ()),
                                      (("--samples", "100:1500"), (100, 1500), 1000, ("--moments", "--quantiles", "0.5")),
                                      ((), (0, len(full)), len(full) + 1, ())):
        _run(atsc, "-u", "--buckets", nb, *extra, *more, tmp_path / "uptime.bro")
        plain = open(tmp_path / "uptime.agg.csv").read()
        _run(atsc, "-u", "--buckets", nb, "--deltas", *extra, *more, tmp_path / "uptime.bro")
        text = open(tmp_path / "uptime.agg.csv").read()
        head, rows = _rows(tmp_path / "uptime.agg.csv")
        # without the flag the file is what it was: the new columns come after all the others
        assert head.endswith(COLS) and head[: -len(COLS)] == plain.split("\n")[0]
        assert [",".join(r[:-9]) for r in rows] == [l for l in plain.split("\n")[1:] if l], (extra, nb)
        assert text.endswith("\n")
        bb, bc = A.bucket_windows(b0, c0, nb)
        assert [int(r[0]) for r in rows] == bb.tolist()
        d = A.delta_data_windows(ctx, bro, bb, bc)
        _check(full, list(zip(bb.tolist(), bc.tolist())), d, "atsc")
        assert _got_cols(rows) == _want_cols(A, d), (extra, nb)
    # csv-compressor -u --from --to --step --deltas on the reference's cpu_utilization values and times
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
    for t0, t1, step in ((times[0], times[-1], 600), (times[10] + 1, times[50] - 1, 60)):
        for f in tmp_path.glob("win*"):
            f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        plain = open(tmp_path / "win.agg.csv").read()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "--deltas", "-o", tmp_path / "win", tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.agg.csv"]
        head, got = _rows(tmp_path / "win.agg.csv")
        assert head == "timestamp,count,min,max,sum,first,last" + COLS
        assert [",".join(r[:-9]) for r in got] == [l for l in plain.split("\n")[1:] if l]
        wb, wc = index.step_windows(int(t0), int(t1), int(step))
        d = A.delta_data_windows(ctx, cbro, wb, wc)
        _check(all_vals, list(zip(wb.tolist(), wc.tolist())), d, "csv-compressor")
        assert _got_cols(got) == _want_cols(A, d), (t0, t1, step)
