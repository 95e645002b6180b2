"""Windowed moments on the GPU: every window of every case against the NumPy model of the documented merge tree
(tests/moments_model.py) applied to the GPU's own full decode -- all six fields bit for bit, any NaN equal to any NaN,
no tolerance, no window left out.  Every codec and frame-length tier (Noop stores integers and cannot carry NaN or Inf:
those come through Constant records and hand-built IDW records with f64 points); windows inside a tile, across tile and
frame boundaries, at tile multiples, of lengths 0, 1 and 2, overlapping, unsorted, sharing mid tiles; budgets that cut a
window into pieces; a plan reused with other windows; the dev, host, stream and .bro entry points and both command
lines; determinism; validation and malformed payloads; aggregate and moments calls interleaved on one plan."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import moments_model as M

pytestmark = pytest.mark.gpu

LENS = [1, 7, 64, 128, 256, 300, 512, 513, 1024, 4096, 4097, 6500, 8192, 20000, 65536, 131072]
T = M.TILE


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
    """a Constant record of n samples of `value` as it is (NaN, +-Inf, -0.0 included): the library's own 64-bit Constant
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


@pytest.fixture(scope="module")
def mixed(A, ctx):
    """every frame length of LENS under auto at e = 5 / 1 / 0 % and forced fft, polynomial, idw, rle, constant, noop;
    hand-built FFT records with 15 and 16 bins"""
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.uint64)
    modes = [(A.AUTO, True, 0.05), (A.AUTO, True, 0.01), (A.AUTO, True, 0.0), (A.FFT, True, 0.05),
             (A.POLYNOMIAL, True, 0.05), (A.IDW, True, 0.05), (A.RLE, False, 0.0), (A.CONSTANT, False, 0.0),
             (A.NOOP, False, 0.0)]
    recs = b""
    for m, (comp, bounded, me) in enumerate(modes):
        x = H.synth_series(1700 + m, int(off[-1]), block=3000)
        if comp == A.RLE:
            x = np.round(x / 8.0) * 8.0
        r, _, _, _ = ctx.compress_host(x, off, comp, bounded, float(np.float32(me)), 0)
        recs += r
    rng = np.random.default_rng(5)
    for n in (128, 256, 1024, 2048, 4096):
        for k in (15, 16):
            recs += _fft_record(rng, n, k)
    return recs


@pytest.fixture(scope="module")
def grid(A, ctx):
    """a run of 131072-sample FFT frames (the large decoder's grid path)"""
    lens = [131072, 65536, 131072, 131072]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    x = H.synth_series(1808, int(off[-1]), klass=1)
    r, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.01)), 0)
    return r


def _frame_lens(recs):
    return [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in H.parse_bro_body(recs, with_count=False)]


def _windows(lens, total, rng, n_random=100):
    """the whole stream, empty windows, lengths 1 and 2, every frame boundary, tile multiples and their neighbours,
    windows inside one tile, random ones up to 300000 samples -- in an order that is not sorted, overlaps included"""
    w = {(0, total), (0, 0), (total, 0), (total - 1, 1), (0, 1), (0, 2), (total - 2, 2)}
    for s in np.cumsum(lens)[:-1]:
        s = int(s)
        for b in (s - 1, s, s + 1):
            if b >= total:
                continue
            w.add((b, 1))
            w.add((max(b - 5, 0), min(11, total - max(b - 5, 0))))
    for k in rng.integers(0, total // T, 40):
        k = int(k)
        for b, c in ((k * T, T), (k * T, 2 * T), (k * T, 5 * T), (k * T - 1, 2), (k * T + 1, T - 2), (k * T + T - 1, T + 2),
                     (k * T + 100, 1500), (k * T + 7, 2), (k * T, 1), (k * T + T - 2, 2), (k * T + 3, 70 * T)):
            if b >= 0 and b + c <= total:
                w.add((b, c))
    for _ in range(n_random):
        b = int(rng.integers(0, total))
        w.add((b, int(rng.integers(0, min(total - b, 300000) + 1))))
    w = sorted(w)
    return [w[i] for i in rng.permutation(len(w))]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _equal(got, want):
    """all six fields bit for bit; any NaN equals any NaN"""
    if len(got) != len(want) or not np.array_equal(got["count"], want["count"]):
        return False
    for k in M.FIELDS[1:]:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if not np.all((_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))):
            return False
    return True


def _check(full, wins, got, label=""):
    """every window against the model on the full decode"""
    assert len(got) == len(wins), label
    want = M.windows_moments(full, wins)
    for i, (b, c) in enumerate(wins):
        assert _equal(got[i:i + 1], want[i:i + 1]), (label, b, c, got[i], want[i])


def _dev(A, ctx, torch, recs, wins, dp=None):
    own = dp is None
    if own:
        dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    d_out = torch.full((max(len(wins), 1) * 6,), -1, dtype=torch.int64, device="cuda")
    dp.moments_windows(body, [w[0] for w in wins], [w[1] for w in wins], d_out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(A.WINDOW_MOMENTS)[: len(wins)].copy()
    if own:
        dp.close()
    return out


def _host(ctx, recs, wins):
    return ctx.moments_windows_host(recs, [w[0] for w in wins], [w[1] for w in wins])


@pytest.mark.parametrize("which", ["mixed", "grid"])
def test_parity_with_full_decode(A, ctx, torch, mixed, grid, which):
    recs = mixed if which == "mixed" else grid
    full = ctx.decompress_host(recs)
    lens = _frame_lens(recs)
    assert sum(lens) == len(full)
    wins = _windows(lens, len(full), np.random.default_rng(23))
    got = _host(ctx, recs, wins)
    _check(full, wins, got, which)
    assert _equal(_dev(A, ctx, torch, recs, wins), got)


def test_budgets_pieces_and_plan_reuse(A, ctx, torch, mixed):
    """one window in several pieces under the least budget (65536 samples a piece), a middle one and the default; the
    batch around a window, its order and repeated calls never change a bit; one plan serves changing window lists"""
    full = ctx.decompress_host(mixed)
    total = len(full)
    rng = np.random.default_rng(31)
    probe = [(0, total), (5, 2043), (2047, 300000), (131071, 2), (total - 4097, 4097), (4096, 65536 * 3), (10, 0),
             (3 * T, 40 * T)]
    probe += [(int(b), int(rng.integers(1, 300000))) for b in rng.integers(0, total - 300000, 12)]
    alone = _host(ctx, mixed, probe)
    _check(full, probe, alone, "probe")
    others = []
    for _ in range(600):
        c = int(rng.choice([1, 2, 60, 2048, 5000, 40000]))
        others.append((int(rng.integers(0, total - c + 1)), c))
    batch = probe + others
    order = rng.permutation(len(batch))
    shuffled = [batch[i] for i in order]
    got = _host(ctx, mixed, shuffled)
    back = np.empty_like(got)
    back[order] = got
    assert _equal(back[: len(probe)], alone)
    _check(full, others[:150], back[len(probe): len(probe) + 150], "others")
    for b, c in probe[:5]:  # overlapping neighbours shifted by a few samples
        near = [(b, c), (max(b - 3, 0), c), (b, max(c - 7, 0)), (b + 1, max(c - 1, 0))]
        k = probe.index((b, c))
        assert _equal(_host(ctx, mixed, near)[:1], alone[k:k + 1])
    dp = A.DPlan(ctx, mixed)
    try:
        for budget in (1, 1 << 20, 3 << 20):  # 65536, 131072 and 393216 samples a piece: (2047, 300000) in 5, 3 and 2
            ctx.set_aggregate_scratch(budget)
            assert _equal(_host(ctx, mixed, shuffled), got), budget
            assert _equal(_dev(A, ctx, torch, mixed, probe, dp), alone), budget
            assert _equal(_dev(A, ctx, torch, mixed, probe[2:3], dp), alone[2:3]), budget
    finally:
        ctx.set_aggregate_scratch(0)
    # the same plan, other windows, fewer and more than before, and again the first list
    assert _equal(_dev(A, ctx, torch, mixed, probe[:3], dp), alone[:3])
    _check(full, others[:200], _dev(A, ctx, torch, mixed, others[:200], dp), "reuse")
    assert len(_dev(A, ctx, torch, mixed, [], dp)) == 0
    assert _equal(_dev(A, ctx, torch, mixed, probe, dp), alone)
    dp.close()
    assert _equal(_host(ctx, mixed, probe), alone)  # repeated


def test_64_and_66_tiles_in_one_window(A, ctx, torch):
    """64 partials fill one combine group exactly, 65 and 66 need a second pass: windows of 64 and 66 tiles (135168
    samples) and their neighbours, on tile multiples and on odd slots, under the default budget and under the least one,
    whose pieces of 32 tiles cut every one of them"""
    nan = float("nan")
    n = 35 * 4096
    rng = np.random.default_rng(642)
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
    nan, inf = float("nan"), float("inf")
    parts = [(1.0, 3), (nan, 5), (-0.0, 2), (2.5, 4), (nan, 3000), (-7.0, 2), (inf, 3), (1.0, 1), (-inf, 2), (nan, 1),
             (-0.0, 4), (0.0, 1), (3.0, 5000)]
    recs = b"".join(_const_record(A, ctx, v, n) for v, n in parts)
    rng = np.random.default_rng(41)
    holes = rng.normal(0, 10, 700)
    holes[rng.random(700) < 0.2] = nan
    holes[[5, 300]] = inf
    holes[[6, 450]] = -inf
    noop = np.round(rng.normal(0, 1e6, 2500))
    r_noop, _, _, _ = ctx.compress_host(noop, np.array([0, 2500], dtype=np.uint64), A.NOOP, False, 0.0, 0)
    sparse = rng.normal(1e9, 1e-3, 3000)
    sparse[rng.random(3000) < 0.2] = nan
    recs += _idw_record(holes) + r_noop + _idw_record(sparse)
    full = ctx.decompress_host(recs)
    at = np.concatenate([[0], np.cumsum([n for _, n in parts])]).tolist()
    c0 = at[-1]
    want = np.concatenate([np.full(n, v) for v, n in parts])
    assert np.array_equal(full[:c0].view(np.uint64), want.view(np.uint64))
    idw = full[c0:c0 + 700]
    assert np.array_equal(np.isnan(idw), np.isnan(holes)) and np.array_equal(np.isinf(idw), np.isinf(holes))
    assert np.array_equal(full[c0 + 700:c0 + 3200], noop)
    assert np.array_equal(np.isnan(full[c0 + 3200:]), np.isnan(sparse)) and np.isnan(sparse).sum() > 400
    wins = [(0, at[4]), (at[1], 5), (at[1], 1), (at[4], 3000), (at[4] + 10, 100), (at[4] - 1, 3002), (at[6], 4),
            (at[6], 6), (at[8], 2), (at[6], 8), (at[10], 4), (at[10], 5), (at[9], 5), (0, at[-1]), (at[2], 0),
            (at[4] + 2047, 3), (0, len(full)), (c0, 700), (c0 + 7, 290), (c0 + 7, 600), (c0 - 100, 900), (c0 + 10, 1),
            (c0 + 5, 1), (c0 + 5, 2), (c0 + 700, 2500), (c0 + 600, 2700), (c0 + 3200, 3000), (c0 + 3300, 2049),
            (c0 + 3200 + 848, 2048)]
    got = _host(ctx, recs, wins)
    _check(full, wins, got, "nonfinite")
    assert _equal(_dev(A, ctx, torch, recs, wins), got)
    r = dict(zip(wins, got))
    assert int(r[(0, at[4])]["count"]) == 9 and int(r[(at[1], 1)]["count"]) == 0
    for w in ((at[1], 1), (at[4], 3000), (at[2], 0)):  # no sample that counts: count 0 and five NaN
        assert int(r[w]["count"]) == 0 and all(np.isnan(r[w][k]) for k in M.FIELDS[1:]), w
    assert int(r[(at[4] - 1, 3002)]["count"]) == 2 and r[(at[4] - 1, 3002)]["t_mean"] == 1500.5
    assert int(r[(at[6], 4)]["count"]) == 4 and np.isnan(r[(at[6], 4)]["m2"])  # Inf - Inf inside the merges
    assert r[(at[10], 5)]["m2"] == 0.0 and r[(at[10], 5)]["c_tx"] == 0.0 and abs(r[(at[10], 5)]["t_m2"] - 10.0) < 1e-9
    w = r[(c0 + 3200, 3000)]  # 1e9 +- 1e-3 with holes: the spread survives
    ok = ~np.isnan(sparse)
    assert int(w["count"]) == int(ok.sum()) and abs(w["m2"] / w["count"] - np.var(full[c0 + 3200:][ok])) < 1e-8


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
        out = np.full(max(len(wins), 1), 0, dtype=A.WINDOW_MOMENTS)
        out["mean"] = 7.0
        b = np.array([w[0] for w in wins], dtype=np.uint64)
        c = np.array([w[1] for w in wins], dtype=np.uint64)
        rc = lib.atsc_moments_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(wins),
                                      b.ctypes.data_as(p), c.ctypes.data_as(p), C.c_void_p(out.ctypes.data))
        return rc, out

    for wins in ([(3 * n, 1)], [(0, nf * n)], [(0, 10), (3 * n - 1, 2)], [(4 * n - 1, 1), (6 * n, 5)]):
        rc, out = raw(bb, wins)
        assert rc == A.capi.E_FORMAT and np.all(out["mean"] == 7.0), (wins, rc)
    for wins in ([(nf * n - 2, 4)], [(0, 5), (nf * n + 1, 0)], [(2 ** 63, 2 ** 63)]):
        rc, out = raw(gb, wins)
        assert rc == A.capi.E_INVALID and np.all(out["mean"] == 7.0), (wins, rc)
    rc, _ = raw(gb, [])
    assert rc == 0
    e = _host(ctx, recs, [(5, 0), (nf * n, 0)])
    assert np.all(e["count"] == 0) and all(np.all(np.isnan(e[k])) for k in M.FIELDS[1:])
    assert len(_host(ctx, recs, [])) == 0
    # the device call: a window beyond the plan, a misaligned result, a null argument -- nothing enqueued; a malformed
    # payload inside a window sets the plan's status word
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(gb.copy()).to("cuda")
    d_out = torch.full((13,), -1, dtype=torch.int64, device="cuda")
    one = np.array([0], dtype=np.uint64)
    cnt = np.array([nf * n + 1], dtype=np.uint64)

    def dev(h_dp, d_body, b, c, ptr):
        return lib.atsc_moments_windows_dev(ctx._h, h_dp, C.c_void_p(d_body), 1, b.ctypes.data_as(p), c.ctypes.data_as(p),
                                            C.c_void_p(ptr), None)

    assert dev(dp._h, body.data_ptr(), one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    cnt[0] = 10
    assert dev(dp._h, body.data_ptr(), one, cnt, d_out.data_ptr() + 4) == A.capi.E_INVALID
    assert dev(dp._h, body.data_ptr(), one, cnt, 0) == A.capi.E_INVALID
    assert dev(None, body.data_ptr(), one, cnt, d_out.data_ptr()) == A.capi.E_INVALID
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())
    dp.close()


def test_interleaved_with_aggregates(A, ctx, torch, mixed):
    """an aggregate call and a moments call on one plan, one after the other and repeatedly: the aggregate results are
    those of a plan that never saw a moments call, and the moments those of a plan of their own"""
    total = len(ctx.decompress_host(mixed))
    rng = np.random.default_rng(43)
    wa = [(int(b), int(rng.integers(0, 200000))) for b in rng.integers(0, total - 200000, 40)] + [(0, total)]
    wm = [(int(b), int(rng.integers(0, 200000))) for b in rng.integers(0, total - 200000, 55)] + [(7, total - 7)]
    body = torch.from_numpy(np.frombuffer(mixed, dtype=np.uint8).copy()).to("cuda")
    s = torch.cuda.current_stream().cuda_stream

    def agg(dp, wins):
        d = torch.full((len(wins) * 6,), -1, dtype=torch.int64, device="cuda")
        dp.aggregate_windows(body, [w[0] for w in wins], [w[1] for w in wins], d, s)
        return d

    def mom(dp, wins):
        d = torch.full((len(wins) * 6,), -1, dtype=torch.int64, device="cuda")
        dp.moments_windows(body, [w[0] for w in wins], [w[1] for w in wins], d, s)
        return d

    dp0 = A.DPlan(ctx, mixed)
    a_alone = agg(dp0, wa)
    torch.cuda.synchronize()
    a_alone = a_alone.cpu().numpy().tobytes()
    dp0.close()
    m_alone = _dev(A, ctx, torch, mixed, wm)
    dp = A.DPlan(ctx, mixed)
    outs = []
    for _ in range(3):  # enqueued back to back, no synchronisation between the two kinds
        outs.append((agg(dp, wa), mom(dp, wm), mom(dp, wa), agg(dp, wm[:5])))
    torch.cuda.synchronize()
    for a, m, m2, _ in outs:
        assert a.cpu().numpy().tobytes() == a_alone
        assert _equal(m.cpu().numpy().view(A.WINDOW_MOMENTS), m_alone)
    dp.close()
    # the counts of the two records agree window by window
    st = np.frombuffer(a_alone, dtype=A.WINDOW_STATS)
    mm = outs[0][2].cpu().numpy().view(A.WINDOW_MOMENTS)
    assert np.array_equal(st["count"], mm["count"])


def test_entry_points_agree(A, ctx, torch, oracle, golden_dir):
    rng = np.random.default_rng(47)
    for name in ("go_gc_heap_goal_bytes", "memory_used", "uptime"):
        x = H.read_wbro(os.path.join(golden_dir, "wbros", name + ".wbro"))
        for comp, err in ((oracle.AUTO, 3), (oracle.FFT, 1), (oracle.POLYNOMIAL, 5), (oracle.RLE, 0), (oracle.NOOP, 0)):
            bro = oracle.compress_data(x, comp, err)
            full = A.decompress_data(ctx, bro)
            _, frames = H.parse_bro(bro)
            lens = [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in frames]
            wins = _windows(lens, len(full), rng, n_random=15)
            b = [w[0] for w in wins]
            c = [w[1] for w in wins]
            via_bro = A.moments_data_windows(ctx, bro, b, c)
            _check(full, wins, via_bro, name)
            records = bro[9:]  # with the frame-count varint
            assert _equal(ctx.moments_windows_host(records, b, c, has_count=True), via_bro), (name, comp)
            s = A.CompressedStream.from_bytes(ctx, bro)
            assert _equal(s.moments_windows(b, c), via_bro), (name, comp)
            n0, p0 = H.varint_decode(bro, 9)
            assert n0 == len(frames)
            assert _equal(_dev(A, ctx, torch, bro[p0:], wins), via_bro), (name, comp)
    s = A.CompressedStream(ctx)  # a stream without a frame holds only empty windows at 0
    e = s.moments_windows([0, 0], [0, 0])
    assert np.all(e["count"] == 0) and np.all(np.isnan(e["mean"]))
    with pytest.raises(A.AtscError):
        s.moments_windows([0], [1])


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def _rows(path):
    lines = open(path).read().split("\n")
    return lines[0], [l.split(",") for l in lines[1:] if l]


def _fit_bits(rows):
    return [[int(b) for b in _bits([float(v) for v in r[-5:]])] for r in rows]


def _want_bits(A, mom):
    f = A.moments_fit(mom)
    out = []
    for r in f:
        v = np.array([r[k] for k in ("mean", "variance", "stddev", "slope", "intercept")])
        v[np.isnan(v)] = np.nan  # the text form keeps no NaN payload
        out.append([int(b) for b in _bits(v)])
    return out


def test_command_lines(A, ctx, golden_dir, tmp_path):
    from oracle import vsri_oracle as VO

    cols = ",mean,stdvar,stddev,slope,intercept"
    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    for extra, (b0, c0) in (((), (0, len(full))), (("--samples", "100:1500"), (100, 1500))):
        for nb in (60, 1000, len(full) + 1):
            for more in ((), ("--quantiles", "0.5", "--histogram", "0:1000:4")):
                _run(atsc, "-u", "--buckets", nb, *extra, *more, tmp_path / "uptime.bro")
                plain = open(tmp_path / "uptime.agg.csv").read()
                _run(atsc, "-u", "--buckets", nb, "--moments", *extra, *more, tmp_path / "uptime.bro")
                text = open(tmp_path / "uptime.agg.csv").read()
                head, rows = _rows(tmp_path / "uptime.agg.csv")
                assert head.endswith(cols) and head[: -len(cols)] == plain.split("\n")[0]
                # without the flag the file is what it was: the new columns come after all the others
                assert [",".join(r[:-5]) for r in rows] == [l for l in plain.split("\n")[1:] if l], (extra, nb)
                assert text.endswith("\n")
                bb, bc = A.bucket_windows(b0, c0, nb)
                assert [int(r[0]) for r in rows] == bb.tolist()
                mom = A.moments_data_windows(ctx, bro, bb, bc)
                _check(full, list(zip(bb.tolist(), bc.tolist())), mom, "atsc")
                assert _fit_bits(rows) == _want_bits(A, mom), (extra, nb)
    # csv-compressor -u --from --to --step --moments on the reference's cpu_utilization values and times
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
    for t0, t1, step in ((times[0], times[-1], 600), (times[10], times[50], 7), (times[10] + 1, times[50] - 1, 60),
                         (times[0] - 1000, times[3], 100), (times[-1] - 50, times[-1] + 500, 1000)):
        for f in tmp_path.glob("win*"):
            f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        plain = open(tmp_path / "win.agg.csv").read()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "--moments", "-o", tmp_path / "win", tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.agg.csv"]
        head, got = _rows(tmp_path / "win.agg.csv")
        assert head == "timestamp,count,min,max,sum,first,last" + cols
        assert [",".join(r[:-5]) for r in got] == [l for l in plain.split("\n")[1:] if l]
        wb, wc = index.step_windows(int(t0), int(t1), int(step))
        mom = A.moments_data_windows(ctx, cbro, wb, wc)
        _check(all_vals, list(zip(wb.tolist(), wc.tolist())), mom, "csv-compressor")
        assert _fit_bits(got) == _want_bits(A, mom), (t0, t1, step)
