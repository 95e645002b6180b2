"""Windowed histograms on the GPU: every row equal, integer for integer, to the NumPy model of the contract
(tests/hist_model.py) run on the library's own full decode -- over every codec and frame-length tier, both closed
sides, 1 to 1024 edges, uniform edges, edges drawn from the decoded values and edges with infinite ends; NaN, +-Inf and
signed-zero samples; independence from the batch, the order and the scratch budget; windows of 2^26 samples and 2^20
windows in one call; validation; the dev, host, stream and .bro entry points; both command lines."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import hist_model as M

pytestmark = pytest.mark.gpu

LENS = [1, 7, 64, 128, 256, 300, 512, 513, 1024, 4096, 4097, 6500, 8192, 20000, 65536, 131072]
N_EDGES = [1, 2, 17, 255, 1024]
MODES = [M.LEFT_CLOSED, M.RIGHT_CLOSED]
GARBAGE = 0x5A5A5A5A5A5A5A5A


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
    """a Constant record of n samples of `value` as it is (NaN, +-Inf, -0.0 included)"""
    r, _, _, _ = ctx.compress_host(np.full(n, 1.5), np.array([0, n], dtype=np.uint64), A.CONSTANT, False, 0.0, 0)
    assert r.endswith(struct.pack("<d", 1.5))
    return r[:-8] + struct.pack("<d", value)


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
        x = H.synth_series(700 + m, int(off[-1]), block=3000)
        if comp == A.RLE:
            x = np.round(x / 8.0) * 8.0
        r, _, _, _ = ctx.compress_host(x, off, comp, bounded, float(np.float32(me)), 0)
        recs += r
    rng = np.random.default_rng(3)
    for n in (128, 256, 1024, 2048, 4096):
        for k in (15, 16):
            recs += _fft_record(rng, n, k)
    return recs


@pytest.fixture(scope="module")
def grid(A, ctx):
    """a run of 131072-sample FFT frames (the large decoder's grid path)"""
    lens = [131072, 65536, 131072, 131072]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    x = H.synth_series(808, int(off[-1]), klass=1)
    r, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.01)), 0)
    return r


def _frame_lens(recs):
    return [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in H.parse_bro_body(recs, with_count=False)]


def _windows(lens, total, rng, n_random=120):
    w = {(0, total), (0, 0), (total, 0), (total - 1, 1), (0, 1)}
    for s in np.cumsum(lens)[:-1]:
        s = int(s)
        for b in (s - 1, s, s + 1):
            if b >= total:
                continue
            w.add((b, 1))
            w.add((max(b - 5, 0), min(11, total - max(b - 5, 0))))
    for _ in range(n_random):
        b = int(rng.integers(0, total))
        w.add((b, int(rng.integers(0, min(total - b, 300000) + 1))))
    return sorted(w)


def _edge_sets(A, full, n_edges, rng):
    """uniform edges over the data's range; edges drawn from the decoded values themselves (a sample equal to an edge
    happens); the same with infinite ends"""
    v = np.unique(full[np.isfinite(full)])  # ascending and distinct as values (-0.0 and 0.0 are one)
    assert len(v) > n_edges
    lo, hi = float(v[0]), float(v[-1])
    sets = {"uniform": A.histogram_edges_uniform(lo, hi, n_edges - 1) if n_edges > 1 else np.array([(lo + hi) / 2])}
    drawn = np.sort(rng.choice(v, size=n_edges, replace=False))
    sets["values"] = drawn
    ends = drawn.copy()
    ends[0] = -np.inf
    if n_edges > 1:
        ends[-1] = np.inf
    sets["inf ends"] = ends
    if n_edges == 1:
        sets["+inf"] = np.array([np.inf])
    return sets


def _b(wins):
    return [w[0] for w in wins]


def _c(wins):
    return [w[1] for w in wins]


def _host(ctx, recs, wins, edges, closed=M.LEFT_CLOSED):
    return ctx.histogram_windows_host(recs, _b(wins), _c(wins), edges, closed)


def _dev(A, ctx, torch, recs, wins, edges, closed=M.LEFT_CLOSED):
    """the device call into a result pre-filled with garbage: every row must come back written"""
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    rows = len(edges) + 2
    d_out = torch.full((max(len(wins), 1) * rows,), GARBAGE, dtype=torch.int64, device="cuda")
    dp.histogram_windows(body, _b(wins), _c(wins), edges, d_out, closed, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)[: len(wins) * rows].reshape(len(wins), rows).copy()
    dp.close()
    return out


def _check(full, wins, edges, closed, got, label=""):
    want = M.windows(full, _b(wins), _c(wins), edges, closed)
    assert got.dtype == np.uint64 and got.shape == want.shape, (label, got.shape, want.shape)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero((got != want).any(axis=1))[0])
        raise AssertionError((label, closed, len(edges), wins[i], got[i], want[i]))
    assert np.array_equal(got.sum(axis=1), np.array(_c(wins), dtype=np.uint64)), label


@pytest.mark.parametrize("which", ["mixed", "grid"])
def test_parity_with_full_decode(A, ctx, torch, mixed, grid, which):
    recs = mixed if which == "mixed" else grid
    full = ctx.decompress_host(recs)
    lens = _frame_lens(recs)
    assert sum(lens) == len(full)
    rng = np.random.default_rng(19)
    wins = _windows(lens, len(full), rng)
    on_edge = 0
    for n_edges in N_EDGES:
        for name, edges in _edge_sets(A, full, n_edges, rng).items():
            assert len(edges) == n_edges
            on_edge += int(np.isin(full, edges).sum())
            for closed in MODES:
                got = _host(ctx, recs, wins, edges, closed)
                _check(full, wins, edges, closed, got, (which, name))
                if n_edges in (2, 1024) or name == "values":
                    assert np.array_equal(_dev(A, ctx, torch, recs, wins, edges, closed), got), (which, name, n_edges)
    assert on_edge > 100  # samples equal to an edge were counted


def test_non_finite_values(A, ctx, torch):
    nan, inf = float("nan"), float("inf")
    parts = [(1.0, 3), (nan, 5), (-0.0, 2), (2.5, 4), (nan, 3000), (-7.0, 2), (inf, 3), (1.0, 1), (-inf, 2), (nan, 1),
             (-0.0, 400), (0.0, 1), (inf, 70000), (-inf, 300), (5e-324, 9), (-5e-324, 9)]
    recs = b"".join(_const_record(A, ctx, v, n) for v, n in parts)
    want = np.concatenate([np.full(n, v) for v, n in parts])
    full = ctx.decompress_host(recs)
    assert full.tobytes() == want.tobytes()
    at = np.concatenate([[0], np.cumsum([n for _, n in parts])]).tolist()
    total = at[-1]
    wins = [(0, total), (at[1], 5), (at[2], 2), (at[4], 3000), (at[4] - 1, 3002), (at[6], 3), (at[8], 2), (at[10], 401),
            (at[10] - 1, 2), (at[12], 70000), (at[12] - 5, 70310), (at[14], 18), (at[1], 0), (total, 0)]
    wins += [(a, 1) for a in at[:-1]]
    for edges in ([0.0], [-0.0], [-inf, 0.0, inf], [-inf], [inf], [-inf, inf], [-5e-324, 0.0, 5e-324], [-7.0, 1.0, 2.5]):
        for closed in MODES:
            got = _host(ctx, recs, wins, edges, closed)
            _check(full, wins, edges, closed, got, edges)
            assert np.array_equal(_dev(A, ctx, torch, recs, wins, edges, closed), got), edges
    # -0.0 equals a 0.0 edge; all NaN; +Inf on a +Inf edge
    assert list(_host(ctx, recs, [(at[10], 400)], [0.0], M.LEFT_CLOSED)[0]) == [0, 400, 0]
    assert list(_host(ctx, recs, [(at[10], 400)], [0.0], M.RIGHT_CLOSED)[0]) == [400, 0, 0]
    assert list(_host(ctx, recs, [(at[4], 3000)], [0.0], M.LEFT_CLOSED)[0]) == [0, 0, 3000]
    assert list(_host(ctx, recs, [(at[12], 70000)], [-inf, inf], M.LEFT_CLOSED)[0]) == [0, 0, 70000, 0]
    assert list(_host(ctx, recs, [(at[12], 70000)], [-inf, inf], M.RIGHT_CLOSED)[0]) == [0, 70000, 0, 0]
    assert list(_host(ctx, recs, [(at[13], 300)], [-inf, inf], M.LEFT_CLOSED)[0]) == [0, 300, 0, 0]
    assert list(_host(ctx, recs, [(at[13], 300)], [-inf, inf], M.RIGHT_CLOSED)[0]) == [300, 0, 0, 0]


@pytest.fixture(scope="module")
def gaps(A, ctx):
    """150 Constant records of 4000 samples, each with a value of its own: 600000 samples that cost nothing to decode"""
    n, fl = 600000, 4000
    recs, _, _, _ = ctx.compress_host(np.repeat(np.arange(n // fl, dtype=np.float64), fl), H.frame_offsets(n, fl), A.CONSTANT,
                                      False, 0.0, 0)
    full = ctx.decompress_host(recs)
    assert len(full) == n and len(np.unique(full)) == n // fl
    return recs, full


# Windows that leave gaps.  Under the least budget (runs of covered ranges less than 64 * 2048 = 131072 samples apart,
# cut every 65536 samples): [1000, 6000) and [106000, 206000) lie 100000 apart and share a run of 205000 samples, four
# pieces from sample 1000 on, of which the first ends in the gap; [400000, 403000) begins 194000 behind that run and
# [590000, 600000) 187000 behind that: a run each.  One window lies across the piece boundary at 1000 + 2 * 65536.
GAP_WINS = [(1000, 5000), (106000, 100000), (1000 + 2 * 65536 - 100, 200), (300000, 0), (400000, 3000), (590000, 10000)]


def test_independence(A, ctx, torch, mixed, gaps):
    full = ctx.decompress_host(mixed)
    total = len(full)
    rng = np.random.default_rng(29)
    edges = _edge_sets(A, full, 17, rng)["values"]
    probe = [(0, total), (5, 2043), (2047, 300000), (131071, 2), (total - 4097, 4097), (10, 257), (99, 16385), (3, 0),
             (200000, 131072), (total, 0)]
    probe += [(int(b), int(c)) for b, c in zip(rng.integers(0, total - 40000, 12), rng.integers(1, 40000, 12))]
    alone = np.array([_host(ctx, mixed, [w], edges)[0] for w in probe])
    _check(full, probe, edges, M.LEFT_CLOSED, alone, "alone")
    others = []
    for _ in range(600):
        c = int(rng.choice([1, 60, 300, 2048, 9000, 40000]))
        others.append((int(rng.integers(0, total - c + 1)), c))
    batch = probe + others + probe[:8] + [(b + 1, max(c - 1, 0)) for b, c in probe[:8]]  # duplicates, overlaps
    order = rng.permutation(len(batch))
    shuffled = [batch[i] for i in order]
    got = _host(ctx, mixed, shuffled, edges)
    _check(full, shuffled, edges, M.LEFT_CLOSED, got, "shuffled")
    back = np.empty_like(got)
    back[order] = got
    assert np.array_equal(back[: len(probe)], alone)
    assert np.array_equal(back[len(probe) + len(others):][:8], alone[:8])
    # the budget: the least (pieces of 65536 samples, spill slots across the 131072-sample frames), and one that cuts
    # the 131072-sample frames at other places
    for budget in (1, (100000 + 2 * 131072) * 8):
        ctx.set_aggregate_scratch(budget)
        try:
            small = _host(ctx, mixed, shuffled, edges)
            small_dev = _dev(A, ctx, torch, mixed, probe, edges)
            small_right = _host(ctx, mixed, probe, edges, M.RIGHT_CLOSED)
        finally:
            ctx.set_aggregate_scratch(0)
        assert np.array_equal(small, got), budget
        assert np.array_equal(small_dev, alone), budget
        _check(full, probe, edges, M.RIGHT_CLOSED, small_right, budget)
    assert np.array_equal(_host(ctx, mixed, probe, edges), alone)  # repeated
    # the least budget over windows that leave gaps (GAP_WINS): runs of pieces, a piece that ends between two windows
    recs, full = gaps
    edges = np.array([2.0, 26.5, 33.0, 100.0, 148.0])
    whole = _host(ctx, recs, GAP_WINS, edges)
    _check(full, GAP_WINS, edges, M.LEFT_CLOSED, whole, "gaps")
    ctx.set_aggregate_scratch(1)
    try:
        small = _host(ctx, recs, GAP_WINS, edges)
        small_dev = _dev(A, ctx, torch, recs, GAP_WINS, edges)
    finally:
        ctx.set_aggregate_scratch(0)
    assert np.array_equal(small, whole) and np.array_equal(small_dev, whole)


def test_validation(A, ctx, torch):
    n, nf = 256, 8
    x = H.synth_series(909, n * nf, klass=2)
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.05)), 0)
    good = ctx.decompress_host(recs)
    lib = A.capi.lib()
    gb = np.frombuffer(recs, dtype=np.uint8)
    p64 = C.POINTER(C.c_uint64)

    def raw(wins, edges, closed=0, ne=None, null_edges=False):
        e = np.ascontiguousarray(edges, dtype=np.float64)
        ne = len(e) if ne is None else ne
        out = np.full(max(len(wins), 1) * (max(len(e), ne if ne < 5000 else 0) + 2), GARBAGE, dtype=np.uint64)
        b = np.array(_b(wins), dtype=np.uint64)
        c = np.array(_c(wins), dtype=np.uint64)
        rc = lib.atsc_histogram_windows(ctx._h, gb.ctypes.data_as(C.POINTER(C.c_uint8)), len(gb), 0, len(wins),
                                        b.ctypes.data_as(p64), c.ctypes.data_as(p64), ne,
                                        None if null_edges else e.ctypes.data_as(C.POINTER(C.c_double)), closed,
                                        out.ctypes.data_as(p64))
        return rc, out

    ok = [(0, 10), (300, 600)]
    e2 = [-1.0, 1.0]
    bad = [([(nf * n - 2, 4)], e2, 0, None), ([(0, 5), (nf * n + 1, 0)], e2, 0, None), ([(2 ** 63, 2 ** 63)], e2, 0, None),
           (ok, e2, 0, 0), (ok, np.arange(1025.0), 0, None), (ok, e2, 0, 2 ** 32 - 1), (ok, [0.0, np.nan], 0, None),
           (ok, [np.nan], 0, None), (ok, [1.0, 1.0], 0, None), (ok, [0.0, -0.0], 0, None), (ok, [-0.0, 0.0], 0, None),
           (ok, [2.0, 1.0], 0, None), (ok, [0.0, 1.0, 0.5], 0, None), (ok, [np.inf, np.inf], 0, None),
           (ok, e2, 2, None), (ok, e2, -1, None)]
    for wins, edges, closed, ne in bad:
        rc, out = raw(wins, edges, closed, ne)
        assert rc == A.capi.E_INVALID and np.all(out == GARBAGE), (wins, list(edges)[:4], closed, ne, rc)
    rc, out = raw(ok, e2, null_edges=True)
    assert rc == A.capi.E_INVALID and np.all(out == GARBAGE)
    rc, out = raw(ok, [2.0, 1.0])
    assert rc == A.capi.E_INVALID and b"ascending" in lib.atsc_ctx_last_error(ctx._h)
    rc, out = raw([], e2)
    assert rc == 0 and np.all(out == GARBAGE)
    rc, out = raw(ok, np.arange(1024.0))
    assert rc == 0
    _check(good, ok, np.arange(1024.0), 0, out.reshape(2, 1026), "1024 edges")
    rc, out = raw(ok, [-np.inf, np.inf], 1)
    assert rc == 0
    _check(good, ok, [-np.inf, np.inf], 1, out.reshape(2, 4), "inf edges")
    # the dev call validates the same way and writes nothing
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(gb.copy()).to("cuda")
    d_out = torch.full((64,), GARBAGE, dtype=torch.int64, device="cuda")
    for wins, edges, closed in (([(nf * n, 1)], e2, 0), (ok, [1.0, 1.0], 0), (ok, [np.nan], 0), (ok, e2, 9), (ok, [], 0)):
        with pytest.raises(A.AtscError) as e:
            dp.histogram_windows(body, _b(wins), _c(wins), edges, d_out, closed)
        assert e.value.rc == A.capi.E_INVALID
    b = np.array(_b(ok), dtype=np.uint64)
    c = np.array(_c(ok), dtype=np.uint64)
    ed = np.array(e2)
    pe = ed.ctypes.data_as(C.POINTER(C.c_double))
    args = (ctx._h, dp._h, C.c_void_p(body.data_ptr()), 2, b.ctypes.data_as(p64), c.ctypes.data_as(p64), 2, pe, 0)
    assert lib.atsc_histogram_windows_dev(*args, C.c_void_p(d_out.data_ptr() + 4), None) == A.capi.E_INVALID  # alignment
    assert lib.atsc_histogram_windows_dev(*args, None, None) == A.capi.E_INVALID
    assert lib.atsc_histogram_windows_dev(*args[:7], None, 0, C.c_void_p(d_out.data_ptr()), None) == A.capi.E_INVALID
    torch.cuda.synchronize()
    assert bool((d_out == GARBAGE).all())
    assert lib.atsc_histogram_windows_dev(*args, C.c_void_p(d_out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    _check(good, ok, e2, 0, d_out.cpu().numpy().view(np.uint64)[:8].reshape(2, 4), "dev")
    assert bool((d_out[8:] == GARBAGE).all())
    # a malformed payload inside a window: the status word in the dev call, ATSC_E_FORMAT with nothing written in the
    # host call; outside every window: not looked at
    frames = H.parse_bro_body(recs, with_count=False)
    pos = sum(len(_rec(f[1], f[2], f[3])) for f in frames[:3])
    rec3 = _rec(frames[3][1], frames[3][2], frames[3][3])
    pay = pos + len(rec3) - len(frames[3][3])
    assert recs[pay] == 15 and recs[pay + 1] < 200
    broken = bytearray(recs)
    broken[pay + 1] = 250
    broken = bytes(broken)
    bb = np.frombuffer(broken, dtype=np.uint8)
    out = np.full(4, GARBAGE, dtype=np.uint64)
    one, cnt = np.array([3 * n], dtype=np.uint64), np.array([1], dtype=np.uint64)
    rc = lib.atsc_histogram_windows(ctx._h, bb.ctypes.data_as(C.POINTER(C.c_uint8)), len(bb), 0, 1, one.ctypes.data_as(p64),
                                    cnt.ctypes.data_as(p64), 2, pe, 0, out.ctypes.data_as(p64))
    assert rc == A.capi.E_FORMAT and np.all(out == GARBAGE)
    outside = [(0, 3 * n), (4 * n, 4 * n), (0, 0)]
    _check(good, outside, e2, 0, _host(ctx, broken, outside, e2), "outside")
    dpb = A.DPlan(ctx, broken)
    bbody = torch.from_numpy(bb.copy()).to("cuda")
    dpb.histogram_windows(bbody, _b(outside), _c(outside), e2, d_out)
    torch.cuda.synchronize()
    _check(good, outside, e2, 0, d_out.cpu().numpy().view(np.uint64)[:12].reshape(3, 4), "dev outside")
    dpb.close()
    dp.close()
    # empty windows only, and none
    z = ctx.histogram_windows_host(recs, [5, nf * n], [0, 0], e2)
    assert z.shape == (2, 4) and not z.any()
    assert ctx.histogram_windows_host(recs, [], [], e2).shape == (0, 4)
    assert not _dev(A, ctx, torch, recs, [(5, 0), (nf * n, 0)], e2).any()


def test_malformed_payload_is_seen_only_inside_a_window(A, ctx, torch):
    """a malformed payload inside a window sets the plan's status word in the dev call; the host call, which is the dev
    call on a plan of the touched records followed by a read of that word, reports it as ATSC_E_FORMAT.
    The status word has no accessor in the C ABI or the Python surface (as for the window decode, the aggregates and
    the quantiles), so that read is the only way to see it: the word itself is checked through the host call, and the
    dev call on the whole broken stream is checked to return ATSC_OK, to finish, and to give the windows that do not
    touch the bad frame their right rows."""
    n, nf = 256, 4
    x = H.synth_series(911, n * nf, klass=2)
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.05)), 0)
    frames = H.parse_bro_body(recs, with_count=False)
    pos = sum(len(_rec(f[1], f[2], f[3])) for f in frames[:2])
    pay = pos + len(_rec(frames[2][1], frames[2][2], frames[2][3])) - len(frames[2][3])
    assert recs[pay] == 15 and recs[pay + 1] < 200
    broken = bytearray(recs)
    broken[pay + 1] = 250
    broken = bytes(broken)
    e2 = [-1.0, 1.0]
    for wins, fails in (([(0, 2 * n)], False), ([(3 * n, n)], False), ([(2 * n + 7, 1)], True), ([(0, 4 * n)], True),
                        ([(0, n), (2 * n - 1, 2)], True)):
        if fails:
            with pytest.raises(A.AtscError) as e:
                _host(ctx, broken, wins, e2)
            assert e.value.rc == A.capi.E_FORMAT, wins
        else:
            _check(ctx.decompress_host(recs), wins, e2, 0, _host(ctx, broken, wins, e2), wins)
    # the dev call with a window inside the bad frame: enqueued and finished; the other windows' rows are right
    wins = [(0, 2 * n), (2 * n + 7, 1), (3 * n, n), (0, n), (2 * n - 1, 2)]
    got = _dev(A, ctx, torch, broken, wins, e2)
    good = ctx.decompress_host(recs)
    clean = [0, 2, 3]
    _check(good, [wins[i] for i in clean], e2, 0, got[clean], "dev, beside the bad frame")
    assert not (got == GARBAGE).any()  # every row was written, the bad frame's windows included


def test_entry_points_agree(A, ctx, torch, oracle, golden_dir):
    rng = np.random.default_rng(37)
    for name in ("go_gc_heap_goal_bytes", "memory_used", "uptime"):
        x = H.read_wbro(os.path.join(golden_dir, "wbros", name + ".wbro"))
        for comp, err in ((oracle.AUTO, 3), (oracle.FFT, 1), (oracle.RLE, 0), (oracle.NOOP, 0)):
            bro = oracle.compress_data(x, comp, err)
            full = A.decompress_data(ctx, bro)
            _, frames = H.parse_bro(bro)
            lens = [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in frames]
            wins = _windows(lens, len(full), rng, n_random=20)
            b, c = _b(wins), _c(wins)
            edges = _edge_sets(A, full, 17, rng)["values"] if len(np.unique(full)) > 17 else np.unique(full)[:1]
            via_bro = A.histogram_data_windows(ctx, bro, b, c, edges, A.HIST_RIGHT_CLOSED)
            _check(full, wins, edges, M.RIGHT_CLOSED, via_bro, name)
            records = bro[9:]  # with the frame-count varint
            assert np.array_equal(ctx.histogram_windows_host(records, b, c, edges, A.HIST_RIGHT_CLOSED, has_count=True), via_bro)
            s = A.CompressedStream.from_bytes(ctx, bro)
            assert np.array_equal(s.histogram_windows(b, c, edges, A.HIST_RIGHT_CLOSED), via_bro), (name, comp)
            n0, p0 = H.varint_decode(bro, 9)
            assert np.array_equal(_dev(A, ctx, torch, bro[p0:], wins, edges, M.RIGHT_CLOSED), via_bro), (name, comp)
    # a stream under construction, and one without a frame
    s = A.CompressedStream(ctx)
    z = s.histogram_windows([0, 0], [0, 0], [0.0, 1.0])
    assert z.shape == (2, 4) and not z.any()
    with pytest.raises(A.AtscError):
        s.histogram_windows([0], [1], [0.0, 1.0])
    x = H.synth_series(41, 5000, klass=2)
    s.compress_chunk_with(x[:3000], A.FFT)
    s.compress_chunk_with(x[3000:], A.NOOP)
    full = s.decompress()
    wins = [(0, 5000), (2990, 20), (3000, 0), (4999, 1)]
    edges = A.histogram_edges_uniform(float(full.min()), float(full.max()), 16)
    _check(full, wins, edges, M.LEFT_CLOSED, s.histogram_windows(_b(wins), _c(wins), edges), "stream")
    with pytest.raises(A.AtscError) as e:
        s.histogram_windows(_b(wins), _c(wins), [1.0, 1.0])
    assert e.value.rc == A.capi.E_INVALID


def test_second_call_while_the_first_is_in_flight(A, ctx, torch, grid):
    full = ctx.decompress_host(grid)
    total = len(full)
    rng = np.random.default_rng(43)
    dp = A.DPlan(ctx, grid)
    body = torch.from_numpy(np.frombuffer(grid, dtype=np.uint8).copy()).to("cuda")
    calls = []
    for k in range(4):
        wins = [(0, total)] + [(int(b), int(c)) for b, c in zip(rng.integers(0, total - 70000, 40), rng.integers(0, 70000, 40))]
        edges = _edge_sets(A, full, [17, 255, 3, 1024][k], rng)["values"]
        d_out = torch.full((len(wins) * (len(edges) + 2),), GARBAGE, dtype=torch.int64, device="cuda")
        calls.append((wins, edges, k & 1, d_out))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for k, (wins, edges, closed, d_out) in enumerate(calls):  # no wait in between; two streams in turn
        dp.histogram_windows(body, _b(wins), _c(wins), edges, d_out, closed, streams[k & 1].cuda_stream)
    torch.cuda.synchronize()
    for wins, edges, closed, d_out in calls:
        got = d_out.cpu().numpy().view(np.uint64).reshape(len(wins), len(edges) + 2)
        _check(full, wins, edges, closed, got, "in flight")
    dp.close()


def test_scale_long_window_and_many_windows(A, ctx, torch):
    n = (1 << 26) + 12345
    x = H.synth_series(515, n, block=65536)
    bro = A.compress_data(ctx, x, A.AUTO, 3)
    del x
    full = A.decompress_data(ctx, bro)
    assert len(full) == n
    rng = np.random.default_rng(47)
    e17 = _edge_sets(A, full[: 1 << 22], 17, rng)["values"]
    e1024 = A.histogram_edges_uniform(float(np.nanmin(full)), float(np.nanmax(full)), 1023)
    # one window over everything, and long overlapping ones, under a budget that forces many pieces
    long_wins = [(0, n), (12345, 1 << 26), (1 << 25, (1 << 25) + 777), (5, 1 << 20), (n - 3, 3), (n, 0)]
    for edges, closed in ((e17, M.LEFT_CLOSED), (e1024, M.RIGHT_CLOSED)):
        ctx.set_aggregate_scratch(64 << 20)
        try:
            small = A.histogram_data_windows(ctx, bro, _b(long_wins), _c(long_wins), edges, closed)
        finally:
            ctx.set_aggregate_scratch(0)
        assert n > 8 * ((64 << 20) // 8)  # at least 8 pieces under the budget
        _check(full, long_wins, edges, closed, small, "long, small budget")
        assert np.array_equal(A.histogram_data_windows(ctx, bro, _b(long_wins), _c(long_wins), edges, closed), small)
    # 2^20 windows of 64 samples in one call
    bb, bc = A.bucket_windows(0, 1 << 26, 64)
    assert len(bb) == 1 << 20
    want = M.windows(full, bb, bc, e17, M.LEFT_CLOSED)
    got = A.histogram_data_windows(ctx, bro, bb, bc, e17, M.LEFT_CLOSED)
    assert np.array_equal(got, want)
    assert np.array_equal(got.sum(axis=1), bc)
    ctx.set_aggregate_scratch(64 << 20)
    try:
        assert np.array_equal(A.histogram_data_windows(ctx, bro, bb, bc, e17, M.LEFT_CLOSED), want)
    finally:
        ctx.set_aggregate_scratch(0)
    # the same through the dev call into garbage, with empty windows in between
    sel = slice(0, 1 << 18)
    wins = list(zip(bb[sel].tolist(), bc[sel].tolist()))
    wins[5::1000] = [(w[0], 0) for w in wins[5::1000]]
    n0, p0 = H.varint_decode(bro, 9)
    got = _dev(A, ctx, torch, bro[p0:], wins, e17, M.RIGHT_CLOSED)
    _check(full, wins, e17, M.RIGHT_CLOSED, got, "2^18 dev")


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def _rows(path):
    lines = open(path).read().split("\n")
    return lines[0], [l.split(",") for l in lines[1:] if l]


def test_command_lines(A, ctx, golden_dir, tmp_path):
    from oracle import vsri_oracle as VO

    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    lo, hi = float(full.min()), float(full.max())
    v = np.unique(full)
    explicit = [repr(float(t)) for t in v[:: max(1, len(v) // 6)][:7]]
    specs = [(",".join(explicit), np.array([float(t) for t in explicit])),
             ("%r:%r:12" % (lo, hi), A.histogram_edges_uniform(lo, hi, 12)),
             ("-inf,%r,inf" % ((lo + hi) / 2), np.array([-np.inf, (lo + hi) / 2, np.inf]))]
    qnames = ["0.5", "0.99"]
    for nb in (60, 1000):
        _run(atsc, "-u", "--buckets", nb, tmp_path / "uptime.bro")
        base_bytes = (tmp_path / "uptime.agg.csv").read_bytes()
        base_head, base_rows = _rows(tmp_path / "uptime.agg.csv")
        _run(atsc, "-u", "--buckets", nb, "--quantiles", ",".join(qnames), tmp_path / "uptime.bro")
        q_bytes = (tmp_path / "uptime.agg.csv").read_bytes()
        q_head, q_rows = _rows(tmp_path / "uptime.agg.csv")
        bb, bc = A.bucket_windows(0, len(full), nb)
        for spec, edges in specs:
            for closed, cname in ((M.LEFT_CLOSED, None), (M.RIGHT_CLOSED, "right"), (M.LEFT_CLOSED, "left")):
                extra = ("--histogram-closed", cname) if cname else ()
                want = M.windows(full, bb, bc, edges, closed)
                cols = ",".join(["h%d" % k for k in range(len(edges) + 1)] + ["hnan"])
                _run(atsc, "-u", "--buckets", nb, "--histogram=" + spec, *extra, tmp_path / "uptime.bro")
                head, rows = _rows(tmp_path / "uptime.agg.csv")
                assert head == base_head + "," + cols
                assert [r[:7] for r in rows] == base_rows
                assert np.array_equal(np.array([[int(t) for t in r[7:]] for r in rows], dtype=np.uint64), want), (nb, spec)
                _run(atsc, "-u", "--buckets", nb, "--quantiles", ",".join(qnames), "--histogram=" + spec, *extra,
                     tmp_path / "uptime.bro")
                head, rows = _rows(tmp_path / "uptime.agg.csv")
                assert head == q_head + "," + cols
                assert [r[:9] for r in rows] == q_rows
                assert np.array_equal(np.array([[int(t) for t in r[9:]] for r in rows], dtype=np.uint64), want), (nb, spec)
        # without --histogram the file is what it was
        _run(atsc, "-u", "--buckets", nb, tmp_path / "uptime.bro")
        assert (tmp_path / "uptime.agg.csv").read_bytes() == base_bytes
        _run(atsc, "-u", "--buckets", nb, "--quantiles", ",".join(qnames), tmp_path / "uptime.bro")
        assert (tmp_path / "uptime.agg.csv").read_bytes() == q_bytes
    # csv-compressor -u --from --to --step --histogram
    lines = open(os.path.join(golden_dir, "csv", "cpu_utilization.csv")).read().split("\n")[1:]
    rows = [l.split(",") for l in lines if l]
    ts = [int(t) * 1000 for t, _ in rows]
    vals = [float(v) for _, v in rows]
    m = tmp_path / "cpu.csv"
    m.write_text(VO.samples_to_csv_text(ts, vals))
    _run(csvc, "--output-vsri", "--compressor", "fft", "-e", "3", m)
    _run(csvc, "-u", "-o", tmp_path / "all", tmp_path / "cpu.bro")
    all_rows = [r for r in (tmp_path / "all.csv").read_text().split("\n")[1:] if r]
    times = np.array([int(r.split(",")[0]) for r in all_rows])
    cfull = A.decompress_data(ctx, (tmp_path / "cpu.bro").read_bytes())
    index = A.Vsri.load(str(tmp_path / "cpu.vsri"))
    clo, chi = float(cfull.min()), float(cfull.max())
    cedges = A.histogram_edges_uniform(clo, chi, 8)
    for t0, t1, step in ((times[0], times[-1], 600), (times[10], times[50], 7)):
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "-o", tmp_path / "base", tmp_path / "cpu.bro")
        base_bytes = (tmp_path / "base.agg.csv").read_bytes()
        base_head, base_rows = _rows(tmp_path / "base.agg.csv")
        wb, wc = index.step_windows(int(t0), int(t1), int(step))
        for closed, cname in ((M.LEFT_CLOSED, "left"), (M.RIGHT_CLOSED, "right")):
            want = M.windows(cfull, wb, wc, cedges, closed)
            cols = ",".join(["h%d" % k for k in range(len(cedges) + 1)] + ["hnan"])
            _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "--histogram", "%r:%r:8" % (clo, chi),
                 "--histogram-closed", cname, "-o", tmp_path / "win", tmp_path / "cpu.bro")
            assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.agg.csv"]
            head, got = _rows(tmp_path / "win.agg.csv")
            assert head == base_head + "," + cols
            assert [r[:7] for r in got] == base_rows
            assert np.array_equal(np.array([[int(t) for t in r[7:]] for r in got], dtype=np.uint64).reshape(want.shape), want)
            _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "--quantiles", "0.5,0.95", "--histogram",
                 "%r:%r:8" % (clo, chi), "--histogram-closed", cname, "-o", tmp_path / "win", tmp_path / "cpu.bro")
            head, got = _rows(tmp_path / "win.agg.csv")
            assert head == base_head + ",q0.5,q0.95," + cols
            assert [r[:7] for r in got] == base_rows
            assert np.array_equal(np.array([[int(t) for t in r[9:]] for r in got], dtype=np.uint64).reshape(want.shape), want)
            for f in tmp_path.glob("win*"):
                f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "-o", tmp_path / "again", tmp_path / "cpu.bro")
        assert (tmp_path / "again.agg.csv").read_bytes() == base_bytes
