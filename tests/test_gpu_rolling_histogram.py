"""Windowed rolling histograms on the GPU: every counter of every row of every case against the NumPy model of the
contract (tests/rolling_histogram_model.py) applied to the GPU's own full decode, exactly.  The streams are the rolling
quantile suite's: the main stream (every frame-length tier below the large one under every codec, one large frame,
Constant records of NaN, +-Inf and zeros of both signs), a Noop stream of 200000 integers, an integer counter with NaN
holes, and an RLE stream of multiples of 8 whose samples sit on the edges and fill a whole wavefront with one bin.  The
widths and strides stand either side of the wavefront, of the stride at which a trip holds one position (64), and of
stride == width where the windows stop overlapping; the ranges hold B - 1 .. 2 B + 1 positions at each clamp of the rule
that sizes a task.  Against atsc_histogram_windows_dev on the listed windows; pieces under the least budget; one plan
shared with a rolling and a windowed histogram call; the host, device, stream and .bro forms; errors that leave the
result untouched; a malformed payload; both command lines."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import rolling_histogram_model as M
from tests import rolling_model as RM
from tests.test_gpu_rolling import CONSTANTS, LENS, _const_record, _fft_record, _rec

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 63, 64, 65, 127, 128, 129, 300, 4096, 70001]
LONG = 200000
SENT = 0x5A5A5A5A5A5A5A5A
LEFT, RIGHT = M.LEFT_CLOSED, M.RIGHT_CLOSED


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


@pytest.fixture(scope="module")
def main(A, ctx):
    """-> (records, full decode, first sample of the Constant records), built as the rolling suite's"""
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.uint64)
    modes = [(A.AUTO, True, 0.05), (A.AUTO, True, 0.01), (A.AUTO, True, 0.0), (A.FFT, True, 0.05),
             (A.POLYNOMIAL, True, 0.05), (A.IDW, True, 0.05), (A.RLE, False, 0.0), (A.CONSTANT, False, 0.0),
             (A.NOOP, False, 0.0)]
    recs = b""
    for m, (comp, bounded, me) in enumerate(modes):
        v = H.synth_series(3100 + m, int(off[-1]), block=3000)
        if comp == A.RLE:
            v = np.round(v / 8.0) * 8.0
        recs += ctx.compress_host(v, off, comp, bounded, float(np.float32(me)), 0)[0]
    rng = np.random.default_rng(17)
    for n in (128, 256, 1024, 2048, 4096):
        for k in (15, 16):
            recs += _fft_record(rng, n, k)
    recs += ctx.compress_host(H.synth_series(3150, 8192, klass=1), np.array([0, 8192], dtype=np.uint64), A.FFT, True,
                              float(np.float32(0.01)), 0)[0]
    at = len(ctx.decompress_host(recs))
    for value, n in CONSTANTS:
        recs += _const_record(A, ctx, value, n)
    recs += ctx.compress_host(H.synth_series(3160, 9000, block=2000), H.frame_offsets(9000, 4096), A.AUTO, True,
                              float(np.float32(0.05)), 0)[0]
    full = ctx.decompress_host(recs)
    assert 40000 <= len(full) <= 200000 and np.isinf(full).any() and np.isnan(full).any()
    return recs, full, at


def _noop_records(A, ctx, x):
    """Noop frames of 4096: cheap to build and to decode; Noop stores 64-bit integers, so x holds integers"""
    return ctx.compress_host(x, H.frame_offsets(len(x), 4096), A.NOOP, False, 0.0, 0)[0]


@pytest.fixture(scope="module")
def long(A, ctx):
    """200000 integers of mixed magnitude, both signs, in Noop frames, no NaN"""
    rng = np.random.default_rng(23)
    x = np.round(rng.normal(0, 1, LONG) * 10.0 ** rng.integers(0, 12, LONG))
    recs = _noop_records(A, ctx, x)
    full = ctx.decompress_host(recs)
    assert np.array_equal(full, x)
    return recs, full


@pytest.fixture(scope="module")
def counter(A, ctx):
    """an integer counter with resets, stored as Noop, with NaN holes (Constant records of NaN between the Noop frames)"""
    rng = np.random.default_rng(29)
    n = 30000
    x = np.cumsum(rng.integers(0, 51, n).astype(np.float64)) + 1000.0
    for r in np.flatnonzero(rng.random(n) < 0.003):
        x[r:] -= x[r] - float(rng.integers(0, 20))
    recs, want = b"", []
    for seg, hole in ((x[:9000], 1), (x[9000:9001], 2), (x[9001:21000], 3), (x[21000:21005], 70), (x[21005:], 0)):
        recs += _noop_records(A, ctx, seg) + (_const_record(A, ctx, np.nan, hole) if hole else b"")
        want += [seg, np.full(hole, np.nan)]
    full = ctx.decompress_host(recs)
    assert np.array_equal(full, np.concatenate(want), equal_nan=True)
    return recs, full


@pytest.fixture(scope="module")
def ties(A, ctx):
    """values rounded to multiples of 8 under RLE: the samples sit on the edges, and a run fills a wavefront with one bin"""
    x = np.round(H.synth_series(3180, 30000, block=2500) / 8.0) * 8.0
    recs = ctx.compress_host(x, H.frame_offsets(len(x), 1024), A.RLE, False, 0.0, 0)[0]
    full = ctx.decompress_host(recs)
    assert len(full) == len(x) and len(np.unique(full[:4096])) < 1024
    return recs, full


def _edges(full, n, zero=False, inf=False):
    """n strictly ascending edges, most of them samples of the stream (its quantiles by the nearest sample), where they
    run out integers above the largest; zero: 0.0 among them; inf: the first is -Inf and the last +Inf"""
    fin = full[np.isfinite(full)]
    e = np.unique(np.quantile(fin, np.linspace(0.02, 0.98, n), method="nearest") + 0.0)  # (+ 0.0: no -0.0 edge)
    if zero:
        e = np.unique(np.concatenate([e, [0.0]]))[:n]
    if len(e) < n:
        e = np.concatenate([e, np.ceil(e[-1]) + 1.0 + np.arange(n - len(e))])
    if inf:
        e = np.concatenate([[-np.inf], e[1:n - 1], [np.inf]]) if n > 2 else np.array([-np.inf, np.inf])[:n]
    assert len(e) == n and np.all(np.diff(e) > 0)
    return e


def _edge_sets(full):
    """(edges, closed) by the place of the stride in the case: n_edges 1, 2, 63, 64, 65 and 12 `le`-style ones"""
    return [(_edges(full, 12, zero=True, inf=True), RIGHT), (_edges(full, 1), LEFT), (_edges(full, 2, inf=True), RIGHT),
            (_edges(full, 63, zero=True), LEFT), (_edges(full, 64), RIGHT), (_edges(full, 65, zero=True), LEFT)]


def _assert_same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape, (label, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (label, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def _ranges(total, w, at):
    """the rolling suite's shapes: ranges that begin at odd and at aligned indices, overlap, come unsorted, are shorter
    than w, equal w, empty and lie over the Constant records (the 3000 NaN and the zeros of both signs among them)"""
    e = max(3, min(700, (1 << 21) // w))
    c0 = max(at - w - 5, 0)
    r = [(4096, min(w + e, total - 4096)), (1, min(w + e // 2, total - 1)), (2047, w), (2048, w - 1), (777, 0),
         (total - w, w), (c0, min(w + 5300, total - c0)), (6001, min(w + e, total - 6001)), (total, 0)]
    return [x for x in r if x[0] + x[1] <= total and x[1] >= 0]


def _strides(w):
    return sorted({s for s in (1, 2, 7, 63, 64, 65, 130, w - 1, w, w + 1) if s >= 1})


@pytest.mark.parametrize("w", WIDTHS)
def test_every_row_matches_the_model(A, ctx, main, long, w):
    recs, full, at = main
    if len(full) < w + 1000:  # the widest: the stream of 200000
        (recs, full), at = long, 150000
    total = len(full)
    sets = _edge_sets(full)
    for k, s in enumerate(_strides(w)):
        edges, closed = sets[k % len(sets)]
        rg = _ranges(total, w, at)
        if M.outputs(total, w, s) * (len(edges) + 2) <= 1 << 22:
            rg.append((0, total))  # whole, where the result stays small
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_histogram_windows_host(recs, b, c, w, edges, s, closed)
        want, woff = M.rolling(full, b, c, w, s, edges, closed)
        assert off.tolist() == woff.tolist() and got.shape == (int(off[-1]), len(edges) + 2)
        assert off[3] == off[4] == off[5] and off[3] - off[2] == 1  # shorter than w: none; equal w: one
        _assert_same(got, want, (w, s, len(edges), closed))
        assert np.all(got.sum(axis=1) == w)
        if s == 1 and w < 3000 and at < 150000:
            assert (got[:, -1] == w).any()  # a window of NaN alone


def test_both_closed_sides_on_every_stream(A, ctx, main, long, counter, ties):
    """edges equal to samples under both sides, -0.0 against a 0.0 edge, +-Inf samples and edges, NaN holes, runs on an edge"""
    for name, (recs, full, *_) in (("main", main), ("long", long), ("counter", counter), ("ties", ties)):
        n = len(full)
        for edges in (_edges(full, 12, zero=True, inf=True), _edges(full, 7, zero=True), np.array([0.0]), np.array([-np.inf, np.inf])):
            for closed in (LEFT, RIGHT):
                for w, s in ((65, 3), (300, 1), (1000, 70)):
                    b, c = [1, 8990, min(20990, n - w - 200)], [min(2 * w + 9000, n - 1), 2 * w + 40, w + 200]
                    got, off = ctx.rolling_histogram_windows_host(recs, b, c, w, edges, s, closed)
                    _assert_same(got, M.rolling(full, b, c, w, s, edges, closed)[0], (name, w, s, len(edges), closed))
    recs, full, at = main
    z = at + int(np.sum([n for _, n in CONSTANTS[:14]]))  # the 2100 samples of -0.0
    assert np.all(full[z:z + 2100] == 0.0) and np.signbit(full[z:z + 2100]).all()
    for closed, k in ((LEFT, 1), (RIGHT, 0)):
        got, _ = ctx.rolling_histogram_windows_host(recs, [z], [2100], 64, [0.0], 1, closed)
        assert np.all(got[:, k] == 64) and np.all(got.sum(axis=1) == 64)


def test_1024_edges_on_a_short_range(A, ctx, main, ties):
    for (recs, full, *_), s in ((main, 1), (ties, 5)):
        edges = _edges(full, 1024, zero=True)
        for closed in (LEFT, RIGHT):
            b, c = [4001, 17], [300 + 700, 300 + 64]
            got, off = ctx.rolling_histogram_windows_host(recs, b, c, 300, edges, s, closed)
            assert got.shape[1] == 1026
            _assert_same(got, M.rolling(full, b, c, 300, s, edges, closed)[0], (s, closed))


def test_tasks_of_fewer_exactly_and_more_than_b_positions(A, ctx, long):
    """ranges of B - 1, B, B + 1 and 2 B + 1 positions, B = clamp(8 ceil(w / s), 64, 2048): the lower clamp under both
    slides and under disjoint windows, a B between the clamps under both slides, the upper clamp"""
    recs, full = long
    edges = _edges(full, 12, inf=True)
    for w, s in ((5, 1), (20, 7), (2000, 300), (100, 100), (100, 250), (20, 1), (300, 15), (700, 65), (3600, 1)):
        bb = M.task_positions(w, s)
        assert bb == {(5, 1): 64, (20, 7): 64, (2000, 300): 64, (100, 100): 64, (100, 250): 64, (20, 1): 160, (300, 15): 160,
                      (700, 65): 88, (3600, 1): 2048}[(w, s)]
        ms = [bb - 1, bb, bb + 1, 2 * bb + 1]
        b = [1 + 45011 * i for i in range(len(ms))]
        c = [(m - 1) * s + w + (s - 1) * (i % 2) for i, m in enumerate(ms)]  # (a tail shorter than the stride adds none)
        assert b[-1] + c[-1] <= LONG
        got, off = ctx.rolling_histogram_windows_host(recs, b, c, w, edges, s, RIGHT)
        assert np.diff(off).tolist() == ms
        _assert_same(got, M.rolling(full, b, c, w, s, edges, RIGHT)[0], (w, s))


def _listed_dev(A, ctx, torch, recs, lo, w, edges, closed):
    """atsc_histogram_windows_dev over the listed windows (lo[i], w)"""
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        d = torch.zeros(len(lo) * (len(edges) + 2), dtype=torch.int64, device="cuda")
        dp.histogram_windows(body, lo, np.full(len(lo), w), edges, d, closed, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d.cpu().numpy().view(np.uint64).reshape(len(lo), len(edges) + 2)
    finally:
        dp.close()


def test_against_the_windowed_histograms_on_the_listed_windows(A, ctx, torch, main, ties):
    """equal bytes with atsc_histogram_windows_dev on the explicitly listed windows of the same positions: its
    one-wavefront tier, its chunk tier and windows of several chunks"""
    recs, full, at = main
    total = len(full)
    sets = _edge_sets(full)
    for k, (w, s) in enumerate(((1, 1), (3, 1), (65, 3), (256, 1), (300, 7), (2049, 5), (8192, 11), (20000, 64))):
        edges, closed = sets[k % len(sets)]
        c0 = max(at - w - 40, 0)
        rg = [(c0, min(w + 5300, total - c0)), (1, min(w + 2000, total - 1))]
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_histogram_windows_host(recs, b, c, w, edges, s, closed)
        listed = _listed_dev(A, ctx, torch, recs, M.positions(b, c, w, s), w, edges, closed)
        assert got.tobytes() == listed.tobytes(), (w, s)
    recs, full = ties
    edges = _edges(full, 12)
    got, off = ctx.rolling_histogram_windows_host(recs, [5], [6000], 1000, edges, 3)
    assert got.tobytes() == _listed_dev(A, ctx, torch, recs, M.positions([5], [6000], 1000, 3), 1000, edges, LEFT).tobytes()


def _raw_host(A, ctx, buf, rg, w, s, edges, closed, n_out=64, null_edges=False):
    out = np.full(n_out, SENT, dtype=np.uint64)
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    e = np.array(edges if len(edges) else [0.5], dtype=np.float64)
    p, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    rc = A.capi.lib().atsc_rolling_histogram_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(rg),
                                                     b.ctypes.data_as(p), c.ctypes.data_as(p), w, s, len(edges),
                                                     None if null_edges else e.ctypes.data_as(pd), closed,
                                                     C.c_void_p(out.ctypes.data))
    return rc, out


def test_pieces_do_not_change_the_bytes(A, ctx, long, main):
    """under the least budget a piece holds 65536 samples and consecutive pieces overlap by w - 1: the 200000 samples
    take several pieces, and the rows are the one-piece call's and the model's; a wider window than the piece is
    ATSC_E_CAPACITY"""
    recs, full = long
    edges = _edges(full, 12, inf=True)
    b, c = [0, 90001], [LONG, 30000]
    try:
        for w, s in ((300, 1), (4096, 3)):
            ref, off = ctx.rolling_histogram_windows_host(recs, b, c, w, edges, s, RIGHT)
            _assert_same(ref, M.rolling(full, b, c, w, s, edges, RIGHT)[0], ("default", w))
            ctx.set_aggregate_scratch(1)
            got, _ = ctx.rolling_histogram_windows_host(recs, b, c, w, edges, s, RIGHT)
            ctx.set_aggregate_scratch(0)
            assert got.tobytes() == ref.tobytes(), (w, s)
        # the main stream under the least budget: a large frame across the pieces' ends
        mrecs, mfull, _ = main
        assert len(mfull) > 65536
        medges = _edges(mfull, 12, zero=True)
        ctx.set_aggregate_scratch(1)
        got, _ = ctx.rolling_histogram_windows_host(mrecs, [0], [len(mfull)], 300, medges, 5)
        buf = np.frombuffer(recs, dtype=np.uint8)
        rc, out = _raw_host(A, ctx, buf, [(0, LONG)], 70001, 1000, edges, RIGHT, n_out=14 * 131)
        msg = A.capi.lib().atsc_ctx_last_error(ctx._h).decode()
        ctx.set_aggregate_scratch(70001 * 8)  # the budget the message names holds it: a piece is one window
        rc2, out2 = _raw_host(A, ctx, buf, [(777, 70001)], 70001, 1000, edges, RIGHT, n_out=14 * 2)
    finally:
        ctx.set_aggregate_scratch(0)
    _assert_same(got, M.rolling(mfull, [0], [len(mfull)], 300, 5, medges)[0], "main, least budget")
    assert rc == A.capi.E_CAPACITY and np.all(out == SENT), rc
    assert msg.startswith("rolling_histogram_windows: a window of 70001 samples does not fit one scratch piece; an aggregate "
                          "scratch budget of %d bytes would hold it" % (70001 * 8)), msg
    assert rc2 == 0
    _assert_same(out2[:14].reshape(1, 14), M.rolling(full, [777], [70001], 70001, 1000, edges, RIGHT)[0], "the named budget")
    assert out2[14:].tolist() == [SENT] * 14


def test_one_plan_serves_a_rolling_a_histogram_and_a_rolling_histogram_call(A, ctx, torch, long):
    """the rolling histograms keep their tables and scratch in the rolling's place of the plan, the windowed histograms
    in their own: enqueued one after the other without a synchronisation in between, each gives its own bytes, twice"""
    recs, full = long
    edges = _edges(full, 12, inf=True)
    b, c, w, s = [5, 100000], [12000, 9000], 3000, 3
    lo = M.positions(b, c, w, s)[::50]
    want_r, off = RM.Pyramid(full).rolling(b, c, w, s)
    n = len(want_r)
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        r1, r2 = (torch.full((4 * n,), SENT, dtype=torch.int64, device="cuda") for _ in range(2))
        h1, h2 = (torch.full((14 * n,), SENT, dtype=torch.int64, device="cuda") for _ in range(2))
        l1, l2 = (torch.full((14 * len(lo),), SENT, dtype=torch.int64, device="cuda") for _ in range(2))
        st = torch.cuda.current_stream().cuda_stream
        dp.rolling_histogram_windows(body, b, c, w, s, edges, h1, RIGHT, st)
        dp.rolling_windows(body, b, c, w, s, r1, st)
        dp.histogram_windows(body, lo, np.full(len(lo), w), edges, l1, RIGHT, st)
        dp.rolling_histogram_windows(body, b, c, w, s, edges, h2, RIGHT, st)
        dp.histogram_windows(body, lo, np.full(len(lo), w), edges, l2, RIGHT, st)
        dp.rolling_windows(body, b, c, w, s, r2, st)
        torch.cuda.synchronize()
        assert r1.cpu().numpy().tobytes() == r2.cpu().numpy().tobytes() == ctx.rolling_windows_host(recs, b, c, w, s)[0].tobytes()
        a = r1.cpu().numpy().view(A.WINDOW_ROLLING)
        assert a["count"].tolist() == want_r["count"].tolist() and a["sum"].tobytes() == want_r["sum"].tobytes()
        first = h1.cpu().numpy().view(np.uint64).reshape(n, 14)
        assert first.tobytes() == h2.cpu().numpy().tobytes()
        _assert_same(first, M.rolling(full, b, c, w, s, edges, RIGHT)[0], "rolling histogram")
        assert l1.cpu().numpy().tobytes() == l2.cpu().numpy().tobytes() == first[::50].tobytes()
    finally:
        dp.close()


def test_host_device_stream_and_bro_forms_agree(A, ctx, torch):
    x = H.synth_series(3170, 50000, block=7000)
    x[12345:12400] = np.nan
    bro = A.compress_data(ctx, x, A.AUTO, 3)
    full = A.decompress_data(ctx, bro)
    edges = _edges(full, 12, inf=True)
    n0, p0 = H.varint_decode(bro, 9)
    body = torch.from_numpy(np.frombuffer(bro[p0:], dtype=np.uint8).copy()).to("cuda")
    dp = A.DPlan(ctx, bro[p0:])
    st = A.CompressedStream.from_bytes(ctx, bro)
    try:
        for (w, s), closed in zip(((300, 1), (65, 7), (4097, 3)), (LEFT, RIGHT, LEFT)):
            b, c = [30001, 20000, 47000], [6000, 5001, 100]  # begins far into the stream: the host call uploads a part
            want, woff = M.rolling(full, b, c, w, s, edges, closed)
            via_bro, off = A.rolling_histogram_data_windows(ctx, bro, b, c, w, edges, s, closed)
            _assert_same(via_bro, want, (w, s))
            assert off.tolist() == woff.tolist()
            host, _ = ctx.rolling_histogram_windows_host(bro[9:], b, c, w, edges, s, closed, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), (w, s)
            assert st.rolling_histogram_windows(b, c, w, edges, s, closed)[0].tobytes() == via_bro.tobytes(), (w, s)
            d = torch.full((14 * len(want) + 1,), -7, dtype=torch.int64, device="cuda")
            rows, doff = dp.rolling_histogram_windows(body, b, c, w, s, edges, d, closed, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert tuple(rows.shape) == want.shape and doff.tolist() == woff.tolist() and int(d[-1]) == -7
            assert rows.cpu().numpy().tobytes() == via_bro.tobytes(), (w, s)
    finally:
        dp.close()


E1 = [0.5]
ERRORS = [([(0, 100)], 0, 1, E1, 0, "width outside"),
          ([(0, 100)], (1 << 20) + 1, 1, E1, 0, "width outside"),
          ([(0, 100)], 10, 0, E1, 0, "stride is 0"),
          ([(LONG - 50, 100)], 10, 1, E1, 0, ""),
          ([(0, 20), (LONG + 1, 0)], 10, 1, E1, 0, ""),
          ([(2 ** 63, 2 ** 63)], 10, 1, E1, 0, ""),
          ([(0, 2 ** 33)], 1, 1, E1, 0, "more than 2^32 - 2 records"),
          ([(0, 100)], 10, 1, [], 0, "n_edges outside"),
          ([(0, 100)], 10, 1, [float(k) for k in range(1025)], 0, "n_edges outside"),
          ([(0, 100)], 10, 1, [0.5, float("nan")], 0, "an edge is NaN"),
          ([(0, 100)], 10, 1, [0.5, 0.5], 0, "edges are not strictly ascending"),
          ([(0, 100)], 10, 1, [0.0, -0.0], 0, "edges are not strictly ascending"),
          ([(0, 100)], 10, 1, [1.0, 0.5], 0, "edges are not strictly ascending"),
          ([(0, 100)], 10, 1, E1, 2, "unknown closed"),
          ([(0, 100)], 10, 1, E1, -1, "unknown closed"),
          ([(0, 1 << 23)], 1, 1, [float(k) for k in range(1024)], 0, "positions x (n_edges + 2) is not below 2^32 - 1"),
          ([(0, (1 << 32) - 2)], 1, 1, E1, 0, "positions x (n_edges + 2) is not below 2^32 - 1")]


def test_errors_leave_the_result_untouched(A, ctx, torch, long):
    recs, full = long
    buf = np.frombuffer(recs, dtype=np.uint8)
    E = A.capi
    for rg, w, s, edges, closed, what in ERRORS:
        rc, out = _raw_host(A, ctx, buf, rg, w, s, edges, closed)
        msg = E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert rc == E.E_INVALID and np.all(out == SENT), (rg, w, s, len(edges), closed, rc)
        assert not what or msg.startswith("rolling_histogram_windows: " + what), msg  # the call's own checks name the call
    rc, out = _raw_host(A, ctx, buf, [(0, 100)], 10, 1, E1, 0, null_edges=True)
    assert rc == E.E_INVALID and np.all(out == SENT)
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(buf.copy()).to("cuda")
    p, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    try:
        def dev(rg, w, s, edges, closed, d_ptr, null_edges=False):
            b = np.array([x[0] for x in rg], dtype=np.uint64)
            c = np.array([x[1] for x in rg], dtype=np.uint64)
            e = np.array(edges if len(edges) else [0.5], dtype=np.float64)
            rc = E.lib().atsc_rolling_histogram_windows_dev(ctx._h, dp._h, C.c_void_p(body.data_ptr()), len(rg), b.ctypes.data_as(p),
                                                            c.ctypes.data_as(p), w, s, len(edges),
                                                            None if null_edges else e.ctypes.data_as(pd), closed, C.c_void_p(d_ptr),
                                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            return rc

        d = torch.full((512,), SENT, dtype=torch.int64, device="cuda")
        for rg, w, s, edges, closed, what in ERRORS:
            assert dev(rg, w, s, edges, closed, d.data_ptr()) == E.E_INVALID and bool((d == SENT).all()), (rg, w, s, len(edges), closed)
            msg = E.lib().atsc_ctx_last_error(ctx._h).decode()
            assert not what or msg.startswith("rolling_histogram_windows: " + what), msg
        assert dev([(0, 100)], 10, 1, E1, 0, d.data_ptr(), null_edges=True) == E.E_INVALID and bool((d == SENT).all())
        assert dev([(0, 100)], 10, 1, E1, 0, d.data_ptr() + 4) == E.E_INVALID and bool((d == SENT).all())
        assert "d_out is not 8-byte aligned" in E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert dev([(0, 100)], 10, 1, E1, 0, d.data_ptr()) == 0 and bool((d[273:] == SENT).all()) and not bool((d[:273] == SENT).any())
    finally:
        dp.close()
    st = A.CompressedStream.from_bytes(ctx, A.compress_data(ctx, np.arange(1000.0), A.NOOP, 0))
    with pytest.raises(A.AtscError) as e:
        st.rolling_histogram_windows([0], [100], (1 << 20) + 1, [0.5])
    assert e.value.rc == E.E_INVALID
    with pytest.raises(A.AtscError) as e:
        st.rolling_histogram_windows([0], [100], 10, [1.5, 1.5])
    assert e.value.rc == E.E_INVALID
    assert st.rolling_histogram_windows([0], [100], 10, [50.0])[0].tolist() == \
        [[min(10, max(0, 50 - j)), 10 - min(10, max(0, 50 - j)), 0] for j in range(91)]
    rc, out = _raw_host(A, ctx, buf, [], 5, 1, E1, 0)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, buf, [(5, 0), (LONG, 0), (7, 4)], 5, 1, E1, 0)  # no range holds a window: no row
    assert rc == 0 and np.all(out == SENT)


def test_malformed_payload(A, ctx, torch):
    n, nf = 256, 8
    x = H.synth_series(909, n * nf, klass=2)
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.05)), 0)
    good = ctx.decompress_host(recs)
    edges = _edges(good, 12)
    frames = H.parse_bro_body(recs, with_count=False)
    pos = sum(len(_rec(f[1], f[2], f[3])) for f in frames[:3])
    rec3 = _rec(frames[3][1], frames[3][2], frames[3][3])
    pay = pos + len(rec3) - len(frames[3][3])
    assert recs[pay] == 15 and recs[pay + 1] < 200
    bad = bytearray(recs)
    bad[pay + 1] = 250  # frame 3: more stored bins than the transform has; the record walk stays valid
    bad = bytes(bad)
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 20, 20), (5 * n + 3, 100), (3 * n + 5, 0)]
    b, c = [w[0] for w in outside], [w[1] for w in outside]
    got, _ = ctx.rolling_histogram_windows_host(bad, b, c, 20, edges, 3)
    _assert_same(got, M.rolling(good, b, c, 20, 3, edges)[0], "outside")
    bb = np.frombuffer(bad, dtype=np.uint8)
    for rg in ([(3 * n, 20)], [(0, nf * n)], [(0, 40), (3 * n - 19, 20)], [(4 * n - 20, 20), (6 * n, 50)]):
        rc, out = _raw_host(A, ctx, bb, rg, 20, 1, edges, 0, n_out=14 * nf * n)
        assert rc == A.capi.E_FORMAT and np.all(out == SENT), (rg, rc)
    # The device call sets the plan's status word, which has no accessor (see tests/test_gpu_histogram.py): the host call
    # above -- the device call on a plan of the touched records, then a read of the plan's word -- is what shows it.  The
    # device call itself returns ATSC_OK, finishes, writes every row, and gives the ranges beside the bad frame theirs.
    dp = A.DPlan(ctx, bad)
    body = torch.from_numpy(bb.copy()).to("cuda")
    try:
        rg = [(0, 3 * n), (3 * n + 7, 40), (4 * n, 100)]
        b, c = [w[0] for w in rg], [w[1] for w in rg]
        want, off = M.rolling(good, b, c, 20, 1, edges)
        d = torch.full((14 * len(want),), SENT, dtype=torch.int64, device="cuda")
        dp.rolling_histogram_windows(body, b, c, 20, 1, edges, d, LEFT, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        h = d.cpu().numpy().view(np.uint64)
        assert not (h == SENT).any()
        clean = np.r_[0: int(off[1]), int(off[2]): int(off[3])]
        _assert_same(h.reshape(-1, 14)[clean], want[clean], "dev, beside the bad frame")
    finally:
        dp.close()


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def _check_rows(plain, with_h, first, n_edges, want, in_front=""):
    """the .roll.csv of one call without and with --rolling-histogram: the other columns are the plain file's, byte for
    byte; the counters' columns come last, named h0 .. h<n_edges>,hnan, and are the model's"""
    base, hl = plain.split("\n"), with_h.split("\n")
    names = "".join(",h%d" % k for k in range(n_edges + 1)) + ",hnan"
    assert base[0] == first + ",count,min,max,sum,mean" + in_front and hl[0] == base[0] + names
    assert len(base) == len(hl) == len(want) + 2 and base[-1] == hl[-1] == ""
    k = n_edges + 2
    for j in range(len(want)):
        cells = hl[1 + j].split(",")
        assert ",".join(cells[:-k]) == base[1 + j]
        assert [int(t) for t in cells[-k:]] == want[j].tolist(), (j, cells[-k:])


def test_csv_compressor_command_line(A, ctx, golden_dir, tmp_path):
    from oracle import vsri_oracle as VO

    csvc = os.path.join(os.path.dirname(A.__file__), "bin", "csv-compressor")
    lines = open(os.path.join(golden_dir, "csv", "cpu_utilization.csv")).read().split("\n")[1:]
    rows = [l.split(",") for l in lines if l]
    m = tmp_path / "cpu.csv"
    m.write_text(VO.samples_to_csv_text([int(t) * 1000 for t, _ in rows], [float(v) for _, v in rows]))
    _run(csvc, "--output-vsri", "--compressor", "fft", "-e", "3", m)
    _run(csvc, "-u", "-o", tmp_path / "all", tmp_path / "cpu.bro")
    times = np.array([int(r.split(",")[0]) for r in (tmp_path / "all.csv").read_text().split("\n")[1:] if r])
    cbro = (tmp_path / "cpu.bro").read_bytes()
    full = A.decompress_data(ctx, cbro)
    fin = full[np.isfinite(full)]
    lo_v, hi_v = float(np.floor(fin.min())), float(np.ceil(fin.max())) + 1.0
    hi = len(times) - 3
    common = (csvc, "-u", "--from", times[10], "--to", times[hi], "-o", tmp_path / "win")
    at = np.flatnonzero((times >= times[10]) & (times <= times[hi]))
    mid = float(np.median(fin))
    for spec, (w, s), hspec, edges, extra, closed in (
            ("20:3", (20, 3), "%r,%r" % (mid, hi_v), [mid, hi_v], (), LEFT),
            ("20", (20, 1), "%r:%r:8" % (lo_v, hi_v), A.histogram_edges_uniform(lo_v, hi_v, 8), ("--histogram-closed", "right"), RIGHT)):
        _run(*common, "--rolling", spec, tmp_path / "cpu.bro")
        plain = (tmp_path / "win.roll.csv").read_text()
        _run(*common, "--rolling", spec, "--rolling-histogram", hspec, *extra, tmp_path / "cpu.bro")
        want, _ = M.rolling(full, [int(at[0])], [len(at)], w, s, edges, closed)
        assert len(want) == M.outputs(len(at), w, s) > 0
        _check_rows(plain, (tmp_path / "win.roll.csv").read_text(), "timestamp", len(edges), want)
    for bad, what in ((("--rolling-histogram", "0.5"), "'--rolling-histogram' needs '--rolling'"),
                      (("--rolling", "20", "--rolling-histogram", "1,x"), "invalid value '1,x' for '--rolling-histogram'"),
                      (("--rolling", "20", "--rolling-histogram", "2,1"), "invalid value '2,1' for '--rolling-histogram'"),
                      (("--rolling", "20", "--histogram-closed", "right"), "'--histogram-closed' needs '--histogram'")):
        r = subprocess.run([str(a) for a in common[:-2]] + list(bad) + [str(tmp_path / "cpu.bro")], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 2 and what in r.stderr, (bad, r.returncode, r.stderr)


def test_command_line(A, ctx, golden_dir, tmp_path):
    atsc = os.path.join(os.path.dirname(A.__file__), "bin", "atsc")
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    fin = full[np.isfinite(full)]
    lo_v, hi_v = float(np.floor(fin.min())), float(np.ceil(fin.max())) + 1.0
    q = [float(v) for v in np.unique(np.quantile(fin, [0.1, 0.5, 0.9], method="nearest"))]
    out = tmp_path / "uptime.roll.csv"
    for spec, (b0, c0), (w, s), hspec, edges, extra, closed in (
            ("20", (0, len(full)), (20, 1), ",".join(repr(v) for v in q), q, (), LEFT),
            ("300:15", (100, 1500), (300, 15), "%r:%r:12" % (lo_v, hi_v), A.histogram_edges_uniform(lo_v, hi_v, 12),
             ("--histogram-closed", "right"), RIGHT)):
        common = (atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--rolling", spec)
        want, _ = M.rolling(full, [b0], [c0], w, s, edges, closed)
        assert len(want) == M.outputs(c0, w, s) > 0
        _run(*common, tmp_path / "uptime.bro")
        plain = out.read_text()
        _run(*common, "--rolling-histogram", hspec, *extra, tmp_path / "uptime.bro")
        _check_rows(plain, out.read_text(), "offset", len(edges), want)
        _run(*common, "--rolling-moments", tmp_path / "uptime.bro")  # behind the moments' columns where both are given
        plain_m = out.read_text()
        _run(*common, "--rolling-moments", "--rolling-histogram", hspec, *extra, tmp_path / "uptime.bro")
        _check_rows(plain_m, out.read_text(), "offset", len(edges), want, ",nonnan,avg,stdvar,stddev,slope,intercept")
    for bad, what in ((("-u", "--rolling-histogram", "0.5"), "'--rolling-histogram' needs '--rolling'"),
                      (("-u", "--samples", "0:10", "--buckets", "5", "--rolling-histogram", "0.5"), "'--rolling-histogram' needs '--rolling'"),
                      (("-u", "--samples", "0:100", "--rolling", "20", "--rolling-histogram", "0:1"),
                       "invalid value '0:1' for '--rolling-histogram'"),
                      (("-u", "--samples", "0:100", "--rolling", "20", "--rolling-histogram", "0:1:0"),
                       "invalid value '0:1:0' for '--rolling-histogram'")):
        r = subprocess.run([atsc, *bad, str(tmp_path / "uptime.bro")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and what in r.stderr, (bad, r.returncode, r.stderr)
