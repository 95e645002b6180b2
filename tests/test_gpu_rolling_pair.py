"""Windowed rolling pair moments on the GPU: every record of every case against the NumPy model of the contract
(tests/rolling_pair_model.py) applied to the GPU's own two full decodes: count exactly, each double bit for bit, except
that where the model's value is NaN any NaN conforms (the main stream holds +-Inf Constant records).  X is the rolling
suite's main stream (every frame-length tier below the large one under every codec, one large frame, Constant records of
NaN, +-Inf and zeros of both signs); Y has another framing: Noop frames of 4096 with Constant-NaN holes in other places
than X's and a large frame that lies across the least budget's first piece end, so that both inputs use spill slots
there.  Noop pairs of mixed magnitudes 1e3 .. 1e17, where every merge rounds, serve the widths across the 2^16 and the
2^18 level and the budgets that cut a range into pieces.  dp_y = dp_x against the rolling moments; swapped inputs;
against atsc_pair_windows_dev on the listed windows; the host, device, stream and .bro calls; a rolling moments, a
rolling pair and a rolling call on one plan; capacity; errors that leave the result untouched; a malformed payload in
either stream; the atsc command line."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import helpers as H
from tests import pair_model as PM
from tests import rolling_model as RM
from tests import rolling_moments_model as MO
from tests import rolling_pair_model as M
from tests.test_gpu_rolling import CONSTANTS, LENS, _const_record, _fft_record, _rec
from tests.test_gpu_rolling_moments import LONG, SENT, WIDTHS, _noop_records, _ranges, _wide

pytestmark = pytest.mark.gpu

DOUBLES = M.FIELDS[1:]
SWAP = ("count", "mean_y", "m2_y", "mean_x", "m2_x", "c_xy")
LEAST_PIECE = 65536 - 3 * 2048  # the least budget's piece: 59392 samples


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
    """-> (X records, X decode, Y records, Y decode, model pyramid, first sample of X's Constant records).  X is built
    as the rolling suite's main stream; Y around it"""
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
    assert 65536 < len(full) <= 200000 and np.isinf(full).any() and np.isnan(full).any()
    # Y: integers in Noop frames of 4096, NaN holes at 20000 (3), 36000 (70), 50 in front of X's Constant records (40)
    # and behind X's end (1); a frame of the large tier over [56000, 64192): across the least budget's first piece end
    # (59392) and across the begin of its second piece for every width the least-budget test uses
    assert at > 70000
    yr = np.random.default_rng(19)

    def ints(n):
        return np.round(yr.normal(0, 1, n) * 10.0 ** yr.integers(0, 7, n))

    yrecs = b""
    for n, hole in ((20000, 3), (15997, 70), (19930, 0)):
        yrecs += _noop_records(A, ctx, ints(n)) + (_const_record(A, ctx, np.nan, hole) if hole else b"")
    yrecs += ctx.compress_host(H.synth_series(3155, 8192, klass=2), np.array([0, 8192], dtype=np.uint64), A.FFT, True,
                               float(np.float32(0.01)), 0)[0]
    yrecs += _noop_records(A, ctx, ints(at - 50 - 64192)) + _const_record(A, ctx, np.nan, 40)
    yrecs += _noop_records(A, ctx, ints(len(full) - (at - 10) + 777)) + _const_record(A, ctx, np.nan, 1)
    yrecs += _noop_records(A, ctx, ints(4500))
    yfull = ctx.decompress_host(yrecs)
    assert len(yfull) == len(full) + 777 + 1 + 4500 and np.isnan(yfull[at - 50:at - 10]).all()
    assert not np.isnan(yfull[56000:64192]).any() and np.isnan(yfull[20000:20003]).all()
    return recs, full, yrecs, yfull, M.Pyramid(full, yfull), at


def _noop(A, ctx, x):
    recs = _noop_records(A, ctx, x)
    full = ctx.decompress_host(recs)
    assert np.array_equal(full, x)
    return recs, full


@pytest.fixture(scope="module")
def long(A, ctx):
    """two streams of 200000 integers of mixed magnitude in Noop frames, no NaN -> (X records, X, Y records, Y, pyramid)"""
    xr, x = _noop(A, ctx, _wide(np.random.default_rng(23), LONG))
    yr, y = _noop(A, ctx, _wide(np.random.default_rng(37), LONG))
    return xr, x, yr, y, M.Pyramid(x, y)


def _assert_same(got, want, label):
    """count exactly; each double bit for bit, any NaN where the model's value is NaN"""
    assert len(got) == len(want), (label, len(got), len(want))
    a = np.ascontiguousarray(got).view(np.uint64).reshape(-1, 6)
    b = np.ascontiguousarray(want).view(np.uint64).reshape(-1, 6)
    ok = a == b
    ok[:, 1:] |= np.isnan(a[:, 1:].view(np.float64)) & np.isnan(b[:, 1:].view(np.float64))
    bad = np.flatnonzero(~ok.all(axis=1))
    assert len(bad) == 0, (label, len(bad), int(bad[0]), a[bad[0]].view(np.float64), b[bad[0]].view(np.float64), a[bad[0]][0],
                           b[bad[0]][0])


def _counts(v, w):
    """the samples that are not NaN in every window of w of v"""
    c = np.concatenate([[0], np.cumsum(~np.isnan(v))])
    return c[w:] - c[:-w]


def _swapped(r):
    out = np.zeros(len(r), dtype=r.dtype)
    for k, v in zip(M.FIELDS, SWAP):
        out[k] = r[v]
    return out


def _dev(A, torch, dpx, bx, dpy, by, b, c, w, s, n, pad=6):
    """the device call -> (its n records, the words behind them, the offsets)"""
    d = torch.full((6 * n + pad,), SENT, dtype=torch.int64, device="cuda")
    off = dpx.rolling_pair_windows(bx, dpy, by, b, c, w, s, d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    return h[: 6 * n].view(A.WINDOW_PAIR), h[6 * n:], off


def _on_device(torch, recs):
    return torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")


@pytest.mark.parametrize("w", WIDTHS)
def test_every_record_matches_the_model(A, ctx, main, w):
    recs, full, yrecs, yfull, P, at = main
    for s in (1, 7, w, 2 * w + 1):
        rg = _ranges(len(full), w, at)
        if s > 7:
            rg = rg[:-1] + [(3, len(full) - 3)]
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_pair_windows_host(recs, yrecs, b, c, w, s)
        want, woff = P.rolling(b, c, w, s)
        assert off.tolist() == woff.tolist() and got.dtype == A.WINDOW_PAIR
        assert off[3] == off[4] == off[5] and off[3] - off[2] == 1  # shorter than w: none; equal w: one
        _assert_same(got, want, (w, s))
        if s == 1:  # X's 3000 NaN give empty windows
            assert np.isnan(got["c_xy"][got["count"] == 0]).all() and ((got["count"] == 0).any() or w > 3000)
            # the last range is the whole of X: windows whose count lies below both streams' own counts (Y's hole ends
            # 10 in front of X's Constant records, whose fourth to eighth samples are NaN)
            whole = got[int(off[-2]):]
            nx, ny = _counts(full, w), _counts(yfull[: len(full)], w)
            assert len(whole) == len(nx) and np.all(whole["count"] <= np.minimum(nx, ny))
            assert w < 64 or np.any((whole["count"] < nx) & (whole["count"] < ny)), w


def test_width_across_the_65536_level(A, ctx, torch, long):
    xr, x, yr, y, P = long
    w = 70001
    dpx, dpy = A.DPlan(ctx, xr), A.DPlan(ctx, yr)
    bx, by = _on_device(torch, xr), _on_device(torch, yr)
    try:
        for s, rg in ((1, [(0, LONG)]), (7, [(65535, LONG - 65535), (1, 140003)]), (w, [(3, LONG - 3)]),
                      (2 * w + 1, [(0, LONG), (60000, w)])):
            b, c = [r[0] for r in rg], [r[1] for r in rg]
            want, woff = P.rolling(b, c, w, s)
            got, rest, off = _dev(A, torch, dpx, bx, dpy, by, b, c, w, s, len(want))
            assert off.tolist() == woff.tolist() and np.all(rest == SENT)
            _assert_same(got, want, (w, s))
    finally:
        dpx.close()
        dpy.close()


def test_width_across_the_262144_level(A, ctx):
    """w = 2^18 + 1: the chunks of level 18 come from the second launch of the upper kernel, over a pyramid that lies
    behind two regions"""
    w = (1 << 18) + 1
    n = (1 << 18) + 5000
    rng = np.random.default_rng(31)
    xr, x = _noop(A, ctx, _wide(rng, n))
    yr, y = _noop(A, ctx, _wide(rng, n + 3))
    got, off = ctx.rolling_pair_windows_host(xr, yr, [0], [n], w, 1)
    want, woff = M.Pyramid(x, y).rolling([0], [n], w, 1)
    assert off.tolist() == woff.tolist() == [0, n - w + 1]
    _assert_same(got, want, w)


def test_the_same_plan_twice_is_the_rolling_moments(A, ctx, torch, main, long):
    """dp_y = dp_x: count, mean_x and m2_x are atsc_rolling_moments_windows_dev's bytes, and m2_y == c_xy == m2_x"""
    for recs, full, rg, shapes in ((main[0], main[1], [(1, len(main[1]) - 1), (main[5] - 5000, 9000)], ((3, 1), (65, 3), (2049, 5))),
                                   (long[0], long[1], [(0, LONG), (60000, 70001)], ((300, 7), (70001, 11)))):
        dp, body = A.DPlan(ctx, recs), _on_device(torch, recs)
        try:
            b, c = [r[0] for r in rg], [r[1] for r in rg]
            for w, s in shapes:
                n = int(A.rolling_offsets(c, w, s)[-1])
                got, rest, _ = _dev(A, torch, dp, body, dp, body, b, c, w, s, n)
                assert n > 0 and np.all(rest == SENT)
                d = torch.full((6 * n,), SENT, dtype=torch.int64, device="cuda")
                dp.rolling_moments_windows(body, b, c, w, s, d, torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                mo = d.cpu().numpy().view(A.WINDOW_MOMENTS)
                for mine, theirs in (("count", "count"), ("mean_x", "mean"), ("m2_x", "m2")):
                    assert got[mine].tobytes() == mo[theirs].tobytes(), (w, s, mine)
                assert got["mean_y"].tobytes() == got["mean_x"].tobytes(), (w, s)
                assert got["m2_y"].tobytes() == got["m2_x"].tobytes() == got["c_xy"].tobytes(), (w, s)
                _assert_same(got, M.Pyramid(full, full).rolling(b, c, w, s)[0], ("y = x", w, s))
        finally:
            dp.close()


def test_swapped_inputs_swap_the_fields(A, ctx, main, long):
    recs, full, yrecs, yfull, P, at = main
    for w, s in ((1, 1), (9, 1), (300, 7), (4097, 3)):
        b, c = [1, at - w - 200], [len(full) - 1, 2 * w + 3500]
        xy, _ = ctx.rolling_pair_windows_host(recs, yrecs, b, c, w, s)
        yx, _ = ctx.rolling_pair_windows_host(yrecs, recs, b, c, w, s)
        _assert_same(yx, _swapped(xy), (w, s))
        _assert_same(xy, P.rolling(b, c, w, s)[0], (w, s))
    xr, x, yr, y, LP = long
    xy, _ = ctx.rolling_pair_windows_host(xr, yr, [5], [LONG - 5], 70001, 13)
    yx, _ = ctx.rolling_pair_windows_host(yr, xr, [5], [LONG - 5], 70001, 13)
    assert yx.tobytes() == _swapped(xy).tobytes()


def _within_both_bounds(x, y, lo, w, mine, theirs, label):
    """each double of `mine` (the rolling pair's) against `theirs` (the windowed pair's) of the window (lo, w): within the
    sum of the two calls' stated bounds, whose scales are the window's exact moments (rational arithmetic)"""
    en, emx, em2x, emy, em2y, _, eax, eay = PM.exact_pair(x[lo:lo + w], y[lo:lo + w])
    a, b = M.bounds(w, en, emx, em2x, emy, em2y), PM.bounds(en, emx, em2x, emy, em2y)
    lims = {"mean_x": (a[0] + b[0]) * float(eax), "m2_x": a[1] + b[1], "mean_y": (a[0] + b[0]) * float(eay),
            "m2_y": a[2] + b[2], "c_xy": a[3] + b[3]}
    for k in DOUBLES:
        assert abs(Fraction(float(mine[k])) - Fraction(float(theirs[k]))) <= lims[k], (label, lo, k, mine[k], theirs[k], lims[k])


def test_against_the_windowed_pair_on_the_listed_windows(A, ctx, torch, main):
    """count exactly on every listed window; the doubles, which come from another tree, within the two bounds where the
    window's samples are finite -- on every 1 + len // 40-th window, exact arithmetic being what the bounds are stated in"""
    recs, full, yrecs, yfull, P, at = main
    total = len(full)
    dpx, dpy = A.DPlan(ctx, recs), A.DPlan(ctx, yrecs)
    bx, by = _on_device(torch, recs), _on_device(torch, yrecs)
    try:
        for w, s in ((1, 1), (2, 1), (3, 1), (65, 3), (300, 7), (2049, 5), (4097, 11)):
            rg = [(max(at - w - 40, 0), min(2 * w + 5300, total - max(at - w - 40, 0))), (1, min(w + 2000, total - 1))]
            b, c = [r[0] for r in rg], [r[1] for r in rg]
            got, off = ctx.rolling_pair_windows_host(recs, yrecs, b, c, w, s)
            lo = np.concatenate([rg[i][0] + s * np.arange(int(off[i + 1] - off[i])) for i in range(len(rg))])
            d = torch.zeros(6 * len(lo), dtype=torch.int64, device="cuda")
            dpx.pair_windows(bx, dpy, by, lo, np.full(len(lo), w), d, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ref = d.cpu().numpy().view(A.WINDOW_PAIR)
            assert got["count"].tobytes() == ref["count"].tobytes(), (w, s)
            checked = 0
            for i in range(0, len(lo), 1 + len(lo) // 40):
                a = int(lo[i])
                vx, vy = full[a:a + w], yfull[a:a + w]
                if got["count"][i] and np.isfinite(vx[~np.isnan(vx)]).all() and np.isfinite(vy[~np.isnan(vy)]).all():
                    _within_both_bounds(full, yfull, a, w, got[i], ref[i], (w, s))
                    checked += 1
            assert checked >= 10, (w, s, checked)
    finally:
        dpx.close()
        dpy.close()


def test_host_device_stream_and_image_calls_agree(A, ctx, torch):
    x = H.synth_series(3170, 50000, block=7000)
    x[12345:12400] = np.nan
    y = H.synth_series(3171, 52000, block=5000)
    y[31000:31020] = np.nan
    bro_x, bro_y = A.compress_data(ctx, x, A.AUTO, 3), A.compress_data(ctx, y, A.FFT, 1)
    P = M.Pyramid(A.decompress_data(ctx, bro_x), A.decompress_data(ctx, bro_y))
    px, py = H.varint_decode(bro_x, 9)[1], H.varint_decode(bro_y, 9)[1]
    dpx, dpy = A.DPlan(ctx, bro_x[px:]), A.DPlan(ctx, bro_y[py:])
    bx, by = _on_device(torch, bro_x[px:]), _on_device(torch, bro_y[py:])
    sx, sy = A.CompressedStream.from_bytes(ctx, bro_x), A.CompressedStream.from_bytes(ctx, bro_y)
    try:
        for w, s in ((300, 1), (65, 7), (4097, 3)):
            b, c = [30001, 20000, 47000], [15000, 12001, 100]  # begins far into the streams: the host call uploads a part of each
            want, woff = P.rolling(b, c, w, s)
            via_bro, off = A.rolling_pair_data_windows(ctx, bro_x, bro_y, b, c, w, s)
            _assert_same(via_bro, want, (w, s))
            assert off.tolist() == woff.tolist()
            host, _ = ctx.rolling_pair_windows_host(bro_x[9:], bro_y[9:], b, c, w, s, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), (w, s)
            assert sx.rolling_pair_windows(sy, b, c, w, s)[0].tobytes() == via_bro.tobytes(), (w, s)
            got, rest, _ = _dev(A, torch, dpx, bx, dpy, by, b, c, w, s, len(want), pad=1)
            assert got.tobytes() == via_bro.tobytes() and np.all(rest == SENT), (w, s)
            fit = A.pair_fit(via_bro)  # the records are the windowed pair moments': the fit applies as it is
            some = via_bro["count"] > 1
            assert len(fit) == len(want) and np.isfinite(fit["slope"][some]).all()
            assert np.all(np.abs(fit["correlation"][some]) <= 1.0)
    finally:
        dpx.close()
        dpy.close()


def test_the_rolling_calls_share_the_plans_place(A, ctx, torch, long):
    """a rolling moments, a rolling pair and a rolling call keep their tables and scratch in one place of the plan:
    enqueued one after the other without a synchronisation in between, each gives its own bytes"""
    xr, x, yr, y, P = long
    b, c, w, s = [5, 100000], [90000, 30000], 3000, 3
    want_r, off = RM.Pyramid(x).rolling(b, c, w, s)
    n = len(want_r)
    dpx, dpy = A.DPlan(ctx, xr), A.DPlan(ctx, yr)
    bx, by = _on_device(torch, xr), _on_device(torch, yr)
    try:
        r1 = torch.full((4 * n,), SENT, dtype=torch.int64, device="cuda")
        m1, p1, p2 = (torch.full((6 * n,), SENT, dtype=torch.int64, device="cuda") for _ in range(3))
        q = torch.cuda.current_stream().cuda_stream
        dpx.rolling_pair_windows(bx, dpy, by, b, c, w, s, p1, q)
        dpx.rolling_moments_windows(bx, b, c, w, s, m1, q)
        dpx.rolling_pair_windows(bx, dpy, by, b, c, w + 2, s, p2, q)  # (another width: other level tables in the same place)
        dpx.rolling_windows(bx, b, c, w, s, r1, q)
        torch.cuda.synchronize()
        a = r1.cpu().numpy().view(A.WINDOW_ROLLING)
        assert a["count"].tolist() == want_r["count"].tolist() and a["sum"].tobytes() == want_r["sum"].tobytes()
        assert m1.cpu().numpy().tobytes() == ctx.rolling_moments_windows_host(xr, b, c, w, s)[0].tobytes()
        _assert_same(m1.cpu().numpy().view(A.WINDOW_MOMENTS), MO.Pyramid(x).rolling(b, c, w, s)[0], "moments between the pairs")
        _assert_same(p1.cpu().numpy().view(A.WINDOW_PAIR), P.rolling(b, c, w, s)[0], "in front of a rolling moments call")
        want_p2, _ = P.rolling(b, c, w + 2, s)
        assert 0 < len(want_p2) <= n
        _assert_same(p2.cpu().numpy()[: 6 * len(want_p2)].view(A.WINDOW_PAIR), want_p2, "between the two others")
    finally:
        dpx.close()
        dpy.close()


def _pieces(n, budget, w):
    """the pieces of a range of n samples from sample 0 of two streams without large frames under a budget, by DESIGN.md's
    piece arithmetic with 28 bytes a slot: the budget's samples halved into the two inputs' shares L (at least 65536), a
    region of Lr = max(65536, 16 L / 28 rounded down to 2048) samples, a piece of Lr - 3 * 2048, consecutive pieces
    overlapping by w - 1"""
    share = max(65536, budget // 8 // 2)
    lp = max(65536, share * 16 // 28 // 2048 * 2048) - 3 * 2048
    k, p = 1, 0
    while p + lp < n:
        p, k = p + lp - (w - 1), k + 1
    return k


def test_pieces_do_not_change_the_bytes(A, ctx, long, main):
    xr, x, yr, y, P = long
    b, c = [0, 90001], [LONG, 30000]
    two, least = 110592 * 28, 1
    try:
        for w in (3000, 50000):  # the second: close to the least budget's piece of 59392, which then advances by 9393
            ref, _ = ctx.rolling_pair_windows_host(xr, yr, b, c, w, 1)
            _assert_same(ref, P.rolling(b, c, w, 1)[0], "default")
            assert _pieces(LONG, two, w) == (2 if w == 3000 else 3) and _pieces(LONG, least, w) >= (3 if w == 3000 else 15)
            for budget in (two, least):
                ctx.set_aggregate_scratch(budget)
                got, _ = ctx.rolling_pair_windows_host(xr, yr, b, c, w, 1)
                assert got.tobytes() == ref.tobytes(), (w, budget)
                if w == 3000:
                    got7, _ = ctx.rolling_pair_windows_host(xr, yr, b, c, w, 7)
                    assert got7.tobytes() == ref[: LONG - w + 1][::7].tobytes() + ref[LONG - w + 1:][::7].tobytes(), budget
            ctx.set_aggregate_scratch(0)
        # the main streams under the least budget: a large frame of each across the pieces' ends.  Y's lies over
        # [56000, 64192), across the first piece's end at 59392; X's over [at - 8192, at), and wx is the width that puts
        # the second piece's end, 2 * 59392 - (wx - 1), 4000 samples in front of `at`
        mrecs, mfull, yrecs, yfull, MP, at = main
        wx = 2 * LEAST_PIECE + 1 - (at - 4000)
        assert 3000 < wx < 50000 and at < len(mfull)
        got = {}
        ctx.set_aggregate_scratch(1)
        for w in (3000, wx):
            assert LEAST_PIECE - (w - 1) < 64192  # the second piece begins inside or in front of Y's large frame
            got[w], _ = ctx.rolling_pair_windows_host(mrecs, yrecs, [0], [len(mfull)], w, 1)
    finally:
        ctx.set_aggregate_scratch(0)
    for w in got:
        _assert_same(got[w], MP.rolling([0], [len(mfull)], w, 1)[0], ("main, least budget", w))


def _raw_host(A, ctx, bufx, bufy, rg, w, s, n_out=16):
    out = np.full(6 * n_out, SENT, dtype=np.uint64)
    b = np.array([r[0] for r in rg], dtype=np.uint64)
    c = np.array([r[1] for r in rg], dtype=np.uint64)
    p, q = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    rc = A.capi.lib().atsc_rolling_pair_windows(ctx._h, bufx.ctypes.data_as(q), len(bufx), 0, bufy.ctypes.data_as(q), len(bufy), 0,
                                                len(rg), b.ctypes.data_as(p), c.ctypes.data_as(p), w, s, C.c_void_p(out.ctypes.data))
    return rc, out


def test_capacity_message_names_a_budget_that_serves(A, ctx, long):
    xr, x, yr, y, P = long
    bx, by = np.frombuffer(xr, dtype=np.uint8), np.frombuffer(yr, dtype=np.uint8)
    E = A.capi
    try:
        ctx.set_aggregate_scratch(1)
        rc, out = _raw_host(A, ctx, bx, by, [(0, 70010)], 70001, 1)
        assert rc == E.E_CAPACITY and np.all(out == SENT)
        msg = E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert msg.startswith("rolling_pair_windows: a window of 70001 samples"), msg
        need = int(msg.split("budget of ")[1].split(" bytes")[0])
        assert need == (70001 + 4 * 2048) * 28  # 8 bytes a sample of each stream and 12 of chunk partials; no large frame: no spill
        ctx.set_aggregate_scratch(need)
        rc, out = _raw_host(A, ctx, bx, by, [(0, 70010)], 70001, 1)
        assert rc == 0 and np.all(out[60:] == SENT)
        _assert_same(out[:60].view(A.WINDOW_PAIR), P.rolling([0], [70010], 70001, 1)[0], "the named budget")
        ctx.set_aggregate_scratch(1)
        rc, out = _raw_host(A, ctx, bx, by, [(0, 59392 + 15)], 59392, 1)  # the widest that the least budget holds
        assert rc == 0 and np.all(out[96:] == SENT)
        _assert_same(out[:96].view(A.WINDOW_PAIR), P.rolling([0], [59392 + 15], 59392, 1)[0], "widest")
        rc, out = _raw_host(A, ctx, bx, by, [(0, 59393 + 15)], 59393, 1)
        assert rc == E.E_CAPACITY and np.all(out == SENT)
    finally:
        ctx.set_aggregate_scratch(0)
    rc, out = _raw_host(A, ctx, bx, by, [(0, 70010)], 70001, 1)  # the default budget holds any width
    assert rc == 0 and np.all(out[60:] == SENT) and not np.any(out[:60] == SENT)


def _raw_dev(A, torch, ctx, dpx, bx, dpy, by, rg, w, s):
    d = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
    b = np.array([r[0] for r in rg], dtype=np.uint64)
    c = np.array([r[1] for r in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    rc = A.capi.lib().atsc_rolling_pair_windows_dev(ctx._h, dpx._h, C.c_void_p(bx.data_ptr()), dpy._h, C.c_void_p(by.data_ptr()),
                                                    len(rg), b.ctypes.data_as(p), c.ctypes.data_as(p), w, s,
                                                    C.c_void_p(d.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool((d == SENT).all())


def test_errors_leave_the_result_untouched(A, ctx, torch, long):
    xr, x, yr, y, P = long
    short = 150000
    sr, _ = _noop(A, ctx, y[:short])
    bufx, bufy, bufs = (np.frombuffer(r, dtype=np.uint8) for r in (xr, yr, sr))
    E = A.capi
    cases = [([(0, 100)], 0, 1, "width outside"), ([(0, 100)], A.ROLLING_MAX_WIDTH + 1, 1, "width outside"),
             ([(0, 100)], 10, 0, "stride is 0"), ([(LONG - 50, 100)], 10, 1, ""), ([(0, 20), (LONG + 1, 0)], 10, 1, ""),
             ([(2 ** 63, 2 ** 63)], 10, 1, ""), ([(0, 2 ** 33)], 1, 1, "more than 2^32 - 2 records")]
    beyond_y = [(0, 50), (short - 50, 100)]  # inside X, beyond the end of the shorter Y only
    for rg, w, s, what in cases:
        rc, out = _raw_host(A, ctx, bufx, bufy, rg, w, s)
        msg = E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert rc == E.E_INVALID and np.all(out == SENT), (rg, w, s, rc)
        assert not what or msg.startswith("rolling_pair_windows: " + what), msg  # the call's own checks name the call
    rc, out = _raw_host(A, ctx, bufx, bufs, beyond_y, 10, 1, n_out=200)
    assert rc == E.E_INVALID and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufs, bufx, beyond_y, 10, 1, n_out=200)
    assert rc == E.E_INVALID and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufx, bufs, [(0, 50), (short - 100, 100)], 10, 1, n_out=200)  # (up to Y's end: served)
    assert rc == 0 and not np.any(out[: 6 * 132] == SENT) and np.all(out[6 * 132:] == SENT)
    other = A.Context(0)
    dpx, dpy, dps, dpo = A.DPlan(ctx, xr), A.DPlan(ctx, yr), A.DPlan(ctx, sr), A.DPlan(other, yr)
    bx, by, bs = (_on_device(torch, r) for r in (xr, yr, sr))
    try:
        for rg, w, s, what in cases:
            rc, clean = _raw_dev(A, torch, ctx, dpx, bx, dpy, by, rg, w, s)
            assert rc == E.E_INVALID and clean, (rg, w, s, rc)
        for px, b1, py, b2 in ((dpx, bx, dps, bs), (dps, bs, dpx, bx)):
            rc, clean = _raw_dev(A, torch, ctx, px, b1, py, b2, beyond_y, 10, 1)
            assert rc == E.E_INVALID and clean, rc
            assert E.lib().atsc_ctx_last_error(ctx._h).decode() == "rolling_pair_windows: window beyond the stream"
        rc, clean = _raw_dev(A, torch, ctx, dpx, bx, dpo, by, [(0, 100)], 10, 1)  # plans of two contexts
        assert rc == E.E_INVALID and clean
        assert E.lib().atsc_ctx_last_error(ctx._h).decode() == "rolling_pair_windows: plans of different contexts"
        rc, clean = _raw_dev(A, torch, ctx, dpx, bx, dpy, by, [], 5, 1)
        assert rc == 0 and clean
        rc, clean = _raw_dev(A, torch, ctx, dpx, bx, dpy, by, [(5, 0), (LONG, 0), (7, 4)], 5, 1)  # no range holds a window
        assert rc == 0 and clean
    finally:
        for d in (dpx, dpy, dps, dpo):
            d.close()
        other.close()
    sx = A.CompressedStream.from_bytes(ctx, A.compress_data(ctx, np.arange(1000.0), A.NOOP, 0))
    sy = A.CompressedStream.from_bytes(ctx, A.compress_data(ctx, np.arange(900.0), A.NOOP, 0))
    for b, c, w in (([0], [100], 0), ([850], [100], 10)):
        with pytest.raises(A.AtscError) as e:
            sx.rolling_pair_windows(sy, b, c, w, 1)
        assert e.value.rc == E.E_INVALID
    got, off = sx.rolling_pair_windows(sy, [800], [100], 10, 1)
    assert len(got) == 91 and np.all(got["count"] == 10) and np.all(got["mean_x"] == got["mean_y"])
    rc, out = _raw_host(A, ctx, bufx, bufy, [], 5, 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufx, bufy, [(5, 0), (LONG, 0), (7, 4)], 5, 1)  # no range holds a window: no record
    assert rc == 0 and np.all(out == SENT)


def test_malformed_payload_in_either_stream(A, ctx, torch):
    n, nf = 256, 8
    x = H.synth_series(909, n * nf, klass=2)
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
    orecs, other = _noop(A, ctx, np.round(H.synth_series(910, n * nf + 300, klass=1) * 100.0))
    bb, ob = np.frombuffer(bad, dtype=np.uint8), np.frombuffer(orecs, dtype=np.uint8)
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 20, 20), (5 * n + 3, 100), (3 * n + 5, 0)]
    b, c = [w[0] for w in outside], [w[1] for w in outside]
    for in_x in (True, False):
        rx, ry, fx, fy = (bad, orecs, good, other) if in_x else (orecs, bad, other, good)
        P = M.Pyramid(fx, fy)
        got, _ = ctx.rolling_pair_windows_host(rx, ry, b, c, 20, 3)
        _assert_same(got, P.rolling(b, c, 20, 3)[0], ("outside", in_x))
        ux, uy = (bb, ob) if in_x else (ob, bb)
        for rg in ([(3 * n, 20)], [(0, nf * n)], [(0, 40), (3 * n - 19, 20)], [(4 * n - 20, 20), (6 * n, 50)]):
            rc, out = _raw_host(A, ctx, ux, uy, rg, 20, 1, n_out=nf * n)
            assert rc == A.capi.E_FORMAT and np.all(out == SENT), (rg, rc, in_x)
        # The device call sets the status word of the plan the payload belongs to; the word has no accessor (see
        # tests/test_gpu_rolling_moments.py): the host call above is what shows it.  The device call returns ATSC_OK,
        # finishes, writes every record, and gives the ranges beside the bad frame their right records.
        dpx, dpy = A.DPlan(ctx, rx), A.DPlan(ctx, ry)
        try:
            rg = [(0, 3 * n), (3 * n + 7, 40), (4 * n, 100)]
            b2, c2 = [w[0] for w in rg], [w[1] for w in rg]
            want, woff = P.rolling(b2, c2, 20, 1)
            got, rest, _ = _dev(A, torch, dpx, _on_device(torch, rx), dpy, _on_device(torch, ry), b2, c2, 20, 1, len(want))
            assert not (got.view(np.uint64) == SENT).any() and np.all(rest == SENT)
            clean = np.r_[0: int(woff[1]), int(woff[2]): int(woff[3])]
            _assert_same(got[clean], want[clean], ("dev, beside the bad frame", in_x))
        finally:
            dpx.close()
            dpy.close()


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


HEAD_M = ",nonnan,avg,stdvar,stddev,slope,intercept"
HEAD_P = ",pair_count,covariance,correlation,slope,intercept"


def test_command_line(A, ctx, golden_dir, tmp_path):
    atsc = os.path.join(os.path.dirname(A.__file__), "bin", "atsc")
    wbro = open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read()
    (tmp_path / "o").mkdir()
    for path, e in ((tmp_path / "uptime.wbro", "1"), (tmp_path / "o" / "other.wbro", "3")):
        path.write_bytes(wbro)
        _run(atsc, "--compressor", "fft", "-e", e, path)
    bro, other = (tmp_path / "uptime.bro").read_bytes(), (tmp_path / "o" / "other.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    assert len(A.decompress_data(ctx, other)) == len(full)
    out = tmp_path / "uptime.roll.csv"
    pair = ("--rolling-pair", tmp_path / "o" / "other.bro")
    for spec, (b0, c0), (w, s) in (("20", (0, len(full)), (20, 1)), ("300:15", (100, 1500), (300, 15))):
        texts = []
        for flags in ((), ("--rolling-moments",), pair, ("--rolling-moments",) + pair, ()):
            _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--rolling", spec, *flags, tmp_path / "uptime.bro")
            texts.append(out.read_text())
        assert texts[0] == texts[4]  # the files of calls without the flag are what they were
        base, ml, pl, bl = (t.split("\n") for t in texts[:4])
        want, _ = A.rolling_pair_data_windows(ctx, bro, other, [b0], [c0], w, s)
        fit = A.pair_fit(want)
        assert len(want) == M.outputs(c0, w, s) > 0
        assert base[0] == "offset,count,min,max,sum,mean" and ml[0] == base[0] + HEAD_M
        assert pl[0] == base[0] + HEAD_P and bl[0] == base[0] + HEAD_M + HEAD_P
        assert len(base) == len(ml) == len(pl) == len(bl) == len(want) + 2 and base[-1] == ""
        for j in range(len(want)):
            cells = pl[1 + j].split(",")
            assert len(cells) == 11 and ",".join(cells[:6]) == base[1 + j]  # the plain columns, byte for byte
            assert bl[1 + j] == ml[1 + j] + "," + ",".join(cells[6:])  # last, behind the moments' columns
            assert int(cells[6]) == want["count"][j]
            if want["count"][j] == 0:
                assert cells[7:] == [""] * 4
                continue
            for cell, k in zip(cells[7:], ("covariance", "correlation", "slope", "intercept")):
                v, e = float(cell), float(fit[k][j])
                assert (math.isnan(v) and math.isnan(e)) or np.float64(v).tobytes() == np.float64(e).tobytes(), (j, k, cell, e)
    for bad in (("-u",) + pair, ("-u", "--samples", "0:10") + pair, ("-u", "--samples", "0:10", "--buckets", "5") + pair):
        r = subprocess.run([atsc, *[str(a) for a in bad], str(tmp_path / "uptime.bro")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "'--rolling-pair' needs '--rolling'" in r.stderr, bad
    # an OTHER that ends before a window fails, as --pair's does
    short = tmp_path / "o" / "short.bro"
    short.write_bytes(A.compress_data(ctx, np.arange(50.0), A.NOOP, 0))
    r = subprocess.run([atsc, "-u", "--samples", "0:100", "--rolling", "20", "--rolling-pair", str(short), str(tmp_path / "uptime.bro")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    # csv-compressor does not take the flag
    csvc = os.path.join(os.path.dirname(A.__file__), "bin", "csv-compressor")
    r = subprocess.run([csvc, "-u", "--rolling", "20", "--rolling-pair", str(short), str(tmp_path / "uptime.bro")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2
