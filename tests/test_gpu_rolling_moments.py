"""Windowed rolling moments on the GPU: every record of every case against the NumPy model of the contract
(tests/rolling_moments_model.py) applied to the GPU's own full decode: count exactly, each double bit for bit, except that
where the model's value is NaN any NaN conforms (the main stream holds +-Inf Constant records).  The main stream is the
rolling suite's (every frame-length tier below the large one under every codec, one large frame, Constant records of NaN,
+-Inf and zeros of both signs); Noop streams of mixed magnitudes 1e3 .. 1e17, where every merge rounds, serve the widths
across the 2^16 and the 2^18 level and the budgets that cut a range into pieces; an integer counter with NaN holes takes
the general rule inside chunks, the NaN-free streams the equal-count path.  Against atsc_moments_windows_dev on the
listed windows; the host, device and stream calls; a rolling, a rolling delta and a rolling moments call on one plan;
errors that leave the result untouched; a malformed payload; both command lines."""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import helpers as H
from tests import moments_model as MM
from tests import rolling_delta_model as DM
from tests import rolling_model as RM
from tests import rolling_moments_model as M
from tests.test_gpu_rolling import CONSTANTS, LENS, _const_record, _fft_record, _rec

pytestmark = pytest.mark.gpu

# around the lowest stored level (8), the wavefront (64), the tile (2048) and the first upper launch (4096)
WIDTHS = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 64, 65, 300, 2048, 2049, 4096, 4097]
LONG = 200000
SENT = 0x5A5A5A5A5A5A5A5A
DOUBLES = M.FIELDS[1:]


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
    """-> (records, full decode, model pyramid, first sample of the Constant records), built as the rolling suite's"""
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
    return recs, full, M.Pyramid(full), at


def _noop_records(A, ctx, x):
    """Noop frames of 4096: cheap to build and to decode; Noop stores 64-bit integers, so x holds integers"""
    return ctx.compress_host(x, H.frame_offsets(len(x), 4096), A.NOOP, False, 0.0, 0)[0]


def _wide(rng, n):
    """n integers of the magnitudes 1e3 .. 1e17, both signs: Noop stores them as they are, and every merge of their
    nodes rounds"""
    return np.round(rng.normal(0, 1, n) * 10.0 ** rng.integers(3, 18, n))


def _noop(A, ctx, x):
    recs = _noop_records(A, ctx, x)
    full = ctx.decompress_host(recs)
    assert np.array_equal(full, x)
    return recs, full, M.Pyramid(full)


@pytest.fixture(scope="module")
def long(A, ctx):
    """200000 integers of mixed magnitude in Noop frames, no NaN: every merge inside a chunk joins equal counts"""
    return _noop(A, ctx, _wide(np.random.default_rng(23), LONG))


@pytest.fixture(scope="module")
def counter(A, ctx):
    """an integer counter with resets, stored as Noop, with NaN holes (Constant records of NaN between the Noop frames):
    chunks over a hole merge unequal counts"""
    rng = np.random.default_rng(29)
    n = 30000
    x = np.cumsum(rng.integers(0, 51, n).astype(np.float64)) + 1000.0
    for r in np.flatnonzero(rng.random(n) < 0.003):
        x[r:] -= x[r] - float(rng.integers(0, 20))
    assert x.min() >= 0 and x.max() < 2 ** 40
    recs, want = b"", []
    for seg, hole in ((x[:9000], 1), (x[9000:9001], 2), (x[9001:21000], 3), (x[21000:21005], 70), (x[21005:], 0)):
        recs += _noop_records(A, ctx, seg) + (_const_record(A, ctx, np.nan, hole) if hole else b"")
        want += [seg, np.full(hole, np.nan)]
    full = ctx.decompress_host(recs)
    assert np.array_equal(full, np.concatenate(want), equal_nan=True)
    return recs, full, M.Pyramid(full)


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


def _ranges(total, w, at):
    """the rolling suite's shapes: ranges that begin at odd and at aligned indices, overlap, come unsorted, are shorter
    than w, equal w, empty, lie over the Constant records, and (last) span the whole stream"""
    r = [(4096, min(3 * w + 700, total - 4096)), (1, min(2 * w + 33, total - 1)), (2047, w), (2048, w - 1), (777, 0),
         (total - w, w), (max(at - w - 5, 0), min(2 * w + 3200, total - max(at - w - 5, 0))),
         (6001, min(w + 900, total - 6001)), (total, 0), (0, total)]
    return [x for x in r if x[0] + x[1] <= total]


@pytest.mark.parametrize("w", WIDTHS)
def test_every_record_matches_the_model(A, ctx, main, w):
    recs, full, P, at = main
    for s in (1, 7, w, 2 * w + 1):
        rg = _ranges(len(full), w, at)
        if s > 7:
            rg = rg[:-1] + [(3, len(full) - 3)]
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_moments_windows_host(recs, b, c, w, s)
        want, woff = P.rolling(b, c, w, s)
        assert off.tolist() == woff.tolist() and got.dtype == A.WINDOW_MOMENTS
        assert off[3] == off[4] == off[5] and off[3] - off[2] == 1  # shorter than w: none; equal w: one
        _assert_same(got, want, (w, s))
        if s == 1:  # the 3000 NaN give empty windows, two +Inf in a window a NaN m2 beside a count
            assert np.isnan(got["mean"][got["count"] == 0]).all() and ((got["count"] == 0).any() or w > 3000)
            assert (np.isnan(got["m2"]) & (got["count"] > 0)).any() or w == 1


def test_width_across_the_65536_level(A, ctx, torch, long):
    recs, full, P = long
    w = 70001
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        for s, rg in ((1, [(0, LONG)]), (7, [(65535, LONG - 65535), (1, 140003)]), (w, [(3, LONG - 3)]),
                      (2 * w + 1, [(0, LONG), (60000, w)])):
            b, c = [x[0] for x in rg], [x[1] for x in rg]
            want, woff = P.rolling(b, c, w, s)
            d = torch.full((6 * len(want) + 6,), SENT, dtype=torch.int64, device="cuda")
            off = dp.rolling_moments_windows(body, b, c, w, s, d, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            h = d.cpu().numpy()
            assert off.tolist() == woff.tolist() and np.all(h[6 * len(want):] == SENT)
            _assert_same(h[: 6 * len(want)].view(A.WINDOW_MOMENTS), want, (w, s))
    finally:
        dp.close()


def test_width_across_the_262144_level(A, ctx):
    """w = 2^18 + 1: the chunks of level 18 come from the second launch of the upper kernel.  In the longer stream the
    windows at 2^18 - 1 and 2^18 read the one at 2^18, which no window of the first stream holds"""
    w = (1 << 18) + 1
    n = (1 << 18) + 5000
    rng = np.random.default_rng(31)
    recs, full, P = _noop(A, ctx, _wide(rng, n))
    got, off = ctx.rolling_moments_windows_host(recs, [0], [n], w, 1)
    want, woff = P.rolling([0], [n], w, 1)
    assert off.tolist() == woff.tolist() == [0, n - w + 1]
    _assert_same(got, want, w)
    recs, full, P = _noop(A, ctx, _wide(rng, (1 << 19) + 16))
    lo = (1 << 18) - 3
    reads = [M.chunks(lo + j, w) for j in range(7)]
    assert [max(l for _, l in c) for c in reads] == [17, 17, 18, 18, 17, 17, 17]
    assert all((1 << 18, 18) in reads[j] for j in (2, 3))
    got, off = ctx.rolling_moments_windows_host(recs, [lo], [w + 6], w, 1)
    _assert_same(got, P.rolling([lo], [w + 6], w, 1)[0], (w, "level 18 read"))


def _listed_dev(A, ctx, torch, recs, lo, w):
    """atsc_moments_windows_dev over the listed windows (lo[i], w)"""
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        d = torch.zeros(6 * len(lo), dtype=torch.int64, device="cuda")
        dp.moments_windows(body, lo, np.full(len(lo), w), d, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d.cpu().numpy().view(A.WINDOW_MOMENTS)
    finally:
        dp.close()


def _within_both_bounds(full, lo, w, mine, theirs, label):
    """each double of `mine` (the rolling moments') against `theirs` (the windowed moments') of the window (lo, w): within
    the sum of the two calls' stated bounds, whose scales are the window's exact moments (rational arithmetic)"""
    en, emean, em2, _, et_m2, _, eabs = MM.exact_moments(full[lo:lo + w])
    r = (lo + w) / w
    a, b = M.bounds(w, en, emean, em2, et_m2), MM.bounds(en, emean, em2, et_m2)
    lims = {"mean": (a[0] + b[0]) * float(eabs), "m2": a[1] + b[1], "t_mean": (a[0] + b[0]) * (lo + w),
            "t_m2": r * (a[2] + b[2]), "c_tx": r * (a[3] + b[3])}
    for k in DOUBLES:
        assert abs(Fraction(float(mine[k])) - Fraction(float(theirs[k]))) <= lims[k], (label, lo, k, mine[k], theirs[k], lims[k])


def test_against_the_windowed_moments_on_the_listed_windows(A, ctx, torch, main, counter):
    """count exactly on every listed window; the doubles, which come from another tree, within the two bounds where the
    window's samples are finite -- on every 1 + len // 40-th window, exact arithmetic being what the bounds are stated in"""
    recs, full, P, at = main
    total = len(full)
    for w, s in ((1, 1), (2, 1), (3, 1), (65, 3), (300, 7), (2049, 5), (4097, 11)):
        rg = [(max(at - w - 40, 0), min(2 * w + 5300, total - max(at - w - 40, 0))), (1, min(w + 2000, total - 1))]
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_moments_windows_host(recs, b, c, w, s)
        lo = np.concatenate([rg[i][0] + s * np.arange(int(off[i + 1] - off[i])) for i in range(len(rg))])
        ref = _listed_dev(A, ctx, torch, recs, lo, w)
        assert got["count"].tobytes() == ref["count"].tobytes(), (w, s)
        checked = 0
        for i in range(0, len(lo), 1 + len(lo) // 40):
            v = full[int(lo[i]):int(lo[i]) + w]
            if got["count"][i] and np.isfinite(v[~np.isnan(v)]).all():
                _within_both_bounds(full, int(lo[i]), w, got[i], ref[i], (w, s))
                checked += 1
        assert checked >= 10, (w, s, checked)
    crecs, cfull, CP = counter
    for w, s in ((2, 1), (9, 1), (300, 7), (4097, 3)):
        got, off = ctx.rolling_moments_windows_host(crecs, [1, 0], [len(cfull) - 1, 3 * w], w, s)
        lo = np.concatenate([1 + s * np.arange(int(off[1])), s * np.arange(int(off[2] - off[1]))])
        ref = _listed_dev(A, ctx, torch, crecs, lo, w)
        assert got["count"].tobytes() == ref["count"].tobytes(), (w, s)
        for i in range(0, len(lo), 1 + len(lo) // 40):
            if got["count"][i]:
                _within_both_bounds(cfull, int(lo[i]), w, got[i], ref[i], ("counter", w, s))


def test_nan_holes_take_the_general_rule_and_nan_free_chunks_the_equal_count_path(A, ctx, counter, long):
    crecs, cfull, CP = counter
    n = len(cfull)
    for w, s in ((2, 1), (3, 1), (8, 1), (9, 1), (64, 1), (65, 3), (300, 7), (2049, 5), (4097, 3)):
        b, c = [0, 8990, 20990], [n, min(2 * w + 40, n - 8990), min(w + 200, n - 20990)]
        got, off = ctx.rolling_moments_windows_host(crecs, b, c, w, s)
        _assert_same(got, CP.rolling(b, c, w, s)[0], ("counter", w, s))
        assert int(got["count"].min()) < w and int(got["count"].max()) == w  # holes inside, and whole windows
        if w <= 64:
            assert int(got["count"].min()) == 0 and np.isnan(got["c_tx"][got["count"] == 0]).all()  # the hole of 70
    recs, full, P = long
    for w, s in ((8, 1), (64, 1), (2048, 1), (4096, 3)):
        b, c = [0, 4096, 12345], [3 * w + 5000, 2 * w, w + 77]
        got, off = ctx.rolling_moments_windows_host(recs, b, c, w, s)
        _assert_same(got, P.rolling(b, c, w, s)[0], ("long", w, s))
        assert np.all(got["count"] == w)
    # a constant window: no spread and no trend, exactly
    flat = _noop_records(A, ctx, np.full(10000, 123456789.0))
    got, _ = ctx.rolling_moments_windows_host(flat, [0, 3], [10000, 9000], 2049, 5)
    assert np.all(got["m2"] == 0.0) and np.all(got["c_tx"] == 0.0) and np.all(got["mean"] == 123456789.0)
    assert np.all(got["t_m2"] > 0.0) and len(got) == 1591 + 1391


def test_host_device_and_stream_calls_agree(A, ctx, torch):
    x = H.synth_series(3170, 50000, block=7000)
    x[12345:12400] = np.nan
    bro = A.compress_data(ctx, x, A.AUTO, 3)
    full = A.decompress_data(ctx, bro)
    P = M.Pyramid(full)
    n0, p0 = H.varint_decode(bro, 9)
    body = torch.from_numpy(np.frombuffer(bro[p0:], dtype=np.uint8).copy()).to("cuda")
    dp = A.DPlan(ctx, bro[p0:])
    st = A.CompressedStream.from_bytes(ctx, bro)
    try:
        for w, s in ((300, 1), (65, 7), (4097, 3)):
            b, c = [30001, 20000, 47000], [15000, 12001, 100]  # begins far into the stream: the host call uploads a part
            want, woff = P.rolling(b, c, w, s)
            via_bro, off = A.rolling_moments_data_windows(ctx, bro, b, c, w, s)
            _assert_same(via_bro, want, (w, s))
            assert off.tolist() == woff.tolist()
            host, _ = ctx.rolling_moments_windows_host(bro[9:], b, c, w, s, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), (w, s)
            assert st.rolling_moments_windows(b, c, w, s)[0].tobytes() == via_bro.tobytes(), (w, s)
            d = torch.zeros(6 * len(want) + 1, dtype=torch.int64, device="cuda")
            dp.rolling_moments_windows(body, b, c, w, s, d, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert d.cpu().numpy()[: 6 * len(want)].tobytes() == via_bro.tobytes(), (w, s)
            fit = A.moments_fit(via_bro)  # the records are the windowed moments': the fit applies as it is
            assert len(fit) == len(want) and np.isfinite(fit["slope"][via_bro["count"] > 1]).all()
    finally:
        dp.close()


def test_the_three_rolling_calls_share_the_plans_place(A, ctx, torch, long):
    """the rolling, the rolling delta and the rolling moments call keep their tables and scratch in one place of the plan:
    enqueued one after the other without a synchronisation in between, each gives its own bytes"""
    recs, full, P = long
    RP, DP = RM.Pyramid(full), DM.Pyramid(full)
    b, c, w, s = [5, 100000], [90000, 30000], 3000, 3
    want_r, off = RP.rolling(b, c, w, s)
    n = len(want_r)
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        r1, r2 = (torch.full((4 * n,), SENT, dtype=torch.int64, device="cuda") for _ in range(2))
        d1 = torch.full((8 * n,), SENT, dtype=torch.int64, device="cuda")
        m1, m2 = (torch.full((6 * n,), SENT, dtype=torch.int64, device="cuda") for _ in range(2))
        q = torch.cuda.current_stream().cuda_stream
        dp.rolling_moments_windows(body, b, c, w, s, m1, q)
        dp.rolling_windows(body, b, c, w, s, r1, q)
        dp.rolling_moments_windows(body, b, c, w + 2, s, m2, q)  # (another width: other level tables in the same place)
        dp.rolling_delta_windows(body, b, c, w + 1, s, d1, q)
        dp.rolling_windows(body, b, c, w, s, r2, q)
        torch.cuda.synchronize()
        first, second = r1.cpu().numpy(), r2.cpu().numpy()
        assert first.tobytes() == second.tobytes() == ctx.rolling_windows_host(recs, b, c, w, s)[0].tobytes()
        a = first.view(A.WINDOW_ROLLING)
        assert a["count"].tolist() == want_r["count"].tolist() and a["sum"].tobytes() == want_r["sum"].tobytes()
        _assert_same(m1.cpu().numpy().view(A.WINDOW_MOMENTS), P.rolling(b, c, w, s)[0], "in front of a rolling call")
        want_m2, _ = P.rolling(b, c, w + 2, s)
        assert 0 < len(want_m2) <= n
        _assert_same(m2.cpu().numpy()[: 6 * len(want_m2)].view(A.WINDOW_MOMENTS), want_m2, "between the two others")
        want_d1, _ = DP.rolling(b, c, w + 1, s)
        assert 0 < len(want_d1) <= n
        assert d1.cpu().numpy()[: 8 * len(want_d1)].tobytes() == want_d1.tobytes()
    finally:
        dp.close()


def _pieces(n, budget, w):
    """the pieces of a range of n samples from sample 0 of a stream without large frames under a budget, by DESIGN.md's
    piece arithmetic: a region of Lr = max(65536, 8 / 20 of budget / 8 rounded down to 2048) samples, a piece of
    Lr - 3 * 2048, consecutive pieces overlapping by w - 1"""
    lp = max(65536, budget // 8 * 8 // 20 // 2048 * 2048) - 3 * 2048
    k, p = 1, 0
    while p + lp < n:
        p, k = p + lp - (w - 1), k + 1
    return k


def test_pieces_do_not_change_the_bytes(A, ctx, long, main):
    recs, full, P = long
    b, c = [0, 90001], [LONG, 30000]
    two, three = 110592 * 20, 1
    try:
        for w in (3000, 50000):  # the second: close to the least budget's piece of 59392, which then advances by 9393
            ref, _ = ctx.rolling_moments_windows_host(recs, b, c, w, 1)
            _assert_same(ref, P.rolling(b, c, w, 1)[0], "default")
            assert _pieces(LONG, two, w) == (2 if w == 3000 else 3) and _pieces(LONG, three, w) >= (3 if w == 3000 else 15)
            for budget in (two, three):
                ctx.set_aggregate_scratch(budget)
                got, _ = ctx.rolling_moments_windows_host(recs, b, c, w, 1)
                assert got.tobytes() == ref.tobytes(), (w, budget)
                if w == 3000:
                    got7, _ = ctx.rolling_moments_windows_host(recs, b, c, w, 7)
                    assert got7.tobytes() == ref[: LONG - w + 1][::7].tobytes() + ref[LONG - w + 1:][::7].tobytes(), budget
            ctx.set_aggregate_scratch(0)
        # the main stream under the least budget: a large frame across the pieces' ends
        mrecs, mfull, MP, _ = main
        ctx.set_aggregate_scratch(1)
        got, _ = ctx.rolling_moments_windows_host(mrecs, [0], [len(mfull)], 3000, 1)
    finally:
        ctx.set_aggregate_scratch(0)
    assert len(mfull) > 65536
    _assert_same(got, MP.rolling([0], [len(mfull)], 3000, 1)[0], "main, least budget")


def _raw_host(A, ctx, buf, rg, w, s, n_out=16):
    out = np.full(6 * n_out, SENT, dtype=np.uint64)
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    rc = A.capi.lib().atsc_rolling_moments_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(rg),
                                                   b.ctypes.data_as(p), c.ctypes.data_as(p), w, s, C.c_void_p(out.ctypes.data))
    return rc, out


def test_capacity_message_names_a_budget_that_serves(A, ctx, long):
    recs, full, P = long
    buf = np.frombuffer(recs, dtype=np.uint8)
    E = A.capi
    try:
        ctx.set_aggregate_scratch(1)
        rc, out = _raw_host(A, ctx, buf, [(0, 70010)], 70001, 1)
        assert rc == E.E_CAPACITY and np.all(out == SENT)
        msg = E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert msg.startswith("rolling_moments_windows: a window of 70001 samples"), msg
        need = int(msg.split("budget of ")[1].split(" bytes")[0])
        assert need == (70001 + 4 * 2048) * 20  # 8 bytes a sample and 12 of chunk partials; no large frame: no spill
        ctx.set_aggregate_scratch(need)
        rc, out = _raw_host(A, ctx, buf, [(0, 70010)], 70001, 1)
        assert rc == 0 and np.all(out[60:] == SENT)
        _assert_same(out[:60].view(A.WINDOW_MOMENTS), P.rolling([0], [70010], 70001, 1)[0], "the named budget")
        ctx.set_aggregate_scratch(1)
        rc, out = _raw_host(A, ctx, buf, [(0, 59392 + 15)], 59392, 1)  # the widest that the least budget holds
        assert rc == 0 and np.all(out[96:] == SENT)
        _assert_same(out[:96].view(A.WINDOW_MOMENTS), P.rolling([0], [59392 + 15], 59392, 1)[0], "widest")
        rc, out = _raw_host(A, ctx, buf, [(0, 59393 + 15)], 59393, 1)
        assert rc == E.E_CAPACITY and np.all(out == SENT)
    finally:
        ctx.set_aggregate_scratch(0)
    rc, out = _raw_host(A, ctx, buf, [(0, 70010)], 70001, 1)  # the default budget holds any width
    assert rc == 0 and np.all(out[60:] == SENT) and not np.any(out[:60] == SENT)


def test_errors_leave_the_result_untouched(A, ctx, torch, long):
    recs, full, P = long
    buf = np.frombuffer(recs, dtype=np.uint8)
    E = A.capi
    cases = [([(0, 100)], 0, 1, "width outside"), ([(0, 100)], A.ROLLING_MAX_WIDTH + 1, 1, "width outside"),
             ([(0, 100)], 10, 0, "stride is 0"), ([(LONG - 50, 100)], 10, 1, ""), ([(0, 20), (LONG + 1, 0)], 10, 1, ""),
             ([(2 ** 63, 2 ** 63)], 10, 1, ""), ([(0, 2 ** 33)], 1, 1, "")]
    for rg, w, s, what in cases:
        rc, out = _raw_host(A, ctx, buf, rg, w, s)
        msg = E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert rc == E.E_INVALID and np.all(out == SENT), (rg, w, s, rc)
        assert not what or msg.startswith("rolling_moments_windows: " + what), msg  # the call's own checks name the call
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(buf.copy()).to("cuda")
    try:
        for rg, w, s, what in cases:
            d = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
            b = np.array([x[0] for x in rg], dtype=np.uint64)
            c = np.array([x[1] for x in rg], dtype=np.uint64)
            p = C.POINTER(C.c_uint64)
            rc = E.lib().atsc_rolling_moments_windows_dev(ctx._h, dp._h, C.c_void_p(body.data_ptr()), len(rg), b.ctypes.data_as(p),
                                                          c.ctypes.data_as(p), w, s, C.c_void_p(d.data_ptr()),
                                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            assert rc == E.E_INVALID and bool((d == SENT).all()), (rg, w, s, rc)
    finally:
        dp.close()
    st = A.CompressedStream.from_bytes(ctx, A.compress_data(ctx, np.arange(1000.0), A.NOOP, 0))
    with pytest.raises(A.AtscError) as e:
        st.rolling_moments_windows([0], [100], 0, 1)
    assert e.value.rc == E.E_INVALID
    rc, out = _raw_host(A, ctx, buf, [], 5, 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, buf, [(5, 0), (LONG, 0), (7, 4)], 5, 1)  # no range holds a window: no record
    assert rc == 0 and np.all(out == SENT)


def test_malformed_payload(A, ctx, torch):
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
    P = M.Pyramid(good)
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 20, 20), (5 * n + 3, 100), (3 * n + 5, 0)]
    b, c = [w[0] for w in outside], [w[1] for w in outside]
    got, _ = ctx.rolling_moments_windows_host(bad, b, c, 20, 3)
    _assert_same(got, P.rolling(b, c, 20, 3)[0], "outside")
    bb = np.frombuffer(bad, dtype=np.uint8)
    for rg in ([(3 * n, 20)], [(0, nf * n)], [(0, 40), (3 * n - 19, 20)], [(4 * n - 20, 20), (6 * n, 50)]):
        rc, out = _raw_host(A, ctx, bb, rg, 20, 1, n_out=nf * n)
        assert rc == A.capi.E_FORMAT and np.all(out == SENT), (rg, rc)
    # The device call sets the plan's status word.  The word has no accessor in the C ABI or the Python surface (see
    # tests/test_gpu_histogram.py): the host call above, which is the device call on a plan of the touched records
    # followed by a read of the plan's word, is what shows it.  The device call itself returns ATSC_OK, finishes, writes
    # every record, and gives the ranges beside the bad frame their right records.
    dp = A.DPlan(ctx, bad)
    body = torch.from_numpy(bb.copy()).to("cuda")
    try:
        rg = [(0, 3 * n), (3 * n + 7, 40), (4 * n, 100)]
        b, c = [w[0] for w in rg], [w[1] for w in rg]
        want, off = P.rolling(b, c, 20, 1)
        d = torch.full((6 * len(want),), SENT, dtype=torch.int64, device="cuda")
        dp.rolling_moments_windows(body, b, c, 20, 1, d, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        h = d.cpu().numpy()
        assert not (h.view(np.uint64) == SENT).any()
        clean = np.r_[0: int(off[1]), int(off[2]): int(off[3])]
        _assert_same(h.view(A.WINDOW_MOMENTS)[clean], want[clean], "dev, beside the bad frame")
    finally:
        dp.close()


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


HEAD_D = ",pairs,rises,falls,up,down,after_falls,max_rise,max_fall,increase"
HEAD_M = ",nonnan,avg,stdvar,stddev,slope,intercept"


def _check_rows(A, plain, deltas, moments, both, first, want):
    """the .roll.csv of one call without a flag, with --rolling-deltas, with --rolling-moments and with both.  The
    rolling's columns are the plain file's, byte for byte; the moments' columns come last, behind the deltas' where
    both are given, and parse back to `want`'s count and to what atsc_moments_fit reads off `want`"""
    base, dl, ml, bl = (t.split("\n") for t in (plain, deltas, moments, both))
    assert base[0] == first + ",count,min,max,sum,mean" and dl[0] == base[0] + HEAD_D
    assert ml[0] == base[0] + HEAD_M and bl[0] == base[0] + HEAD_D + HEAD_M
    assert len(base) == len(dl) == len(ml) == len(bl) == len(want) + 2 and base[-1] == ""
    fit = A.moments_fit(want)
    for j in range(len(want)):
        cells = ml[1 + j].split(",")
        assert len(cells) == 12 and ",".join(cells[:6]) == base[1 + j]
        assert bl[1 + j] == dl[1 + j] + "," + ",".join(cells[6:])  # behind the deltas' columns, which are what they were
        if want["count"][j] == 0:
            assert cells[6:] == [""] * 6
            continue
        assert int(cells[6]) == want["count"][j]
        for cell, k in zip(cells[7:], ("mean", "variance", "stddev", "slope", "intercept")):
            v, e = float(cell), float(fit[k][j])
            assert (math.isnan(v) and math.isnan(e)) or np.float64(v).tobytes() == np.float64(e).tobytes(), (j, k, cell, e)


def _four(run, out):
    """the .roll.csv of `run(flags)` for no flag, each flag and both; the flagless run once more at the end"""
    texts = []
    for flags in ((), ("--rolling-deltas",), ("--rolling-moments",), ("--rolling-deltas", "--rolling-moments"), ()):
        run(flags)
        texts.append(out.read_text())
    assert texts[0] == texts[4]
    return texts[:4]


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
    hi = len(times) - 3
    for (t0, t1), spec, (w, s) in (((times[10], times[hi]), "20:3", (20, 3)), ((times[10], times[12]), "20", (20, 1))):
        for f in tmp_path.glob("win*"):
            f.unlink()
        texts = _four(lambda flags: _run(csvc, "-u", "--from", t0, "--to", t1, "--rolling", spec, *flags, "-o", tmp_path / "win",
                                         tmp_path / "cpu.bro"), tmp_path / "win.roll.csv")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.roll.csv"]
        at = np.flatnonzero((times >= t0) & (times <= t1))
        want, _ = A.rolling_moments_data_windows(ctx, cbro, [int(at[0])], [len(at)], w, s)
        assert len(want) == M.outputs(len(at), w, s)
        _check_rows(A, *texts, "timestamp", want)
    r = subprocess.run([csvc, "-u", "--from", str(times[10]), "--to", str(times[hi]), "--rolling-moments", str(tmp_path / "cpu.bro")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "'--rolling-moments' needs '--rolling'" in r.stderr


def test_command_line(A, ctx, golden_dir, tmp_path):
    atsc = os.path.join(os.path.dirname(A.__file__), "bin", "atsc")
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    for spec, (b0, c0), (w, s) in (("20", (0, len(full)), (20, 1)), ("300:15", (100, 1500), (300, 15))):
        texts = _four(lambda flags: _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--rolling", spec, *flags,
                                         tmp_path / "uptime.bro"), tmp_path / "uptime.roll.csv")
        want, _ = A.rolling_moments_data_windows(ctx, bro, [b0], [c0], w, s)
        assert len(want) == M.outputs(c0, w, s) > 0
        _check_rows(A, *texts, "offset", want)
    for bad in (("-u", "--rolling-moments"), ("-u", "--samples", "0:10", "--rolling-moments"),
                ("-u", "--samples", "0:10", "--buckets", "5", "--rolling-moments")):
        r = subprocess.run([atsc, *bad, str(tmp_path / "uptime.bro")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "'--rolling-moments' needs '--rolling'" in r.stderr, bad
