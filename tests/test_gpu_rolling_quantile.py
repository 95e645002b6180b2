"""Windowed rolling quantiles on the GPU: every row of every case against the NumPy model of the contract
(tests/rolling_quantile_model.py) applied to the GPU's own full decode, bit for bit, except that where the model's value
is NaN any NaN conforms.  The streams are the rolling suite's: the main stream (every frame-length tier below the large
one under every codec, one large frame, Constant records of NaN, +-Inf and zeros of both signs), a Noop stream of 200000
integers, an integer counter with NaN holes; an RLE stream of values rounded to multiples of 8 brings the ties.  The
widths stand either side of the wavefront, of the windowed quantiles' tiers and of every threshold of the rule that
sizes a task (P = 512 .. 8192 at w = 256, 512, 1024, 2048); a case holds at most 2^25 positions x width.  Against
atsc_quantile_windows_dev on the listed windows; pieces under the least budget; one plan shared with a rolling and a
windowed quantile call; the host, device and stream calls; errors that leave the result untouched; a malformed payload;
both command lines."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import rolling_model as RM
from tests import rolling_quantile_model as M
from tests.test_gpu_rolling import CONSTANTS, LENS, _const_record, _fft_record, _rec

pytestmark = pytest.mark.gpu

# the issue's widths, and 511 .. 513 and 1023 .. 1025 beside 255 .. 257 and 2047 .. 2049: the thresholds of span_keys
WIDTHS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
          8191, 8192]
LONG = 200000
SENT = 0x5A5A5A5A5A5A5A5A
L1 = [0.5]
L3 = [1.0, 0.0, 0.5]
L3B = [0.9, 0.5, 0.9]  # unsorted, a duplicate
L64 = [((37 * k) % 64) / 63.0 for k in range(62)] + [0.5, 0.5]  # unsorted, 0 and 1 inside, a duplicate
PROBE = [0.5, 0.9, 0.99]


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
    """-> (records, full decode, its keys, first sample of the Constant records), built as the rolling suite's"""
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
    return recs, full, M.stream_keys(full), at


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
    return recs, full, M.stream_keys(full)


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
    return recs, full, M.stream_keys(full)


@pytest.fixture(scope="module")
def ties(A, ctx):
    """values rounded to multiples of 8 under RLE: long runs and few distinct values in a window"""
    x = np.round(H.synth_series(3180, 30000, block=2500) / 8.0) * 8.0
    recs = ctx.compress_host(x, H.frame_offsets(len(x), 1024), A.RLE, False, 0.0, 0)[0]
    full = ctx.decompress_host(recs)
    assert len(full) == len(x) and len(np.unique(full[:4096])) < 1024
    return recs, full, M.stream_keys(full)


def _assert_same(got, want, label):
    """each double bit for bit, any NaN where the model's value is NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~ok.all(axis=1))
    assert len(bad) == 0, (label, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


def _extra(w):
    """positions beside the window in a range: a case stays below 2^25 positions x width"""
    return max(3, min(700, (1 << 21) // w))


def _ranges(total, w, at):
    """the rolling suite's shapes: ranges that begin at odd and at aligned indices, overlap, come unsorted, are shorter
    than w, equal w, empty and lie over the Constant records (the 3000 NaN among them)"""
    e = _extra(w)
    c0 = max(at - w - 5, 0)
    r = [(4096, min(w + e, total - 4096)), (1, min(w + e // 2, total - 1)), (2047, w), (2048, w - 1), (777, 0),
         (total - w, w), (c0, min(w + 3200, total - c0)), (6001, min(w + e, total - 6001)), (total, 0)]
    return [x for x in r if x[0] + x[1] <= total]


def _strides(w):
    return [1, 2, 7, 64, w + 1, 8193]


@pytest.mark.parametrize("w", WIDTHS)
def test_every_row_matches_the_model(A, ctx, main, w):
    recs, full, keys, at = main
    total = len(full)
    for k, s in enumerate(_strides(w)):
        levels = (L3, L1, L3B, L64, L3, L64)[k]
        method = M.METHODS[(WIDTHS.index(w) + k) % 4]
        rg = _ranges(total, w, at)
        if M.outputs(total, w, s) * w <= 1 << 24:
            rg.append((0, total))  # whole: at every stride from the width on, and at the strides below it that keep the case small
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_quantile_windows_host(recs, b, c, w, levels, s, method)
        want, woff = M.rolling(full, b, c, w, s, levels, method, keys)
        assert off.tolist() == woff.tolist() and got.shape == (int(off[-1]), len(levels))
        assert off[3] == off[4] == off[5] and off[3] - off[2] == 1  # shorter than w: none; equal w: one
        assert int(off[-1]) * w <= 1 << 25
        _assert_same(got, want, (w, s, method))
        if s == 1 and w < 3000:  # the 3000 NaN give empty windows
            assert np.isnan(got).all(axis=1).any()


@pytest.mark.parametrize("method", M.METHODS)
def test_levels_and_methods(A, ctx, main, ties, counter, method):
    """n_q = 1, 3 and 64 under every method, on the main stream, on ties and over NaN holes"""
    for name, (recs, full, keys, *_) in (("main", main), ("ties", ties), ("counter", counter)):
        n = len(full)
        for w, s in ((65, 3), (300, 7), (1000, 3)):
            b, c = [1, 8990, min(20990, n - w - 200)], [min(2 * w + 500, n - 1), 2 * w + 40, w + 200]
            for levels in (L1, L3, L3B, L64):
                got, off = ctx.rolling_quantile_windows_host(recs, b, c, w, levels, s, method)
                _assert_same(got, M.rolling(full, b, c, w, s, levels, method, keys)[0], (name, w, s, method, len(levels)))


def test_ties_and_nan_holes(A, ctx, ties, counter):
    recs, full, keys = ties
    lv = [0.5, 0.55, 0.9]
    for w, s in ((2, 1), (64, 1), (257, 1), (2049, 5), (8192, 1)):
        b, c = [0, 4096, 12345], [w + _extra(w), w + _extra(w) // 2, w + 77]
        got, _ = ctx.rolling_quantile_windows_host(recs, b, c, w, lv, s, M.LOWER)
        _assert_same(got, M.rolling(full, b, c, w, s, lv, M.LOWER, keys)[0], ("ties", w, s))
        assert w != 257 or (got[:, 0] == got[:, 1]).any()  # (the stretch at 12345: one run of equal values spans two levels)
    recs, full, keys = counter
    n = len(full)
    for w, s in ((2, 1), (3, 1), (64, 1), (65, 3), (300, 7), (2049, 5), (4097, 3)):
        b, c = [8000, 8990, 20990], [min(2 * w + 1200, n - 8000), min(2 * w + 40, n - 8990), min(w + 200, n - 20990)]
        got, _ = ctx.rolling_quantile_windows_host(recs, b, c, w, PROBE, s)
        _assert_same(got, M.rolling(full, b, c, w, s, PROBE, M.LINEAR, keys)[0], ("counter", w, s))
        if w <= 64:
            assert np.isnan(got).all(axis=1).any()  # a window inside the hole of 70


def test_tasks_of_fewer_exactly_and_more_than_b_positions(A, ctx, long):
    """ranges of B - 1, B and B + 1 positions (and of 2 B and 2 B + 1), B = (P - w) / s + 1, for P = 512, 1024 and 8192"""
    recs, full, keys = long
    for w, s in ((20, 1), (300, 1), (300, 7), (3600, 4), (3600, 64), (7000, 1)):
        bb = M.task_positions(w, s)
        assert bb == {(20, 1): 493, (300, 1): 725, (300, 7): 104, (3600, 4): 1149, (3600, 64): 72, (7000, 1): 1193}[(w, s)]
        ms = [bb - 1, bb, bb + 1] + ([2 * bb, 2 * bb + 1] if bb * w < 1 << 21 else [])
        b = [1 + 20011 * i for i in range(len(ms))]
        c = [(m - 1) * s + w + (s - 1) * (i % 2) for i, m in enumerate(ms)]  # (a tail shorter than the stride adds none)
        got, off = ctx.rolling_quantile_windows_host(recs, b, c, w, PROBE, s)
        assert np.diff(off).tolist() == ms
        _assert_same(got, M.rolling(full, b, c, w, s, PROBE, M.LINEAR, keys)[0], (w, s))


def _listed_dev(A, ctx, torch, recs, lo, w, levels, method):
    """atsc_quantile_windows_dev over the listed windows (lo[i], w)"""
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        d = torch.zeros(len(lo) * len(levels), dtype=torch.float64, device="cuda")
        dp.quantile_windows(body, lo, np.full(len(lo), w), levels, d, method, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d.cpu().numpy().reshape(len(lo), len(levels))
    finally:
        dp.close()


def test_against_the_windowed_quantiles_on_the_listed_windows(A, ctx, torch, main, ties):
    """equal bits (any NaN for NaN) with atsc_quantile_windows_dev on the explicitly listed windows of the same positions:
    its short tier (w <= 256), its medium tier and, at 8192, the same sort"""
    recs, full, keys, at = main
    total = len(full)
    for k, (w, s) in enumerate(((1, 1), (3, 1), (65, 3), (256, 1), (300, 7), (2049, 5), (8192, 11))):
        method = M.METHODS[k % 4]
        c0 = max(at - w - 40, 0)
        rg = [(c0, min(w + 3300, total - c0)), (1, min(w + 2000, total - 1))]
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_quantile_windows_host(recs, b, c, w, L3B + [0.0, 1.0], s, method)
        lo = M.positions(b, c, w, s)
        _assert_same(got, _listed_dev(A, ctx, torch, recs, lo, w, L3B + [0.0, 1.0], method), (w, s))
    recs, full, keys = ties
    got, off = ctx.rolling_quantile_windows_host(recs, [5], [6000], 1000, PROBE, 3)
    _assert_same(got, _listed_dev(A, ctx, torch, recs, M.positions([5], [6000], 1000, 3), 1000, PROBE, M.LINEAR), "ties")


def test_pieces_do_not_change_the_bytes(A, ctx, long, main):
    """under the least budget a piece holds 65536 samples and consecutive pieces overlap by w - 1: the 200000 samples
    take four pieces, and the rows are the one-piece call's"""
    recs, full, keys = long
    b, c = [0, 90001], [LONG, 30000]
    try:
        for w, s in ((300, 1), (8192, 3)):
            ref, off = ctx.rolling_quantile_windows_host(recs, b, c, w, PROBE, s)
            assert len(ref) == M.outputs(LONG, w, s) + M.outputs(30000, w, s)
            # the model on the rows whose windows lie round the pieces' ends, and on a few others
            ends = [65536, 2 * 65536 - (w - 1), 3 * 65536 - 2 * (w - 1)]
            pick = sorted({j for e in ends for j in range(max((e - w) // s - 3, 0), (e - w) // s + 4)} |
                          set(range(0, int(off[1]), max(1, int(off[1]) // 40))))
            _assert_same(ref[pick], M.rows(full, np.array(pick) * s, w, PROBE, M.LINEAR, keys), ("default", w))
            ctx.set_aggregate_scratch(1)
            got, _ = ctx.rolling_quantile_windows_host(recs, b, c, w, PROBE, s)
            ctx.set_aggregate_scratch(0)
            assert got.tobytes() == ref.tobytes(), (w, s)
        # the main stream under the least budget: a large frame across the pieces' ends
        mrecs, mfull, mkeys, _ = main
        assert len(mfull) > 65536
        ctx.set_aggregate_scratch(1)
        got, _ = ctx.rolling_quantile_windows_host(mrecs, [0], [len(mfull)], 300, PROBE, 5)
    finally:
        ctx.set_aggregate_scratch(0)
    _assert_same(got, M.rolling(mfull, [0], [len(mfull)], 300, 5, PROBE, M.LINEAR, mkeys)[0], "main, least budget")


def test_one_plan_serves_a_rolling_a_quantile_and_a_rolling_quantile_call(A, ctx, torch, long):
    """the rolling quantiles keep their tables and scratch in the rolling's place of the plan, the windowed quantiles in
    their own: enqueued one after the other without a synchronisation in between, each gives its own bytes, twice"""
    recs, full, keys = long
    b, c, w, s = [5, 100000], [12000, 9000], 3000, 3
    lo = M.positions(b, c, w, s)[::50]
    want_r, off = RM.Pyramid(full).rolling(b, c, w, s)
    n = len(want_r)
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        r1, r2 = (torch.full((4 * n,), SENT, dtype=torch.int64, device="cuda") for _ in range(2))
        q1, q2 = (torch.zeros(3 * n, dtype=torch.float64, device="cuda") for _ in range(2))
        l1, l2 = (torch.zeros(3 * len(lo), dtype=torch.float64, device="cuda") for _ in range(2))
        st = torch.cuda.current_stream().cuda_stream
        dp.rolling_quantile_windows(body, b, c, w, s, PROBE, q1, M.LINEAR, st)
        dp.rolling_windows(body, b, c, w, s, r1, st)
        dp.quantile_windows(body, lo, np.full(len(lo), w), PROBE, l1, M.LINEAR, st)
        dp.rolling_quantile_windows(body, b, c, w, s, PROBE, q2, M.LINEAR, st)
        dp.quantile_windows(body, lo, np.full(len(lo), w), PROBE, l2, M.LINEAR, st)
        dp.rolling_windows(body, b, c, w, s, r2, st)
        torch.cuda.synchronize()
        assert r1.cpu().numpy().tobytes() == r2.cpu().numpy().tobytes() == ctx.rolling_windows_host(recs, b, c, w, s)[0].tobytes()
        a = r1.cpu().numpy().view(A.WINDOW_ROLLING)
        assert a["count"].tolist() == want_r["count"].tolist() and a["sum"].tobytes() == want_r["sum"].tobytes()
        first = q1.cpu().numpy().reshape(n, 3)
        assert first.tobytes() == q2.cpu().numpy().tobytes()
        _assert_same(first, M.rolling(full, b, c, w, s, PROBE, M.LINEAR, keys)[0], "rolling quantile")
        assert l1.cpu().numpy().tobytes() == l2.cpu().numpy().tobytes() == first[::50].tobytes()
    finally:
        dp.close()


def test_host_device_and_stream_calls_agree(A, ctx, torch):
    x = H.synth_series(3170, 50000, block=7000)
    x[12345:12400] = np.nan
    bro = A.compress_data(ctx, x, A.AUTO, 3)
    full = A.decompress_data(ctx, bro)
    keys = M.stream_keys(full)
    n0, p0 = H.varint_decode(bro, 9)
    body = torch.from_numpy(np.frombuffer(bro[p0:], dtype=np.uint8).copy()).to("cuda")
    dp = A.DPlan(ctx, bro[p0:])
    st = A.CompressedStream.from_bytes(ctx, bro)
    try:
        for (w, s), method in zip(((300, 1), (65, 7), (4097, 3)), (M.LINEAR, M.NEAREST, M.HIGHER)):
            b, c = [30001, 20000, 47000], [6000, 5001, 100]  # begins far into the stream: the host call uploads a part
            want, woff = M.rolling(full, b, c, w, s, PROBE, method, keys)
            via_bro, off = A.rolling_quantile_data_windows(ctx, bro, b, c, w, PROBE, s, method)
            _assert_same(via_bro, want, (w, s))
            assert off.tolist() == woff.tolist() and via_bro.shape == want.shape
            host, _ = ctx.rolling_quantile_windows_host(bro[9:], b, c, w, PROBE, s, method, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), (w, s)
            assert st.rolling_quantile_windows(b, c, w, PROBE, s, method)[0].tobytes() == via_bro.tobytes(), (w, s)
            d = torch.full((3 * len(want) + 1,), -7.0, dtype=torch.float64, device="cuda")
            rows, doff = dp.rolling_quantile_windows(body, b, c, w, s, PROBE, d, method, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rows.shape == want.shape and doff.tolist() == woff.tolist() and float(d[-1]) == -7.0
            assert rows.cpu().numpy().tobytes() == via_bro.tobytes(), (w, s)
    finally:
        dp.close()


def _raw_host(A, ctx, buf, rg, w, s, levels, method, n_out=64, null_q=False):
    out = np.full(n_out, SENT, dtype=np.uint64)
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    q = np.array(levels if len(levels) else [0.5], dtype=np.float64)
    p, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    rc = A.capi.lib().atsc_rolling_quantile_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(rg),
                                                    b.ctypes.data_as(p), c.ctypes.data_as(p), w, s, len(levels),
                                                    None if null_q else q.ctypes.data_as(pd), method,
                                                    C.c_void_p(out.ctypes.data))
    return rc, out


ERRORS = [([(0, 100)], 0, 1, [0.5], 0, "width outside"),
          ([(0, 100)], 10, 0, [0.5], 0, "stride is 0"),
          ([(LONG - 50, 100)], 10, 1, [0.5], 0, ""),
          ([(0, 20), (LONG + 1, 0)], 10, 1, [0.5], 0, ""),
          ([(2 ** 63, 2 ** 63)], 10, 1, [0.5], 0, ""),
          ([(0, 2 ** 33)], 1, 1, [0.5], 0, ""),
          ([(0, 20000)], 8193, 1, [0.5], 0, "width above 8192"),
          ([(0, 20000)], 1 << 20, 1, [0.5], 0, "width above 8192"),
          ([(0, 100)], 10, 1, [], 0, "n_q outside"),
          ([(0, 100)], 10, 1, [0.5] * 65, 0, "n_q outside"),
          ([(0, 100)], 10, 1, [0.5, float("nan")], 0, "a level is NaN or outside"),
          ([(0, 100)], 10, 1, [-0.001], 0, "a level is NaN or outside"),
          ([(0, 100)], 10, 1, [0.5, 1.5], 0, "a level is NaN or outside"),
          ([(0, 100)], 10, 1, [0.5], 4, "unknown method"),
          ([(0, 100)], 10, 1, [0.5], -1, "unknown method")]


def test_errors_leave_the_result_untouched(A, ctx, torch, long):
    recs, full, keys = long
    buf = np.frombuffer(recs, dtype=np.uint8)
    E = A.capi
    for rg, w, s, levels, method, what in ERRORS:
        rc, out = _raw_host(A, ctx, buf, rg, w, s, levels, method)
        msg = E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert rc == E.E_INVALID and np.all(out == SENT), (rg, w, s, levels, method, rc)
        assert not what or msg.startswith("rolling_quantile_windows: " + what), msg  # the call's own checks name the call
        if w > 8192:
            assert "8192" in msg and "atsc_quantile_windows with listed windows" in msg, msg
    rc, out = _raw_host(A, ctx, buf, [(0, 100)], 10, 1, [0.5], 0, null_q=True)
    assert rc == E.E_INVALID and np.all(out == SENT)
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(buf.copy()).to("cuda")
    p, pd = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    try:
        def dev(rg, w, s, levels, method, d_ptr, null_q=False):
            b = np.array([x[0] for x in rg], dtype=np.uint64)
            c = np.array([x[1] for x in rg], dtype=np.uint64)
            q = np.array(levels if len(levels) else [0.5], dtype=np.float64)
            rc = E.lib().atsc_rolling_quantile_windows_dev(ctx._h, dp._h, C.c_void_p(body.data_ptr()), len(rg), b.ctypes.data_as(p),
                                                           c.ctypes.data_as(p), w, s, len(levels),
                                                           None if null_q else q.ctypes.data_as(pd), method, C.c_void_p(d_ptr),
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            return rc

        d = torch.full((256,), SENT, dtype=torch.int64, device="cuda")
        for rg, w, s, levels, method, what in ERRORS:
            assert dev(rg, w, s, levels, method, d.data_ptr()) == E.E_INVALID and bool((d == SENT).all()), (rg, w, s, levels, method)
        assert dev([(0, 100)], 10, 1, [0.5], 0, d.data_ptr(), null_q=True) == E.E_INVALID and bool((d == SENT).all())
        assert dev([(0, 100)], 10, 1, [0.5], 0, d.data_ptr() + 4) == E.E_INVALID and bool((d == SENT).all())
        assert "d_out is not 8-byte aligned" in E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert dev([(0, 100)], 10, 1, [0.5], 0, d.data_ptr()) == 0 and bool((d[91:] == SENT).all()) and not bool((d[:91] == SENT).any())
    finally:
        dp.close()
    st = A.CompressedStream.from_bytes(ctx, A.compress_data(ctx, np.arange(1000.0), A.NOOP, 0))
    with pytest.raises(A.AtscError) as e:
        st.rolling_quantile_windows([0], [100], 8193, [0.5])
    assert e.value.rc == E.E_INVALID
    with pytest.raises(A.AtscError) as e:
        st.rolling_quantile_windows([0], [100], 10, [1.5])
    assert e.value.rc == E.E_INVALID
    assert st.rolling_quantile_windows([0], [100], 10, [0.5])[0][:, 0].tolist() == [4.5 + j for j in range(91)]
    rc, out = _raw_host(A, ctx, buf, [], 5, 1, [0.5], 0)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, buf, [(5, 0), (LONG, 0), (7, 4)], 5, 1, [0.5], 0)  # no range holds a window: no row
    assert rc == 0 and np.all(out == SENT)
    # the least budget holds the widest window: there is no capacity case
    try:
        ctx.set_aggregate_scratch(1)
        rc, out = _raw_host(A, ctx, buf, [(0, 8192 + 15)], 8192, 1, [0.5, 1.0], 0)
    finally:
        ctx.set_aggregate_scratch(0)
    assert rc == 0 and np.all(out[32:] == SENT)
    _assert_same(out[:32].view(np.float64).reshape(16, 2), M.rolling(full, [0], [8192 + 15], 8192, 1, [0.5, 1.0], M.LINEAR, keys)[0],
                 "widest, least budget")


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
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 20, 20), (5 * n + 3, 100), (3 * n + 5, 0)]
    b, c = [w[0] for w in outside], [w[1] for w in outside]
    got, _ = ctx.rolling_quantile_windows_host(bad, b, c, 20, PROBE, 3)
    _assert_same(got, M.rolling(good, b, c, 20, 3, PROBE)[0], "outside")
    bb = np.frombuffer(bad, dtype=np.uint8)
    for rg in ([(3 * n, 20)], [(0, nf * n)], [(0, 40), (3 * n - 19, 20)], [(4 * n - 20, 20), (6 * n, 50)]):
        rc, out = _raw_host(A, ctx, bb, rg, 20, 1, PROBE, 0, n_out=3 * nf * n)
        assert rc == A.capi.E_FORMAT and np.all(out == SENT), (rg, rc)
    # The device call sets the plan's status word, which has no accessor (see tests/test_gpu_histogram.py): the host call
    # above -- the device call on a plan of the touched records, then a read of the plan's word -- is what shows it.  The
    # device call itself returns ATSC_OK, finishes, writes every row, and gives the ranges beside the bad frame theirs.
    dp = A.DPlan(ctx, bad)
    body = torch.from_numpy(bb.copy()).to("cuda")
    try:
        rg = [(0, 3 * n), (3 * n + 7, 40), (4 * n, 100)]
        b, c = [w[0] for w in rg], [w[1] for w in rg]
        want, off = M.rolling(good, b, c, 20, 1, PROBE)
        d = torch.full((3 * len(want),), SENT, dtype=torch.int64, device="cuda")
        dp.rolling_quantile_windows(body, b, c, 20, 1, PROBE, d.view(torch.float64), M.LINEAR, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        h = d.cpu().numpy().view(np.uint64)
        assert not (h == SENT).any()
        clean = np.r_[0: int(off[1]), int(off[2]): int(off[3])]
        _assert_same(h.view(np.float64).reshape(-1, 3)[clean], want[clean], "dev, beside the bad frame")
    finally:
        dp.close()


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def _check_rows(plain, with_q, first, names, want, in_front=""):
    """the .roll.csv of one call without and with --rolling-quantiles: the other columns are the plain file's, byte for
    byte; the levels' columns come last, named q<level as typed>, and parse back to the model's bits"""
    base, ql = plain.split("\n"), with_q.split("\n")
    assert base[0] == first + ",count,min,max,sum,mean" + in_front and ql[0] == base[0] + "".join(",q" + t for t in names)
    assert len(base) == len(ql) == len(want) + 2 and base[-1] == ql[-1] == ""
    k = len(names)
    for j in range(len(want)):
        cells = ql[1 + j].split(",")
        assert ",".join(cells[:-k]) == base[1 + j]
        got = np.array([float(t) for t in cells[-k:]])
        _assert_same(got[None, :], want[j][None, :], (j, cells[-k:]))


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
    hi = len(times) - 3
    common = (csvc, "-u", "--from", times[10], "--to", times[hi], "-o", tmp_path / "win")
    at = np.flatnonzero((times >= times[10]) & (times <= times[hi]))
    for spec, (w, s), names, extra, method in (("20:3", (20, 3), ["0.5", "0.99"], (), M.LINEAR),
                                               ("20", (20, 1), ["1", "0.50", "0"], ("--rolling-quantile-method", "lower"), M.LOWER)):
        _run(*common, "--rolling", spec, tmp_path / "cpu.bro")
        plain = (tmp_path / "win.roll.csv").read_text()
        _run(*common, "--rolling", spec, "--rolling-quantiles", ",".join(names), *extra, tmp_path / "cpu.bro")
        want, _ = M.rolling(full, [int(at[0])], [len(at)], w, s, [float(t) for t in names], method)
        assert len(want) == M.outputs(len(at), w, s) > 0
        _check_rows(plain, (tmp_path / "win.roll.csv").read_text(), "timestamp", names, want)
    for bad, what in ((("--rolling-quantiles", "0.5"), "'--rolling-quantiles' needs '--rolling'"),
                      (("--rolling", "20", "--rolling-quantile-method", "lower"), "'--rolling-quantile-method' needs '--rolling-quantiles'"),
                      (("--rolling", "8193", "--rolling-quantiles", "0.5"), "'--rolling-quantiles' needs a '--rolling' W in 1..=8192"),
                      (("--rolling", "20", "--rolling-quantiles", "0.5,1.5"), "invalid value '0.5,1.5' for '--rolling-quantiles'")):
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
    out = tmp_path / "uptime.roll.csv"
    for spec, (b0, c0), (w, s), names, extra, method in (
            ("20", (0, len(full)), (20, 1), ["0.5", "0.9", "0.99"], (), M.LINEAR),
            ("300:15", (100, 1500), (300, 15), ["0.25", "1.0"], ("--rolling-quantile-method", "nearest"), M.NEAREST)):
        common = (atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--rolling", spec)
        want, _ = M.rolling(full, [b0], [c0], w, s, [float(t) for t in names], method)
        assert len(want) == M.outputs(c0, w, s) > 0
        _run(*common, tmp_path / "uptime.bro")
        plain = out.read_text()
        _run(*common, "--rolling-quantiles", ",".join(names), *extra, tmp_path / "uptime.bro")
        _check_rows(plain, out.read_text(), "offset", names, want)
        _run(*common, "--rolling-moments", tmp_path / "uptime.bro")  # behind the moments' columns where both are given
        plain_m = out.read_text()
        _run(*common, "--rolling-moments", "--rolling-quantiles", ",".join(names), *extra, tmp_path / "uptime.bro")
        _check_rows(plain_m, out.read_text(), "offset", names, want, ",nonnan,avg,stdvar,stddev,slope,intercept")
    for bad, what in ((("-u", "--rolling-quantiles", "0.5"), "'--rolling-quantiles' needs '--rolling'"),
                      (("-u", "--samples", "0:10", "--buckets", "5", "--rolling-quantiles", "0.5"), "'--rolling-quantiles' needs '--rolling'"),
                      (("-u", "--samples", "0:100", "--rolling", "20", "--rolling-quantile-method", "lower"),
                       "'--rolling-quantile-method' needs '--rolling-quantiles'"),
                      (("-u", "--samples", "0:100", "--rolling", "8193", "--rolling-quantiles", "0.5"),
                       "'--rolling-quantiles' needs a '--rolling' W in 1..=8192"),
                      (("-u", "--samples", "0:100", "--rolling", "20", "--rolling-quantile-method", "median", "--rolling-quantiles", "0.5"),
                       "invalid value 'median' for '--rolling-quantile-method'")):
        r = subprocess.run([atsc, *bad, str(tmp_path / "uptime.bro")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and what in r.stderr, (bad, r.returncode, r.stderr)
