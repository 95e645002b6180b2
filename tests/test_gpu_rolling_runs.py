"""Windowed rolling runs on the GPU: every record of every case against the NumPy model of the contract
(tests/rolling_runs_model.py) applied to the GPU's own full decode, bit for bit in all ten fields (under a +-Inf limit
excess may be NaN, and then any NaN conforms).  The main stream is the rolling suite's (every frame-length tier below the
large one under every codec, one large frame, Constant records of NaN, +-Inf and zeros of both signs); a run-structured
integer stream in Noop frames serves the widths across the 2^16 and the 2^18 level, the budgets that cut a range into
pieces and the comparison of all ten fields with atsc_runs_windows_dev.  The host, device and stream calls; a rolling and
a rolling runs call on one plan; errors that leave the result untouched; a malformed payload; both command lines."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import rolling_model as RM
from tests import rolling_runs_model as M
from tests import runs_model as R
from tests.test_gpu_rolling import CONSTANTS, LENS, _const_record, _fft_record, _rec

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 5, 8, 9, 64, 65, 300, 2048, 2049, 4097]  # a level closes at w = 2^l
SENT = 0x5A5A5A5A5A5A5A5A
INTS = M.FIELDS[:9]
LIMIT = 5.0  # of the run-structured streams: inside samples are 10 .. 16, the others 0 .. 5


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


class Models:
    """the model pyramids of one stream, one per condition, built when first asked for"""

    def __init__(self, full):
        self.full, self.made = full, {}

    def __call__(self, op, limit):
        key = (op, np.float64(limit).tobytes())
        if key not in self.made:
            self.made[key] = M.Pyramid(self.full, op, limit)
        return self.made[key]


@pytest.fixture(scope="module")
def main(A, ctx):
    """-> (records, full decode, models, first sample of the Constant records, a limit near the median), built as the
    rolling suite's"""
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
    assert 40000 <= len(full) <= 200000
    limit = float(np.nanmedian(full[np.isfinite(full)]))
    inside = R.inside_mask(full, R.GT, limit).mean()
    assert 0.2 < inside < 0.8
    return recs, full, Models(full), at, limit


def _run_stream(rng, n, forced=()):
    """n integers: runs of 1 .. 5000 samples over LIMIT (10 .. 16) between gaps of 1 .. 300 samples at or under it
    (0 .. 5); forced: stretches that are inside whatever was drawn"""
    x = np.empty(n)
    at, inside = 0, False
    while at < n:
        ln = int(rng.integers(1, 5001)) if inside else int(rng.integers(1, 301))
        seg = x[at:at + ln]
        seg[:] = rng.integers(10, 17, len(seg)) if inside else rng.integers(0, 6, len(seg))
        at, inside = at + ln, not inside
    for a, b in forced:
        x[a:b] = 10.0 + (np.arange(a, b) % 7)
    return x


def _noop_records(A, ctx, x):
    """Noop frames of 4096: cheap to build and to decode; Noop stores 64-bit integers, so x holds integers"""
    return ctx.compress_host(x, H.frame_offsets(len(x), 4096), A.NOOP, False, 0.0, 0)[0]


def _noop(A, ctx, x):
    recs = _noop_records(A, ctx, x)
    full = ctx.decompress_host(recs)
    assert np.array_equal(full, x)
    return recs, full, Models(full)


@pytest.fixture(scope="module")
def long(A, ctx):
    """200000 integers in runs, stored as Noop, with NaN holes (Constant records of NaN between the Noop frames), one of
    them inside a run; runs across index 65536 and across multiples of 2048"""
    x = _run_stream(np.random.default_rng(23), 200000, forced=((65000, 66500), (69990, 70010), (149000, 151000)))
    recs, want = b"", []
    for seg, hole in ((x[:70000], 1), (x[70000:70001], 2), (x[70001:150000], 3), (x[150000:], 0)):
        recs += _noop_records(A, ctx, seg) + (_const_record(A, ctx, np.nan, hole) if hole else b"")
        want += [seg, np.full(hole, np.nan)]
    full = ctx.decompress_host(recs)
    assert np.array_equal(full, np.concatenate(want), equal_nan=True) and len(full) == 200006
    m = R.inside_mask(full, R.GT, LIMIT)
    assert m[65535] and m[65536] and m[69999] and not m[70000] and m[70001]
    d = np.diff(np.concatenate(([0], m.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    assert np.any(starts // 2048 != (ends - 1) // 2048) and (ends - starts).max() > 4000 and (ends - starts).min() == 1
    return recs, full, Models(full)


def _assert_same(got, want, label, nan_excess=False):
    """bit for bit, field by field; nan_excess: excess may be NaN, and is then NaN in both"""
    assert len(got) == len(want), (label, len(got), len(want))
    a = np.ascontiguousarray(got).view(np.uint64).reshape(-1, 10).copy()
    b = np.ascontiguousarray(want).view(np.uint64).reshape(-1, 10).copy()
    if nan_excess:
        both = np.isnan(a[:, 9].view(np.float64)) & np.isnan(b[:, 9].view(np.float64))
        a[both, 9] = b[both, 9] = 0
    bad = np.flatnonzero((a != b).any(axis=1))
    assert len(bad) == 0, (label, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


def _ranges(total, w, at):
    """the rolling suite's shapes: ranges that begin at odd and at aligned indices, overlap, come unsorted, are shorter
    than w, equal w, empty, lie over the Constant records, and (last) span the whole stream"""
    r = [(4096, min(3 * w + 700, total - 4096)), (1, min(2 * w + 33, total - 1)), (2047, w), (2048, w - 1), (777, 0),
         (total - w, w), (max(at - w - 5, 0), min(2 * w + 3200, total - max(at - w - 5, 0))),
         (6001, min(w + 900, total - 6001)), (total, 0), (0, total)]
    return [x for x in r if x[0] + x[1] <= total]


@pytest.mark.parametrize("w", WIDTHS)
def test_every_record_matches_the_model(A, ctx, main, w):
    recs, full, models, at, limit = main
    P = models(A.RUNS_GT, limit)
    for s in (1, 7, w, 2 * w + 1):
        rg = _ranges(len(full), w, at)
        if s > 7:
            rg = rg[:-1] + [(3, len(full) - 3)]
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_runs_windows_host(recs, b, c, w, A.RUNS_GT, limit, s)
        want, woff = P.rolling(b, c, w, s)
        assert off.tolist() == woff.tolist() and got.dtype == A.WINDOW_RUNS
        assert off[3] == off[4] == off[5] and off[3] - off[2] == 1  # shorter than w: none; equal w: one
        _assert_same(got, want, (w, s))
        assert np.all(got["samples"] == w) and len(got) > 0
        if s == 1 and w <= 9:  # the records hold what the cases are about
            assert (got["inside"] == 0).any() and (got["inside"] == w).any()
            assert np.all(got["first_at"][got["inside"] == 0] == A.RUNS_NONE)


@pytest.mark.parametrize("w", [1, 9, 300, 2049])
def test_all_six_ops_and_three_limits(A, ctx, main, w):
    """a limit that the Constant records hold (EQ and NE, GE and GT differ there), +0.0 against samples of -0.0, and
    +Inf (x - limit is -Inf, or NaN for a sample of +Inf)"""
    recs, full, models, at, _ = main
    total = len(full)
    rg = [(max(at - w - 40, 0), min(2 * w + 5300, total - max(at - w - 40, 0))), (1, min(w + 2000, total - 1))]
    b, c = [x[0] for x in rg], [x[1] for x in rg]
    for limit in (2.5, 0.0, np.inf):
        seen = set()
        for op in R.OPS:
            got, off = ctx.rolling_runs_windows_host(recs, b, c, w, op, limit, 1)
            want, woff = models(op, limit).rolling(b, c, w, 1)
            assert off.tolist() == woff.tolist()
            _assert_same(got, want, (w, op, limit), nan_excess=bool(np.isinf(limit)))
            for k in INTS:
                assert got[k].tobytes() == want[k].tobytes(), (w, op, limit, k)
            seen.add(got["inside"].tobytes())
        # no two operators select the same samples here; under +Inf GE is EQ and LT is NE
        assert len(seen) == (4 if np.isinf(limit) else 6), (w, limit)


def _dev(A, torch, dp, body, b, c, w, s, op, limit, n):
    d = torch.full((10 * n + 10,), SENT, dtype=torch.int64, device="cuda")
    off = dp.rolling_runs_windows(body, b, c, w, s, op, limit, d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = d.cpu().numpy()
    assert np.all(h[10 * n:] == SENT)  # the sentinel behind the result
    return h[: 10 * n].view(A.WINDOW_RUNS), off


def test_width_across_the_65536_level(A, ctx, torch, long):
    recs, full, models = long
    n = len(full)
    w = 70001
    P = models(A.RUNS_GT, LIMIT)
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        for s, rg in ((1, [(58000, w + 12000)]), (7, [(65535, n - 65535), (1, 140003)]), (w, [(3, n - 3)]),
                      (2 * w + 1, [(0, n), (60000, w)])):
            b, c = [x[0] for x in rg], [x[1] for x in rg]
            want, woff = P.rolling(b, c, w, s)
            got, off = _dev(A, torch, dp, body, b, c, w, s, A.RUNS_GT, LIMIT, len(want))
            assert off.tolist() == woff.tolist()
            _assert_same(got, want, (w, s))
        assert int(want["longest"].max()) > 4000
    finally:
        dp.close()


def test_width_across_the_262144_level(A, ctx):
    """w = 2^18 + 1: the chunks of level 18 come from the second launch of the upper kernel.  In the stream of
    2^18 + 5000 samples the window at 0 reads the aligned chunk of that level at 0; in the longer stream the windows at
    2^18 - 1 and 2^18 read the one at 2^18"""
    w = (1 << 18) + 1
    n = (1 << 18) + 5000
    rng = np.random.default_rng(31)
    recs, full, models = _noop(A, ctx, _run_stream(rng, n, forced=((262000, 263000),)))
    assert max(l for _, l in M.chunks(0, w)) == 18
    got, off = ctx.rolling_runs_windows_host(recs, [0], [n], w, A.RUNS_GT, LIMIT, 1)
    want, woff = models(A.RUNS_GT, LIMIT).rolling([0], [n], w, 1)
    assert off.tolist() == woff.tolist() == [0, n - w + 1]
    _assert_same(got, want, w)
    recs, full, models = _noop(A, ctx, _run_stream(rng, (1 << 19) + 16, forced=((262000, 263000), (524000, 524300))))
    lo = (1 << 18) - 4
    assert [max(l for _, l in M.chunks(lo + j, w)) for j in range(7)] == [17, 17, 17, 18, 18, 17, 17]
    got, off = ctx.rolling_runs_windows_host(recs, [lo], [w + 6], w, A.RUNS_LE, LIMIT, 1)
    _assert_same(got, models(A.RUNS_LE, LIMIT).rolling([lo], [w + 6], w, 1)[0], (w, "level 18 read"))


def _listed_dev(A, ctx, torch, recs, lo, w, op, limit):
    """atsc_runs_windows_dev over the listed windows (lo[i], w)"""
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        d = torch.zeros(10 * len(lo), dtype=torch.int64, device="cuda")
        dp.runs_windows(body, lo, np.full(len(lo), w), op, limit, d, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d.cpu().numpy().view(A.WINDOW_RUNS)
    finally:
        dp.close()


def test_against_the_windowed_runs_on_the_listed_windows(A, ctx, torch, main, long):
    recs, full, models, at, limit = main
    total = len(full)
    for (w, s), (op, lim) in zip(((1, 1), (2, 1), (3, 1), (65, 3), (300, 7), (2049, 5), (4097, 11)),
                                 ((A.RUNS_GT, limit), (A.RUNS_EQ, 0.0), (A.RUNS_NE, 2.5), (A.RUNS_LE, limit), (A.RUNS_GE, 1.0),
                                  (A.RUNS_GT, limit), (A.RUNS_LT, np.inf))):
        rg = [(max(at - w - 40, 0), min(2 * w + 5300, total - max(at - w - 40, 0))), (1, min(w + 2000, total - 1))]
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_runs_windows_host(recs, b, c, w, op, lim, s)
        lo = np.concatenate([rg[i][0] + s * np.arange(int(off[i + 1] - off[i])) for i in range(len(rg))])
        ref = _listed_dev(A, ctx, torch, recs, lo, w, op, lim)
        for k in INTS:
            assert got[k].tobytes() == ref[k].tobytes(), (w, s, k)
    # the integer stream: excess is exact, so the whole record is the windowed runs'
    lrecs, lfull, lmodels = long
    for (w, s), (op, lim) in zip(((2, 1), (9, 1), (300, 7), (4097, 3)),
                                 ((A.RUNS_GT, LIMIT), (A.RUNS_NE, 12.0), (A.RUNS_LE, LIMIT), (A.RUNS_GT, LIMIT))):
        got, off = ctx.rolling_runs_windows_host(lrecs, [60001, 0], [20000, 3 * w], w, op, lim, s)
        lo = np.concatenate([60001 + s * np.arange(int(off[1])), s * np.arange(int(off[2] - off[1]))])
        ref = _listed_dev(A, ctx, torch, lrecs, lo, w, op, lim)
        assert got.tobytes() == ref.tobytes(), (w, s)
        assert int(got["inside"].max()) > 0 and int(got["inside"].min()) < w  # samples of both kinds are inside the windows
        _assert_same(got, lmodels(op, lim).records(lo, w), ("integers", w, s))


def test_host_device_and_stream_calls_agree(A, ctx, torch):
    x = H.synth_series(3170, 50000, block=7000)
    x[12345:12400] = np.nan
    bro = A.compress_data(ctx, x, A.AUTO, 3)
    full = A.decompress_data(ctx, bro)
    limit = float(np.nanmedian(full))
    n0, p0 = H.varint_decode(bro, 9)
    body = torch.from_numpy(np.frombuffer(bro[p0:], dtype=np.uint8).copy()).to("cuda")
    dp = A.DPlan(ctx, bro[p0:])
    st = A.CompressedStream.from_bytes(ctx, bro)
    try:
        for (w, s), op in zip(((300, 1), (65, 7), (4097, 3)), (A.RUNS_GT, A.RUNS_LE, A.RUNS_NE)):
            b, c = [30001, 20000, 47000], [15000, 12001, 100]  # begins far into the stream: the host call uploads a part
            want, woff = M.Pyramid(full, op, limit).rolling(b, c, w, s)
            via_bro, off = A.rolling_runs_data_windows(ctx, bro, b, c, w, op, limit, s)
            _assert_same(via_bro, want, (w, s))
            assert off.tolist() == woff.tolist()
            host, _ = ctx.rolling_runs_windows_host(bro[9:], b, c, w, op, limit, s, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), (w, s)
            assert st.rolling_runs_windows(b, c, w, op, limit, s)[0].tobytes() == via_bro.tobytes(), (w, s)
            got, _ = _dev(A, torch, dp, body, b, c, w, s, op, limit, len(want))
            assert got.tobytes() == via_bro.tobytes(), (w, s)
    finally:
        dp.close()


def test_rolling_and_rolling_runs_share_the_plans_place(A, ctx, torch, long):
    """the two calls keep their tables and scratch in one place of the plan: enqueued one after the other without a
    synchronisation in between, each gives its own bytes"""
    recs, full, models = long
    RP = RM.Pyramid(full)
    b, c, w, s = [5, 100000], [90000, 30000], 3000, 3
    want_r, off = RP.rolling(b, c, w, s)
    n = len(want_r)
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    try:
        r1, r2 = (torch.full((4 * n,), SENT, dtype=torch.int64, device="cuda") for _ in range(2))
        d1, d2 = (torch.full((10 * n,), SENT, dtype=torch.int64, device="cuda") for _ in range(2))
        q = torch.cuda.current_stream().cuda_stream
        dp.rolling_windows(body, b, c, w, s, r1, q)
        dp.rolling_runs_windows(body, b, c, w + 1, s, A.RUNS_GT, LIMIT, d1, q)  # (another width: other level tables in the same place)
        dp.rolling_runs_windows(body, b, c, w + 1, s, A.RUNS_LE, LIMIT, d2, q)  # (another condition: another pyramid)
        dp.rolling_windows(body, b, c, w, s, r2, q)
        torch.cuda.synchronize()
        first, second = r1.cpu().numpy(), r2.cpu().numpy()
        assert first.tobytes() == second.tobytes() == ctx.rolling_windows_host(recs, b, c, w, s)[0].tobytes()
        a, e = first.view(A.WINDOW_ROLLING), want_r
        assert a["count"].tolist() == e["count"].tolist() and a["sum"].tobytes() == e["sum"].tobytes()
        for d, op in ((d1, A.RUNS_GT), (d2, A.RUNS_LE)):
            want, _ = models(op, LIMIT).rolling(b, c, w + 1, s)
            assert 0 < len(want) <= n
            _assert_same(d.cpu().numpy()[: 10 * len(want)].view(A.WINDOW_RUNS), want, ("between two rolling calls", op))
    finally:
        dp.close()


def _pieces(n, budget, w):
    """the pieces of a range of n samples from sample 0 of a stream without large frames under a budget, by DESIGN.md's
    piece arithmetic: a region of Lr = max(65536, 8 / 16 of budget / 8 rounded down to 2048) samples, a piece of
    Lr - 3 * 2048, consecutive pieces overlapping by w - 1"""
    lp = max(65536, budget // 8 * 8 // 16 // 2048 * 2048) - 3 * 2048
    k, p = 1, 0
    while p + lp < n:
        p, k = p + lp - (w - 1), k + 1
    return k


def test_pieces_do_not_change_the_bytes(A, ctx, long, main):
    recs, full, models = long
    n = len(full)
    P = models(A.RUNS_GT, LIMIT)
    b, c = [0, 90001], [n, 30000]
    two, three = 110592 * 16, 1
    try:
        for w in (3000, 50000):  # the second: close to the least budget's piece of 59392, which then advances by 9393
            ref, _ = ctx.rolling_runs_windows_host(recs, b, c, w, A.RUNS_GT, LIMIT, 1)
            _assert_same(ref, P.rolling(b, c, w, 1)[0], "default")
            assert _pieces(n, two, w) == (2 if w == 3000 else 3) and _pieces(n, three, w) >= (3 if w == 3000 else 15)
            for budget in (two, three):
                ctx.set_aggregate_scratch(budget)
                got, _ = ctx.rolling_runs_windows_host(recs, b, c, w, A.RUNS_GT, LIMIT, 1)
                assert got.tobytes() == ref.tobytes(), (w, budget)
                if w == 3000:
                    got7, _ = ctx.rolling_runs_windows_host(recs, b, c, w, A.RUNS_GT, LIMIT, 7)
                    assert got7.tobytes() == ref[: n - w + 1][::7].tobytes() + ref[n - w + 1:][::7].tobytes(), budget
            ctx.set_aggregate_scratch(0)
        # the main stream under the least budget: a large frame across the pieces' ends
        mrecs, mfull, mmodels, _, limit = main
        ctx.set_aggregate_scratch(1)
        got, _ = ctx.rolling_runs_windows_host(mrecs, [0], [len(mfull)], 3000, A.RUNS_GT, limit, 1)
    finally:
        ctx.set_aggregate_scratch(0)
    assert len(mfull) > 65536
    _assert_same(got, mmodels(A.RUNS_GT, limit).rolling([0], [len(mfull)], 3000, 1)[0], "main, least budget")


def _raw_host(A, ctx, buf, rg, w, s, op=0, limit=LIMIT, n_out=16):
    out = np.full(10 * n_out, SENT, dtype=np.uint64)
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    rc = A.capi.lib().atsc_rolling_runs_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(rg),
                                                b.ctypes.data_as(p), c.ctypes.data_as(p), w, s, op, limit,
                                                C.c_void_p(out.ctypes.data))
    return rc, out


def test_capacity_message_names_a_budget_that_serves(A, ctx, long):
    recs, full, models = long
    P = models(A.RUNS_GT, LIMIT)
    buf = np.frombuffer(recs, dtype=np.uint8)
    E = A.capi
    try:
        ctx.set_aggregate_scratch(1)
        rc, out = _raw_host(A, ctx, buf, [(0, 70010)], 70001, 1)
        assert rc == E.E_CAPACITY and np.all(out == SENT)
        msg = E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert msg.startswith("rolling_runs_windows: a window of 70001 samples"), msg
        need = int(msg.split("budget of ")[1].split(" bytes")[0])
        assert need == (70001 + 4 * 2048) * 16  # 8 bytes a sample and 8 of chunk partials; no large frame: no spill
        ctx.set_aggregate_scratch(need)
        rc, out = _raw_host(A, ctx, buf, [(0, 70010)], 70001, 1)
        assert rc == 0 and np.all(out[100:] == SENT)
        _assert_same(out[:100].view(A.WINDOW_RUNS), P.rolling([0], [70010], 70001, 1)[0], "the named budget")
        ctx.set_aggregate_scratch(1)
        rc, out = _raw_host(A, ctx, buf, [(0, 59392 + 15)], 59392, 1)  # the widest that the least budget holds
        assert rc == 0 and np.all(out[160:] == SENT)
        _assert_same(out[:160].view(A.WINDOW_RUNS), P.rolling([0], [59392 + 15], 59392, 1)[0], "widest")
        rc, out = _raw_host(A, ctx, buf, [(0, 59393 + 15)], 59393, 1)
        assert rc == E.E_CAPACITY and np.all(out == SENT)
    finally:
        ctx.set_aggregate_scratch(0)
    rc, out = _raw_host(A, ctx, buf, [(0, 70010)], 70001, 1)  # the default budget holds any width
    assert rc == 0 and np.all(out[100:] == SENT) and not np.any(out[:100:10] == SENT)


def test_errors_leave_the_result_untouched(A, ctx, torch, long):
    recs, full, models = long
    n = len(full)
    buf = np.frombuffer(recs, dtype=np.uint8)
    E = A.capi
    gt, nan = A.RUNS_GT, float("nan")
    cases = [([(0, 100)], 0, 1, gt, 1.0, "width outside"), ([(0, 100)], A.ROLLING_MAX_WIDTH + 1, 1, gt, 1.0, "width outside"),
             ([(0, 100)], 10, 0, gt, 1.0, "stride is 0"), ([(0, 100)], 10, 1, 6, 1.0, "unknown op"),
             ([(0, 100)], 10, 1, -1, 1.0, "unknown op"), ([(0, 100)], 10, 1, gt, nan, "limit is NaN"),
             ([(0, 100)], 0, 0, 6, nan, "unknown op"),  # the condition is checked first
             ([(n - 50, 100)], 10, 1, gt, 1.0, ""), ([(0, 20), (n + 1, 0)], 10, 1, gt, 1.0, ""),
             ([(2 ** 63, 2 ** 63)], 10, 1, gt, 1.0, ""), ([(0, 2 ** 33)], 1, 1, gt, 1.0, "")]
    for rg, w, s, op, limit, what in cases:
        rc, out = _raw_host(A, ctx, buf, rg, w, s, op, limit)
        msg = E.lib().atsc_ctx_last_error(ctx._h).decode()
        assert rc == E.E_INVALID and np.all(out == SENT), (rg, w, s, rc)
        assert not what or msg.startswith("rolling_runs_windows: " + what), msg  # the call's own checks name the call
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(buf.copy()).to("cuda")
    try:
        for rg, w, s, op, limit, what in cases:
            d = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
            b = np.array([x[0] for x in rg], dtype=np.uint64)
            c = np.array([x[1] for x in rg], dtype=np.uint64)
            p = C.POINTER(C.c_uint64)
            rc = E.lib().atsc_rolling_runs_windows_dev(ctx._h, dp._h, C.c_void_p(body.data_ptr()), len(rg), b.ctypes.data_as(p),
                                                       c.ctypes.data_as(p), w, s, op, limit, C.c_void_p(d.data_ptr()),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            assert rc == E.E_INVALID and bool((d == SENT).all()), (rg, w, s, rc)
    finally:
        dp.close()
    st = A.CompressedStream.from_bytes(ctx, A.compress_data(ctx, np.arange(1000.0), A.NOOP, 0))
    for w, op, limit in ((0, gt, 1.0), (5, 6, 1.0), (5, gt, nan)):
        with pytest.raises(A.AtscError) as e:
            st.rolling_runs_windows([0], [100], w, op, limit, 1)
        assert e.value.rc == E.E_INVALID
    rc, out = _raw_host(A, ctx, buf, [], 5, 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, buf, [(5, 0), (n, 0), (7, 4)], 5, 1)  # no range holds a window: no record
    assert rc == 0 and np.all(out == SENT)


def test_malformed_payload(A, ctx):
    n, nf = 256, 8
    x = H.synth_series(909, n * nf, klass=2)
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.05)), 0)
    good = ctx.decompress_host(recs)
    limit = float(np.median(good))
    frames = H.parse_bro_body(recs, with_count=False)
    pos = sum(len(_rec(f[1], f[2], f[3])) for f in frames[:3])
    rec3 = _rec(frames[3][1], frames[3][2], frames[3][3])
    pay = pos + len(rec3) - len(frames[3][3])
    assert recs[pay] == 15 and recs[pay + 1] < 200
    bad = bytearray(recs)
    bad[pay + 1] = 250  # frame 3: more stored bins than the transform has; the record walk stays valid
    bad = bytes(bad)
    P = M.Pyramid(good, A.RUNS_GT, limit)
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 20, 20), (5 * n + 3, 100), (3 * n + 5, 0)]
    b, c = [w[0] for w in outside], [w[1] for w in outside]
    got, _ = ctx.rolling_runs_windows_host(bad, b, c, 20, A.RUNS_GT, limit, 3)
    _assert_same(got, P.rolling(b, c, 20, 3)[0], "outside")
    bb = np.frombuffer(bad, dtype=np.uint8)
    for rg in ([(3 * n, 20)], [(0, nf * n)], [(0, 40), (3 * n - 19, 20)], [(4 * n - 20, 20), (6 * n, 50)]):
        rc, out = _raw_host(A, ctx, bb, rg, 20, 1, A.RUNS_GT, limit, n_out=nf * n)
        assert rc == A.capi.E_FORMAT and np.all(out == SENT), (rg, rc)


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


HEAD = ",samples,inside,runs,longest,longest_at,first_at,last_at,head,tail,excess"


def _check_rows(A, plain, text, first, want):
    """text: the .roll.csv with --rolling-runs; plain: the same call's without.  The rolling's columns are the plain
    file's, the columns behind them parse back to the records `want`, an empty cell being ATSC_RUNS_NONE"""
    lines, base = text.split("\n"), plain.split("\n")
    assert base[0] == first + ",count,min,max,sum,mean" and lines[0] == base[0] + HEAD and len(lines) == len(base)
    rows = [l.split(",") for l in lines[1:] if l]
    assert [",".join(r[:6]) for r in rows] == [l for l in base[1:] if l] and all(len(r) == 16 for r in rows)
    assert len(rows) == len(want) >= 2
    back = np.zeros(len(rows), dtype=A.WINDOW_RUNS)
    for k, name in enumerate(M.FIELDS):
        back[name] = [float(r[6 + k]) if k == 9 else A.RUNS_NONE if r[6 + k] == "" else int(r[6 + k]) for r in rows]
    _assert_same(back, want, "columns")


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
    limit = float(np.round(np.median(full)))
    hi = len(times) - 3
    for (t0, t1), spec, (w, s), (name, op) in (((times[10], times[hi]), "20:3", (20, 3), ("gt", A.RUNS_GT)),
                                               ((times[10], times[32]), "20", (20, 1), ("le", A.RUNS_LE))):
        for f in tmp_path.glob("win*"):
            f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--rolling", spec, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        plain = (tmp_path / "win.roll.csv").read_text()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--rolling", spec, "--rolling-runs", "%s:%r" % (name, limit), "-o", tmp_path / "win",
             tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.roll.csv"]
        at = np.flatnonzero((times >= t0) & (times <= t1))
        want = M.Pyramid(full, op, limit).rolling([int(at[0])], [len(at)], w, s)[0]
        assert len(want) == M.outputs(len(at), w, s)
        _check_rows(A, plain, (tmp_path / "win.roll.csv").read_text(), "timestamp", want)
    r = subprocess.run([csvc, "-u", "--from", str(times[10]), "--to", str(times[hi]), "--rolling-runs", "gt:1", str(tmp_path / "cpu.bro")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "'--rolling-runs' needs '--rolling'" in r.stderr


def test_command_line(A, ctx, golden_dir, tmp_path):
    atsc = os.path.join(os.path.dirname(A.__file__), "bin", "atsc")
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    limit = float(np.round(np.median(full)))
    empty = 0
    for spec, (b0, c0), (w, s), (name, op) in (("20", (0, len(full)), (20, 1), ("gt", A.RUNS_GT)),
                                               ("300:15", (100, 1500), (300, 15), ("ne", A.RUNS_NE)),
                                               ("3", (0, min(len(full), 400)), (3, 1), ("eq", A.RUNS_EQ))):
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--rolling", spec, tmp_path / "uptime.bro")
        plain = (tmp_path / "uptime.roll.csv").read_text()
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--rolling", spec, "--rolling-runs", "%s:%r" % (name, limit),
             tmp_path / "uptime.bro")
        want = M.Pyramid(full, op, limit).rolling([b0], [c0], w, s)[0]
        assert len(want) == M.outputs(c0, w, s) > 0
        empty += int((want["inside"] == 0).sum())
        _check_rows(A, plain, (tmp_path / "uptime.roll.csv").read_text(), "offset", want)
    assert empty > 0  # some position's cells were empty
    for bad in (("-u", "--rolling-runs", "gt:1"), ("-u", "--samples", "0:10", "--rolling-runs", "gt:1"),
                ("-u", "--samples", "0:10", "--buckets", "5", "--rolling-runs", "gt:1")):
        r = subprocess.run([atsc, *bad, str(tmp_path / "uptime.bro")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "'--rolling-runs' needs '--rolling'" in r.stderr, bad
    r = subprocess.run([atsc, "-u", "--samples", "0:10", "--rolling", "3", "--rolling-runs", "over:1", str(tmp_path / "uptime.bro")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "'--rolling-runs' wants OP:LIMIT" in r.stderr
