"""Windowed across on the GPU: every record of every case against the NumPy model of the contract
(tests/across_model.py) applied to the GPU's own full decodes -- count, min_at, max_at, min, max and sum bit for bit, any
NaN equal to any NaN, no tolerance.  Five streams of different framings (256-sample frames, 4096-sample frames, the
mixed-length ladder under several codecs, one with a large frame, one of hand-built Constant records), every one with a
zone of Constant records in front where all of them are NaN and where zeros of both signs meet in both orders; 64 Noop
streams; N = 1 against the window decode; one position through different ranges and strides; the shapes at which the
kernel takes another path (pairs, single positions, a full task from an odd sample, a result 8 bytes off a multiple of
16); budgets that cut a range
into pieces with a large frame across a piece's end; the host, device, stream and image calls; every error of the
contract with the result untouched; a malformed payload in one stream of three; the atsc command line."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import across_model as M
from tests import helpers as H

pytestmark = pytest.mark.gpu

LENS = [1, 7, 64, 128, 256, 300, 512, 513, 1024, 2048, 4096]  # the rolling suite's ladder
SENT = 0x5A5A5A5A5A5A5A5A
NAN = float("nan")
# the first 24 samples of each of the five streams, as Constant records: every stream NaN at 0 .. 7; zeros of both signs
# in both orders at 8 .. 15 (streams 0 and 1) and 12 .. 15 (stream 2); +Inf with -Inf at 16 .. 19
ZONES = [[(NAN, 8), (-0.0, 4), (0.0, 4), (np.inf, 4), (1.0, 4)],
         [(NAN, 8), (0.0, 4), (-0.0, 4), (-np.inf, 4), (1.0, 4)],
         [(NAN, 8), (NAN, 4), (0.0, 2), (-0.0, 2), (2.0, 4), (1.0, 4)],
         [(NAN, 8), (-0.0, 8), (NAN, 4), (0.5, 4)],
         [(NAN, 8), (NAN, 8), (np.inf, 4), (1.0, 4)]]
LONG = 200000


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


def _const_record(A, ctx, value, n):
    """a Constant record of n samples of `value` as it is (NaN, +-Inf, -0.0 included): the library's own 64-bit Constant
    record of a stand-in, with the stored double replaced"""
    r, _, _, _ = ctx.compress_host(np.full(n, 1.5), np.array([0, n], dtype=np.uint64), A.CONSTANT, False, 0.0, 0)
    assert r.endswith(struct.pack("<d", 1.5))
    return r[:-8] + struct.pack("<d", value)


def _comp(A, ctx, v, off, comp, bounded, me):
    return ctx.compress_host(v, off, comp, bounded, float(np.float32(me)), 0)[0]


@pytest.fixture(scope="module")
def five(A, ctx):
    """-> (records of the five streams, their full decodes, the length they share)"""
    zone = [b"".join(_const_record(A, ctx, v, n) for v, n in z) for z in ZONES]
    recs = []
    # 0: 256-sample frames under auto at 5 %
    recs.append(zone[0] + _comp(A, ctx, H.synth_series(4100, 40100, block=3000), H.frame_offsets(40100, 256), A.AUTO, True, 0.05))
    # 1: 4096-sample frames under FFT at 1 %
    recs.append(zone[1] + _comp(A, ctx, H.synth_series(4101, 40960, klass=1), H.frame_offsets(40960, 4096), A.FFT, True, 0.01))
    # 2: the mixed-length ladder under several codecs
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.uint64)
    r = zone[2]
    for m, (comp, bounded, me) in enumerate([(A.AUTO, True, 0.05), (A.FFT, True, 0.05), (A.POLYNOMIAL, True, 0.05),
                                             (A.RLE, False, 0.0), (A.NOOP, False, 0.0)]):
        v = H.synth_series(4110 + m, int(off[-1]), block=3000)
        if comp == A.RLE:
            v = np.round(v / 8.0) * 8.0
        r += _comp(A, ctx, v, off, comp, bounded, me)
    recs.append(r)
    # 3: one 8192-sample frame of the large tier between 4096-sample frames
    r = zone[3] + _comp(A, ctx, H.synth_series(4120, 16384, block=5000), H.frame_offsets(16384, 4096), A.AUTO, True, 0.05)
    r += _comp(A, ctx, H.synth_series(4121, 8192, klass=1), np.array([0, 8192], dtype=np.uint64), A.FFT, True, 0.01)
    r += _comp(A, ctx, H.synth_series(4122, 16384, block=5000), H.frame_offsets(16384, 4096), A.AUTO, True, 0.05)
    recs.append(r)
    # 4: hand-built Constant records only
    rng = np.random.default_rng(41)
    values = [1.0, NAN, -0.0, 2.5, np.inf, -7.0, -np.inf, 0.0, 3.0, NAN, -0.0, 0.0]
    r, n, k = zone[4], 24, 0
    while n < 40050:
        m = int(rng.integers(1, 3000))
        r += _const_record(A, ctx, values[k % len(values)], m)
        n, k = n + m, k + 1
    recs.append(r)
    fulls = [ctx.decompress_host(x) for x in recs]
    total = min(len(f) for f in fulls)
    assert 40000 <= total <= 41000 and len({len(f) for f in fulls}) > 1
    return recs, fulls, total


def _words(r):
    """a record array as 64-bit words, every NaN as one NaN"""
    w = np.ascontiguousarray(r).view(np.uint64).reshape(-1, 4).copy()
    f = w.view(np.float64)
    w[:, 1:][np.isnan(f[:, 1:])] = np.float64("nan").view(np.uint64)
    return w


def _assert_same(got, want, label):
    assert len(got) == len(want), (label, len(got), len(want))
    a, b = _words(got), _words(want)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert len(bad) == 0, (label, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


def _ranges(total):
    """ranges that begin odd and even, overlap, come unsorted, are empty, have count == 1, end at the shortest stream's last
    sample and (last) span the whole of it"""
    return [(4096, 5000), (1, 2051), (4500, 3000), (777, 0), (30001, 1), (2047, 4098), (total - 1235, 1235), (total, 0),
            (0, 40), (9, 10), (0, total)]


def test_the_inputs_hold_the_edge_cases(five):
    recs, fulls, total = five
    for n in (1, 2, 3, 5):
        assert np.all([np.isnan(f[:8]).all() for f in fulls[:n]])  # every stream NaN
    a, b = fulls[0], fulls[1]
    neg_first = (a[:24] == 0.0) & np.signbit(a[:24]) & (b[:24] == 0.0) & ~np.signbit(b[:24])
    pos_first = (a[:24] == 0.0) & ~np.signbit(a[:24]) & (b[:24] == 0.0) & np.signbit(b[:24])
    assert neg_first.sum() == 4 and pos_first.sum() == 4
    assert np.isposinf(a[16:20]).all() and np.isneginf(b[16:20]).all()
    assert np.isnan(fulls[4]).sum() > 1000 and np.isinf(fulls[4]).sum() > 1000


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_every_record_matches_the_model(A, ctx, five, n):
    recs, fulls, total = five
    rg = _ranges(total)
    b, c = [x[0] for x in rg], [x[1] for x in rg]
    for s in (1, 2, 7, 5000):
        got, off = ctx.across_windows_host(recs[:n], b, c, s)
        want, woff = M.across(fulls[:n], b, c, s)
        assert off.tolist() == woff.tolist() and got.dtype == A.ACROSS_RECORD
        assert off[3] == off[4] and off[5] - off[4] == 1 and off[7] == off[8]  # empty: none; count == 1: one
        _assert_same(got, want, (n, s))
    # the zone: all NaN, then the zero ties in both orders
    z, _ = ctx.across_windows_host(recs[:n], [0], [24], 1)
    assert np.all(z["count"][:8] == 0) and np.all(z["min_at"][:8] == 0xFFFF) and np.all(z["max_at"][:8] == 0xFFFF)
    assert np.isnan(z["min"][:8]).all() and np.isnan(z["max"][:8]).all() and np.all(z["sum"][:8].view(np.uint64) == 0)
    if n >= 2:
        assert np.signbit(z["min"][8:12]).all() and not np.signbit(z["min"][12:16]).any()
        assert np.all(z["min_at"][8:16] == 0) and np.all(z["max_at"][8:16] == 0)
        assert np.isnan(z["sum"][16:20]).all() and np.all(z["max_at"][16:20] == 0) and np.all(z["min_at"][16:20] == 1)


def test_sixty_four_streams(A, ctx):
    rng = np.random.default_rng(64)
    n, ns = 6000, 64
    recs, fulls = [], []
    # (Noop stores rounded integers, a NaN among them as 0: the holes are Constant records of NaN between the Noop frames)
    holes = {m: _const_record(A, ctx, NAN, m) for m in (1, 5, 37)}
    for k in range(ns):
        x = np.round(rng.normal(0, 1, n) * 10.0 ** rng.integers(2, 6, n))
        r, at = b"", 0
        for i, m in enumerate(holes):
            cut = 1000 + 1500 * i + int(rng.integers(0, 1000))
            r += _comp(A, ctx, x[at:cut], H.frame_offsets(cut - at, 1024 + 64 * (k % 5)), A.NOOP, False, 0.0) + holes[m]
            at = cut + m
        recs.append(r + _comp(A, ctx, x[at:], H.frame_offsets(n - at, 1024 + 64 * (k % 5)), A.NOOP, False, 0.0))
        fulls.append(ctx.decompress_host(recs[-1]))
        assert len(fulls[-1]) == n and np.isnan(fulls[-1]).sum() == 43
    b, c = [0, 1, 4001], [n, 3000, 1999]
    cols = np.array(fulls)
    for s in (1, 3):
        got, off = ctx.across_windows_host(recs, b, c, s)
        _assert_same(got, M.across(fulls, b, c, s)[0], (64, s))
        rev, _ = ctx.across_windows_host(recs[::-1], b, c, s)
        _assert_same(rev, M.across(fulls[::-1], b, c, s)[0], (64, s, "reversed"))
        assert np.array_equal(got["count"], rev["count"])
        assert got["min"].tobytes() == rev["min"].tobytes() and got["max"].tobytes() == rev["max"].tobytes()
        # where the extreme is held by one stream only, the reversed list names it from the other end
        idx = np.concatenate([b[i] + s * np.arange(int(off[i + 1] - off[i])) for i in range(len(b))])
        with np.errstate(invalid="ignore"):
            one_min = (cols[:, idx] == got["min"]).sum(axis=0) == 1
            one_max = (cols[:, idx] == got["max"]).sum(axis=0) == 1
        assert one_min.mean() > 0.9 and one_max.mean() > 0.9
        assert np.all(rev["min_at"][one_min] == ns - 1 - got["min_at"][one_min])
        assert np.all(rev["max_at"][one_max] == ns - 1 - got["max_at"][one_max])


def test_one_stream_against_the_window_decode(A, ctx, five):
    recs, fulls, total = five
    for k in (2, 4):
        b0, c0 = 3, total - 3
        got, off = ctx.across_windows_host([recs[k]], [b0], [c0], 1)
        x = ctx.decompress_window_host(recs[k], b0, c0)
        ok = ~np.isnan(x)
        assert ok.any() and (~ok).any()
        assert np.array_equal(got["count"], ok.astype(np.uint32))
        for f in ("min", "max", "sum"):
            assert got[f][ok].tobytes() == x[ok].tobytes(), (k, f)
        assert np.all(got["min_at"][ok] == 0) and np.all(got["max_at"][~ok] == 0xFFFF)


def test_one_position_through_different_ranges_and_strides(A, ctx, five):
    recs, fulls, total = five
    for q in (12345, 17, 8192):
        ref, _ = ctx.across_windows_host(recs, [q], [1], 1)
        assert len(ref) == 1
        _assert_same(ref, M.across(fulls, [q], [1], 1)[0], q)
        for b, c, s in ((q - 14 if q >= 14 else q % 7, 100, 7), (q % 5000, total - q % 5000, 5000), (q, total - q, 2),
                        (1, total - 1, q - 1), (q - 1, 2, 1), (q % 2, q + 2, 2)):
            got, off = ctx.across_windows_host(recs, [0, b, 2048], [3, c, 30], s)
            j = int(off[1]) + (q - b) // s
            assert (q - b) % s == 0 and j < int(off[2]) and got[j: j + 1].tobytes() == ref.tobytes(), (q, b, c, s)


@pytest.mark.parametrize("shift", [0, 1])
def test_shapes_where_the_kernel_takes_another_path(A, ctx, torch, five, shift):
    """ranges with an odd and an even first sample of every length around a pair, a wavefront and a task -- one position
    and two positions from an odd sample (a head alone; a head and a tail, no pair), a full task from an odd sample --
    at stride 1 (pairs) and at another; the result at a multiple of 16 bytes and 8 bytes off one"""
    recs, fulls, total = five
    task = 512  # ACR_TASK
    rg = [(b0, n) for b0 in (1001, 1000) for n in (0, 1, 2, 3, 63, 64, 65, task - 1, task, task + 1)] + [(2047, 2), (total, 0)]
    b, c = [x[0] for x in rg], [x[1] for x in rg]
    bodies = [torch.from_numpy(np.frombuffer(r, dtype=np.uint8).copy()).to("cuda") for r in recs]
    dps = [A.DPlan(ctx, r) for r in recs]
    try:
        for s in (1, 3):
            want, woff = M.across(fulls, b, c, s)
            d = torch.full((shift + 4 * len(want) + 8,), SENT, dtype=torch.int64, device="cuda")
            doff = dps[0].across_windows(bodies[0], dps[1:], bodies[1:], b, c, d[shift:], s,
                                         torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert (d.data_ptr() + 8 * shift) % 16 == 8 * shift
            h = d.cpu().numpy().view(np.uint64)
            assert doff.tolist() == woff.tolist() and np.all(h[:shift] == SENT) and np.all(h[shift + 4 * len(want):] == SENT)
            _assert_same(h[shift: shift + 4 * len(want)].view(A.ACROSS_RECORD), want, (s, shift))
    finally:
        for dp in dps:
            dp.close()


def _pieces(n, budget, n_in, n_large):
    """the pieces of a range of n samples from sample 0 by DESIGN.md's piece arithmetic: the budget less two large frames'
    room for every stream with large frames, shared by the n_in regions, in whole tiles of 2048 and at least 65536"""
    want = budget // 8 - n_large * 2 * 131072
    piece = max(65536, want // n_in // 2048 * 2048 if want > 0 else 0)
    return -(-(-(-n // 2048) * 2048) // piece)


def test_pieces_do_not_change_the_bytes(A, ctx):
    rng = np.random.default_rng(29)
    recs, fulls = [], []
    for k in range(3):
        x = np.round(rng.normal(0, 1, LONG) * 10.0 ** rng.integers(0, 6, LONG))
        recs.append(_comp(A, ctx, x, H.frame_offsets(LONG, 4096), A.NOOP, False, 0.0))
    # the large-frame stream: an 8192-sample frame over [63488, 71680), across the least budget's first piece end at 65536
    x = np.round(rng.normal(0, 100, LONG), 3)
    r = _comp(A, ctx, x[:63488], H.frame_offsets(63488, 4096), A.NOOP, False, 0.0)
    r += _comp(A, ctx, H.synth_series(4130, 8192, klass=1), np.array([0, 8192], dtype=np.uint64), A.FFT, True, 0.01)
    r += _comp(A, ctx, x[71680:], H.frame_offsets(LONG - 71680, 4096), A.NOOP, False, 0.0)
    recs.append(r)
    fulls = [ctx.decompress_host(v) for v in recs]
    assert all(len(f) == LONG for f in fulls)
    b, c = [0, 90001], [LONG, 30000]
    want, _ = M.across(fulls, b, c, 1)
    want7, _ = M.across(fulls, b, c, 7)
    ref, _ = ctx.across_windows_host(recs, b, c, 1)
    _assert_same(ref, want, "default")
    two, least = 8 * (4 * 100352 + 2 * 131072), 1
    assert _pieces(LONG, 8 * (2 ** 24 + 2 * 131072), 4, 1) == 1 and _pieces(LONG, two, 4, 1) == 2 and _pieces(LONG, least, 4, 1) == 4
    try:
        for budget in (two, least):
            ctx.set_aggregate_scratch(budget)
            got, _ = ctx.across_windows_host(recs, b, c, 1)
            assert got.tobytes() == ref.tobytes(), budget
            got7, _ = ctx.across_windows_host(recs, b, c, 7)
            _assert_same(got7, want7, (budget, 7))
    finally:
        ctx.set_aggregate_scratch(0)


def test_host_device_stream_and_image_calls_agree(A, ctx, torch):
    bros, fulls = [], []
    for k in range(3):
        x = H.synth_series(4140 + k, 50000 + 100 * k, block=7000)
        bros.append(A.compress_data(ctx, x, A.AUTO, 3))
        fulls.append(A.decompress_data(ctx, bros[-1]))
    p0 = [H.varint_decode(bro, 9)[1] for bro in bros]
    bodies = [torch.from_numpy(np.frombuffer(bro[p:], dtype=np.uint8).copy()).to("cuda") for bro, p in zip(bros, p0)]
    dps = [A.DPlan(ctx, bro[p:]) for bro, p in zip(bros, p0)]
    sts = [A.CompressedStream.from_bytes(ctx, bro) for bro in bros]
    try:
        for s in (1, 7):
            b, c = [30001, 20000, 47000], [15000, 12001, 100]  # begins far into the streams: the host call uploads a part
            want, woff = M.across(fulls, b, c, s)
            via_bro, off = A.across_data_windows(ctx, bros, b, c, s)
            _assert_same(via_bro, want, s)
            assert off.tolist() == woff.tolist()
            host, _ = ctx.across_windows_host([bro[9:] for bro in bros], b, c, s, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), s
            plain, _ = ctx.across_windows_host([bro[p:] for bro, p in zip(bros, p0)], b, c, s)
            assert plain.tobytes() == via_bro.tobytes(), s
            assert sts[0].across_windows(sts[1:], b, c, s)[0].tobytes() == via_bro.tobytes(), s
            d = torch.full((4 * len(want) + 8,), SENT, dtype=torch.int64, device="cuda")
            doff = dps[0].across_windows(bodies[0], dps[1:], bodies[1:], b, c, d, s, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            h = d.cpu().numpy()
            assert doff.tolist() == woff.tolist() and np.all(h[4 * len(want):] == SENT)
            assert h[: 4 * len(want)].tobytes() == via_bro.tobytes(), s
        # the same plan and the same stream twice in a list
        d = torch.full((4 * 100 + 8,), SENT, dtype=torch.int64, device="cuda")
        dps[0].across_windows(bodies[0], [dps[1], dps[0]], [bodies[1], bodies[0]], [40000], [100], d, 1,
                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        twice = M.across([fulls[0], fulls[1], fulls[0]], [40000], [100], 1)[0]
        _assert_same(d.cpu().numpy()[:400].view(A.ACROSS_RECORD), twice, "twice")
        _assert_same(sts[0].across_windows([sts[1], sts[0]], [40000], [100], 1)[0], twice, "twice, streams")
    finally:
        for dp in dps:
            dp.close()


def _ptrs(values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _raw_host(A, ctx, bufs, rg, s, n_streams=None, null_list=False, null_entry=None, n_out=16):
    out = np.full(4 * n_out, SENT, dtype=np.uint64)
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    ptr = [x.ctypes.data for x in bufs]
    if null_entry is not None:
        ptr[null_entry] = None
    lens = np.array([len(x) for x in bufs], dtype=np.uint64)
    flags = np.zeros(max(len(bufs), 1), dtype=np.int32)
    rc = A.capi.lib().atsc_across_windows(ctx._h, len(bufs) if n_streams is None else n_streams, None if null_list else _ptrs(ptr),
                                          lens.ctypes.data_as(p), flags.ctypes.data_as(C.POINTER(C.c_int32)), len(rg),
                                          b.ctypes.data_as(p), c.ctypes.data_as(p), s, C.c_void_p(out.ctypes.data))
    return rc, out


def _raw_dev(A, ctx, torch, dps, bodies, rg, s, n_streams=None, null_list=False, null_entry=None):
    d = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    plans, ptr = [x._h.value for x in dps], [x.data_ptr() for x in bodies]
    if null_entry is not None:
        plans[null_entry] = None
    rc = A.capi.lib().atsc_across_windows_dev(ctx._h, len(dps) if n_streams is None else n_streams, None if null_list else _ptrs(plans),
                                              _ptrs(ptr), len(rg), b.ctypes.data_as(p), c.ctypes.data_as(p), s,
                                              C.c_void_p(d.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool((d == SENT).all())


def test_errors_leave_the_result_untouched(A, ctx, torch):
    rng = np.random.default_rng(7)
    E = A.capi
    lens = (9000, 9000, 6000)  # only stream 2 of 3 is too short for a range past 6000
    recs = [_comp(A, ctx, rng.normal(0, 1, n), H.frame_offsets(n, 1024), A.NOOP, False, 0.0) for n in lens]
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in recs]
    cases = [dict(rg=[(0, 10)], s=1, n_streams=0), dict(rg=[(0, 10)], s=1, n_streams=65), dict(rg=[(0, 10)], s=1, null_list=True),
             dict(rg=[(0, 10)], s=1, null_entry=1), dict(rg=[(0, 10)], s=0), dict(rg=[(0, 2 ** 33)], s=1),
             dict(rg=[(0, 2 ** 32 - 1), (0, 5)], s=1), dict(rg=[(0, 7000)], s=1), dict(rg=[(0, 10), (5999, 2)], s=1),
             dict(rg=[(0, 10), (6001, 0)], s=1), dict(rg=[(2 ** 63, 2 ** 63)], s=1), dict(rg=[(2 ** 64 - 1, 2)], s=3)]
    for kw in cases:
        rc, out = _raw_host(A, ctx, bufs, **kw)
        assert rc == E.E_INVALID and np.all(out == SENT), (kw, rc)
    ctx2 = A.Context(0)
    dps = [A.DPlan(ctx, r) for r in recs]
    bodies = [torch.from_numpy(x.copy()).to("cuda") for x in bufs]
    other = A.DPlan(ctx2, recs[0])
    try:
        for kw in cases:
            rc, untouched = _raw_dev(A, ctx, torch, dps, bodies, **kw)
            assert rc == E.E_INVALID and untouched, (kw, rc)
        rc, untouched = _raw_dev(A, ctx, torch, [dps[0], other, dps[1]], [bodies[0], bodies[0], bodies[1]], [(0, 10)], 1)
        assert rc == E.E_INVALID and untouched  # plans of different contexts
        sa, sb = A.CompressedStream.from_bytes(ctx, A.bro_prefix(9) + recs[0]), A.CompressedStream.from_bytes(ctx2, A.bro_prefix(9) + recs[0])
        with pytest.raises(A.AtscError) as ei:
            sa.across_windows([sb], [0], [10])  # streams of different contexts
        assert ei.value.rc == E.E_INVALID
        del sa, sb
        # the two good streams alone hold the range; within all three, n_windows == 0 and empty ranges write nothing
        rc, untouched = _raw_dev(A, ctx, torch, dps[:2], bodies[:2], [(0, 7000)], 1000)
        assert rc == 0 and not untouched
    finally:
        other.close()
        for dp in dps:
            dp.close()
        ctx2.close()
    rc, out = _raw_host(A, ctx, bufs[:2], [(0, 7000)], 1000)
    assert rc == 0 and np.all(out[28:] == SENT) and not np.any(out[:28] == SENT)
    rc, out = _raw_host(A, ctx, bufs, [], 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufs, [(5, 0), (6000, 0)], 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufs, [(5999, 1)], 1)  # the shortest stream's last sample
    assert rc == 0 and np.all(out[4:] == SENT) and (out[0] & 0xFFFFFFFF) == 3


def test_malformed_payload_in_one_stream_of_three(A, ctx):
    n, nf = 256, 8
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs = [_comp(A, ctx, H.synth_series(920 + k, n * nf, klass=2), off, A.FFT, True, 0.05) for k in range(3)]
    good = [ctx.decompress_host(r) for r in recs]
    frames = H.parse_bro_body(recs[1], with_count=False)
    pos = sum(len(_rec(f[1], f[2], f[3])) for f in frames[:3])
    rec3 = _rec(frames[3][1], frames[3][2], frames[3][3])
    pay = pos + len(rec3) - len(frames[3][3])
    assert recs[1][pay] == 15 and recs[1][pay + 1] < 200
    bad = bytearray(recs[1])
    bad[pay + 1] = 250  # stream 1, frame 3: more stored bins than the transform has; the record walk stays valid
    lst = [recs[0], bytes(bad), recs[2]]
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 20, 20), (5 * n + 3, 100), (3 * n + 5, 0)]
    b, c = [w[0] for w in outside], [w[1] for w in outside]
    for s in (1, 3):
        got, _ = ctx.across_windows_host(lst, b, c, s)
        _assert_same(got, M.across(good, b, c, s)[0], ("outside", s))
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in lst]
    for rg in ([(3 * n, 20)], [(0, nf * n)], [(0, 40), (3 * n - 19, 20)], [(4 * n - 20, 20), (6 * n, 50)]):
        for s in (1, 300):
            rc, out = _raw_host(A, ctx, bufs, rg, s, n_out=nf * n)
            assert rc == A.capi.E_FORMAT and np.all(out == SENT), (rg, s, rc)


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def test_command_line(A, ctx, golden_dir, tmp_path):
    atsc = os.path.join(os.path.dirname(A.__file__), "bin", "atsc")
    names = ("uptime", "memory_used", "go_gc_heap_goal_bytes")
    bros = []
    for name in names:
        src = tmp_path / (name + ".wbro")
        src.write_bytes(open(os.path.join(golden_dir, "wbros", name + ".wbro"), "rb").read())
        _run(atsc, "--compressor", "fft", "-e", "1", src)
        bros.append((tmp_path / (name + ".bro")).read_bytes())
    total = min(len(A.decompress_data(ctx, b)) for b in bros)
    assert total > 1000
    paths = [tmp_path / (name + ".bro") for name in names]
    for k, (b0, c0), s in ((2, (0, total), None), (3, (100, total - 100), None), (3, (7, 1000), 15), (2, (total - 1, 1), 4)):
        listed = ",".join(str(p) for p in paths[1:k])
        stride = [] if s is None else ["--across-stride", s]
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--across", listed, *stride, paths[0])
        lines = (tmp_path / "uptime.across.csv").read_text().split("\n")
        assert lines[0] == "offset,count,min,min_at,max,max_at,sum,mean"
        rows = [l.split(",") for l in lines[1:] if l]
        s = s or 1
        want, _ = A.across_data_windows(ctx, bros[:k], [b0], [c0], s)
        assert len(rows) == len(want) == M.outputs(c0, s) > 0
        assert [int(r[0]) for r in rows] == [j * s for j in range(len(rows))]
        back = np.zeros(len(rows), dtype=A.ACROSS_RECORD)
        back["count"] = [int(r[1]) for r in rows]
        for col, name in ((2, "min"), (4, "max"), (6, "sum")):
            back[name] = [float(r[col]) for r in rows]
        for col, name in ((3, "min_at"), (5, "max_at")):
            back[name] = [int(r[col]) if r[col] else 0xFFFF for r in rows]
        _assert_same(back, want, (k, b0, c0, s))
        assert np.all(want["count"] == k)
        assert [float(r[7]) for r in rows] == [float(v["sum"]) / int(v["count"]) for v in want]
    one = str(paths[1])
    for bad in (("-u", "--across", one), ("-u", "--samples", "0:10", "--buckets", "5", "--across", one),
                ("-u", "--samples", "0:10", "--rolling", "5", "--across", one), ("-u", "--samples", "0:10", "--where", "gt:0", "--across", one),
                ("-u", "--samples", "0:10", "--across", one + ",,"), ("-u", "--samples", "0:10", "--across", ""),
                ("-u", "--samples", "0:10", "--across", ",".join([one] * 64)),
                ("-u", "--samples", "0:10", "--across", one, "--across-stride", "0"), ("-u", "--samples", "0:10", "--across-stride", "2")):
        r = subprocess.run([atsc, *bad, str(paths[0])], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
    _run(atsc, "-u", "--samples", "0:10", "--across", ",".join([one] * 63), paths[0])  # 63 listed files: 64 streams
