"""Windowed across moments on the GPU: every record of every case against the NumPy model of the contract
(tests/across_moments_model.py) applied to the GPU's own full decodes -- bit for bit, any NaN equal to any NaN, no
tolerance, no position left out.  Five short streams (NaN runs, +-Inf, zeros of both signs, a constant series, a series
at 1e9 +- 1e-3, one series twice, three framings) for N = 1, 2, 3, 5; 64 plans over eight Noop series with NaN holes for
N = 8 .. 64; the ranges, strides and result alignments at which the kernel takes another path; N = 1 against the window
decode, count against the across' own, one position through different ranges and strides; budgets that cut a range
into pieces with a large frame across a piece's end; the host, device, stream and image calls;
atsc_across_moments_merge over the device's records; every error of the contract with the result untouched; a malformed
payload in one stream of three; the atsc command line."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import across_model as AM
from tests import across_moments_model as M
from tests import helpers as H

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A5A5A5A5A
NAN = float("nan")
# the first 24 samples of each of the five streams, as Constant records: every stream NaN at 0 .. 7; zeros of both signs
# at 8 .. 15; +Inf with -Inf at 16 .. 19 (streams 0 and 1 are one series: stream 2 brings the -Inf)
ZONES = [[(NAN, 8), (-0.0, 4), (0.0, 4), (np.inf, 4), (1.0, 4)],
         [(NAN, 8), (NAN, 4), (0.0, 2), (-0.0, 2), (-np.inf, 4), (1.0, 4)],
         [(NAN, 8), (-0.0, 8), (NAN, 4), (0.5, 4)],
         [(NAN, 8), (NAN, 8), (np.inf, 4), (1.0, 4)]]
LONG = 200000
TASK = 512  # positions per task of the position kernel (ACR_TASK)


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
    rng = np.random.default_rng(53)
    recs = []
    # 0 and 1: one series, 256-sample frames under auto at 5 %: every column holds a tie
    r = zone[0] + _comp(A, ctx, H.synth_series(5100, 5100, block=1500), H.frame_offsets(5100, 256), A.AUTO, True, 0.05)
    recs += [r, r]
    # 2: 1e9 +- 1e-3 in 256-sample frames, kept exactly (RLE)
    recs.append(zone[1] + _comp(A, ctx, 1e9 + rng.normal(0, 1e-3, 5200), H.frame_offsets(5200, 256), A.RLE, False, 0.0))
    # 3: a constant series in 4096-sample frames
    recs.append(zone[2] + _comp(A, ctx, np.full(5300, 1234.5678), H.frame_offsets(5300, 4096), A.CONSTANT, False, 0.0))
    # 4: hand-built Constant records of any length: NaN runs, +-Inf, zeros of both signs
    values = [1.0, NAN, -0.0, 2.5, np.inf, -7.0, -np.inf, 0.0, 3.0, NAN, -0.0, 0.0]
    r, n, k = zone[3], 24, 0
    while n < 5050:
        m = int(rng.integers(1, 400))
        r += _const_record(A, ctx, values[k % len(values)], m)
        n, k = n + m, k + 1
    recs.append(r)
    fulls = [ctx.decompress_host(x) for x in recs]
    total = min(len(f) for f in fulls)
    assert 5000 <= total <= 5500 and len({len(f) for f in fulls}) > 1
    return recs, fulls, total


@pytest.fixture(scope="module")
def many(A, ctx):
    """-> (records of 64 streams, their full decodes): eight Noop series of 3000 samples with Constant-NaN holes, in five
    framings, each listed eight times"""
    rng = np.random.default_rng(64)
    n = 3000
    recs, fulls = [], []
    # (Noop stores rounded integers, a NaN among them as 0: the holes are Constant records of NaN between the Noop frames)
    holes = {m: _const_record(A, ctx, NAN, m) for m in (1, 5, 37)}
    for k in range(8):
        x = np.round(rng.normal(0, 1, n) * 10.0 ** rng.integers(2, 6, n))
        r, at = b"", 0
        for i, m in enumerate(holes):
            cut = 500 + 750 * i + int(rng.integers(0, 500))
            r += _comp(A, ctx, x[at:cut], H.frame_offsets(cut - at, 512 + 64 * (k % 5)), A.NOOP, False, 0.0) + holes[m]
            at = cut + m
        recs.append(r + _comp(A, ctx, x[at:], H.frame_offsets(n - at, 512 + 64 * (k % 5)), A.NOOP, False, 0.0))
        fulls.append(ctx.decompress_host(recs[-1]))
        assert len(fulls[-1]) == n and np.isnan(fulls[-1]).sum() == 43
    order = [(3 * j + j // 8) % 8 for j in range(64)]  # every series eight times, never twice in a row
    return [recs[j] for j in order], [fulls[j] for j in order]


def _assert_same(got, want, label):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.shape == want.shape and got.dtype == want.dtype == M.dtype, (label, got.shape, want.shape, got.dtype)
    if M.same(got, want):
        return
    bad = np.argwhere((M.words(got) != M.words(want)).any(axis=1))[:, 0]
    assert False, (label, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


def _ranges(total):
    """ranges that begin odd and even, overlap, come unsorted, are empty, have count == 1, end at the shortest stream's last
    sample and (last) span the whole of it"""
    return [(2048, 1500), (1, 2051), (2500, 1000), (777, 0), (3001, 1), (2047, 2050), (total - 1235, 1235), (total, 0),
            (0, 40), (9, 10), (0, total)]


def test_the_inputs_hold_the_edge_cases(five, many):
    recs, fulls, total = five
    x = np.array([f[:total] for f in fulls])
    assert np.isnan(x[:, :8]).all()  # every stream NaN: holds for every N
    some = np.isnan(x[:, :24])
    assert (some.any(axis=0) & ~some.all(axis=0)).sum() >= 4  # NaN in some streams only
    assert recs[0] == recs[1] and fulls[0].tobytes() == fulls[1].tobytes()  # one series twice: every column has a tie
    zero = x[:, 8:16] == 0.0
    assert (zero & np.signbit(x[:, 8:16])).any() and (zero & ~np.signbit(x[:, 8:16])).any()  # zeros of both signs
    assert np.isposinf(x[0, 16:20]).all() and np.isneginf(x[2, 16:20]).all()  # +Inf with -Inf in one column
    assert np.isnan(fulls[4]).sum() > 300 and np.isposinf(fulls[4]).sum() > 100 and np.isneginf(fulls[4]).sum() > 100
    assert np.isnan(x[4]).any() and (~np.isnan(x[4])).any()
    near = x[2, 24:]  # the series at 1e9 +- 1e-3: a spread that a sum of squares would lose
    assert np.all(np.abs(near - 1e9) < 1e-2) and 1e-4 < np.std(near - 1e9) < 1e-2 and len(np.unique(near)) > 1000
    assert np.all(x[3, 24:] == 1234.5678)  # the constant series
    assert len({len(f) for f in fulls}) > 1
    # the 64 streams: eight series, each eight times; NaN holes in every one
    y = np.array(many[1])
    assert len({f.tobytes() for f in many[1]}) == 8 and np.isnan(y).any(axis=0).sum() > 100
    assert all(many[1][j].tobytes() != many[1][j + 1].tobytes() for j in range(63))


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_every_record_matches_the_model(A, ctx, five, n):
    recs, fulls, total = five
    rg = _ranges(total)
    b, c = [x[0] for x in rg], [x[1] for x in rg]
    for s in (1, 2, 7, 5000):
        got, off = ctx.across_moments_windows_host(recs[:n], b, c, s)
        want, woff = M.across_moments(fulls[:n], b, c, s)
        assert off.tolist() == woff.tolist() == A.across_offsets(c, s).tolist()
        assert off[3] == off[4] and off[5] - off[4] == 1 and off[7] == off[8]  # empty: none; count == 1: one
        assert got.dtype == A.ACROSS_MOMENTS
        _assert_same(got, want, (n, s))
        assert np.all(got["count"] + got["nans"] == n)
    # the zone: NaN, NaN where all streams are NaN; a column of equal values has no spread, exactly
    z, _ = ctx.across_moments_windows_host(recs[:n], [0], [24], 1)
    assert np.all(z["count"][:8] == 0) and np.all(z["nans"][:8] == n) and np.isnan(z["mean"][:8]).all() and np.isnan(z["m2"][:8]).all()
    if n <= 2:  # streams 0 and 1 are one series
        rest, _ = ctx.across_moments_windows_host(recs[:n], [24], [total - 24], 1)
        assert np.all(rest["m2"] == 0.0) and rest["mean"].tobytes() == fulls[0][24:total].tobytes()


def test_one_stream_against_the_window_decode(A, ctx, five):
    recs, fulls, total = five
    for j in (2, 4):
        b0, c0 = 3, total - 3
        x = ctx.decompress_window_host(recs[j], b0, c0)
        ok = ~np.isnan(x)
        assert ok.any() and (~ok).any()
        got, off = ctx.across_moments_windows_host([recs[j]], [b0], [c0], 1)
        assert got.shape == (c0,) and np.array_equal(got["count"], ok.astype(np.uint32)) and np.all(got["count"] + got["nans"] == 1)
        fin = ok & np.isfinite(x)
        assert got["mean"][ok].tobytes() == x[ok].tobytes() and np.all(got["m2"][ok] == 0.0) and not np.signbit(got["m2"][ok]).any()
        assert np.isnan(got["mean"][~ok]).all() and np.isnan(got["m2"][~ok]).all() and fin.any()


@pytest.mark.parametrize("n", [8, 9, 16, 17, 33, 63, 64])
def test_many_streams(A, ctx, many, n):
    recs, fulls = many
    recs, fulls = recs[:n], fulls[:n]
    b, c = [0, 1, 2001], [3000, 1500, 999]
    for s in (1, 3):
        got, off = ctx.across_moments_windows_host(recs, b, c, s)
        want, woff = M.across_moments(fulls, b, c, s)
        assert off.tolist() == woff.tolist()
        _assert_same(got, want, (n, s))
        # the across' own count
        acr, aoff = ctx.across_windows_host(recs, b, c, s)
        assert aoff.tolist() == off.tolist() and np.array_equal(got["count"], acr["count"]) and np.all(got["count"] + got["nans"] == n)
        assert (got["nans"] > 0).any() and (got["count"] == n).any()


def test_shapes_where_the_kernel_takes_another_path(A, ctx, torch, five):
    """ranges with an odd and an even first sample of every length around a wavefront and a task; a full task from an odd
    sample (the pairs fill every lane, the two single positions wrap); strides on both sides of a wavefront and beyond a
    range; results at a multiple of 16 bytes and 8 bytes off one"""
    recs, fulls, total = five
    lengths = [0, 1, 2, 63, 64, 65, 129, TASK - 1, TASK, TASK + 1]
    rg = [(b0, n) for b0 in (1001, 1000) for n in lengths]
    rg += [(1, 2 * TASK + 6), (2, 2 * TASK + 6), (1000, 65), (1010, 3), (total - TASK - 1, TASK + 1), (total, 0), (2047, 2)]
    b, c = [x[0] for x in rg], [x[1] for x in rg]
    bodies = [torch.from_numpy(np.frombuffer(r, dtype=np.uint8).copy()).to("cuda") for r in recs]
    dps = [A.DPlan(ctx, r) for r in recs]
    try:
        for s in (1, 2, 3, 64, 2 * TASK + 7):
            want, woff = M.across_moments(fulls, b, c, s)
            host, off = ctx.across_moments_windows_host(recs, b, c, s)
            assert off.tolist() == woff.tolist()
            _assert_same(host, want, ("host", s))
            for shift in (0, 1):
                d = torch.full((shift + 3 * len(want) + 8,), SENT, dtype=torch.int64, device="cuda")
                rows, doff = dps[0].across_moments_windows(bodies[0], dps[1:], bodies[1:], b, c, d[shift:], s,
                                                           torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert (d.data_ptr() + 8 * shift) % 16 == 8 * shift
                h = d.cpu().numpy().view(np.uint64)
                assert doff.tolist() == woff.tolist() and np.all(h[:shift] == SENT) and np.all(h[shift + 3 * len(want):] == SENT)
                assert h[shift: shift + 3 * len(want)].tobytes() == host.tobytes(), (s, shift)
                assert tuple(rows.shape) == (len(want), 24)
    finally:
        for dp in dps:
            dp.close()


def test_one_position_through_different_ranges_and_strides(A, ctx, five):
    recs, fulls, total = five
    for q in (1234, 17, 4096):
        ref, _ = ctx.across_moments_windows_host(recs, [q], [1], 1)
        assert ref.shape == (1,)
        _assert_same(ref, M.across_moments(fulls, [q], [1], 1)[0], q)
        for b, c, s in ((q - 14 if q >= 14 else q % 7, 100, 7), (q % 500, total - q % 500, 500), (q, total - q, 2),
                        (1, total - 1, q - 1), (q - 1, 2, 1), (q % 2, q + 2, 2), (q - 1, 3, 1), (q, 700, 1), (q - 513, 600, 1)):
            if b < 0:
                continue
            got, off = ctx.across_moments_windows_host(recs, [0, b, 2048], [3, c, 30], s)
            j = int(off[1]) + (q - b) // s
            assert (q - b) % s == 0 and j < int(off[2]) and got[j: j + 1].tobytes() == ref.tobytes(), (q, b, c, s)


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
    b, c = [0, 90001], [LONG, 30000]  # the second range begins odd and crosses the least budget's piece end at 131072
    want, _ = M.across_moments(fulls, b, c, 1)
    want7, _ = M.across_moments(fulls, b, c, 7)
    ref, _ = ctx.across_moments_windows_host(recs, b, c, 1)
    _assert_same(ref, want, "default")
    two, least = 8 * (4 * 100352 + 2 * 131072), 1
    assert _pieces(LONG, 8 * (2 ** 24 + 2 * 131072), 4, 1) == 1 and _pieces(LONG, two, 4, 1) == 2 and _pieces(LONG, least, 4, 1) == 4
    try:
        for budget in (two, least):
            ctx.set_aggregate_scratch(budget)
            got, _ = ctx.across_moments_windows_host(recs, b, c, 1)
            assert got.tobytes() == ref.tobytes(), budget
            got7, _ = ctx.across_moments_windows_host(recs, b, c, 7)
            _assert_same(got7, want7, (budget, 7))
    finally:
        ctx.set_aggregate_scratch(0)


def test_host_device_stream_and_image_calls_agree(A, ctx, torch):
    bros, fulls = [], []
    for k in range(3):
        x = H.synth_series(5140 + k, 20000 + 100 * k, block=7000)
        bros.append(A.compress_data(ctx, x, A.AUTO, 3))
        fulls.append(A.decompress_data(ctx, bros[-1]))
    p0 = [H.varint_decode(bro, 9)[1] for bro in bros]
    bodies = [torch.from_numpy(np.frombuffer(bro[p:], dtype=np.uint8).copy()).to("cuda") for bro, p in zip(bros, p0)]
    dps = [A.DPlan(ctx, bro[p:]) for bro, p in zip(bros, p0)]
    sts = [A.CompressedStream.from_bytes(ctx, bro) for bro in bros]
    try:
        for s in (1, 7):
            b, c = [10001, 5000, 19000], [7000, 6001, 100]  # begins far into the streams: the host call uploads a part
            want, woff = M.across_moments(fulls, b, c, s)
            via_bro, off = A.across_moments_data_windows(ctx, bros, b, c, s)
            _assert_same(via_bro, want, s)
            assert off.tolist() == woff.tolist()
            host, _ = ctx.across_moments_windows_host([bro[9:] for bro in bros], b, c, s, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), s
            plain, _ = ctx.across_moments_windows_host([bro[p:] for bro, p in zip(bros, p0)], b, c, s)
            assert plain.tobytes() == via_bro.tobytes(), s
            assert sts[0].across_moments_windows(sts[1:], b, c, s)[0].tobytes() == via_bro.tobytes(), s
            for shift in (0, 1):
                d = torch.full((shift + 3 * len(want) + 8,), SENT, dtype=torch.int64, device="cuda")
                rows, doff = dps[0].across_moments_windows(bodies[0], dps[1:], bodies[1:], b, c, d[shift:], s,
                                                           torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                h = d.cpu().numpy().view(np.uint64)
                assert doff.tolist() == woff.tolist() and np.all(h[:shift] == SENT) and np.all(h[shift + 3 * len(want):] == SENT)
                assert h[shift: shift + 3 * len(want)].tobytes() == via_bro.tobytes(), (s, shift)
                assert rows.cpu().numpy().view(A.ACROSS_MOMENTS).reshape(-1).tobytes() == via_bro.tobytes()
        # the same plan and the same stream twice in a list
        d = torch.full((3 * 100 + 8,), SENT, dtype=torch.int64, device="cuda")
        rows, _ = dps[0].across_moments_windows(bodies[0], [dps[1], dps[0]], [bodies[1], bodies[0]], [15000], [100], d,
                                                stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        twice = M.across_moments([fulls[0], fulls[1], fulls[0]], [15000], [100], 1)[0]
        _assert_same(rows.cpu().numpy().view(M.dtype).reshape(-1), twice, "twice")
        _assert_same(sts[0].across_moments_windows([sts[1], sts[0]], [15000], [100])[0], twice, "twice, streams")
    finally:
        for dp in dps:
            dp.close()


def test_merge_on_the_devices_records(A, ctx, many):
    recs, fulls = many
    b, c = [501, 2000], [900, 300]  # NaN holes inside
    x = M.columns(fulls, b, c, 2)
    assert np.isnan(x).any()
    whole, _ = ctx.across_moments_windows_host(recs[:12], b, c, 2)
    _assert_same(whole, M.records(x[:12]), "12")

    def merged(parts):
        out = np.zeros(len(parts[0]), dtype=M.dtype)
        for p in range(len(out)):
            out[p] = A.across_moments_merge(np.array([part[p] for part in parts]))
        return out

    singles = [ctx.across_moments_windows_host([r], b, c, 2)[0] for r in recs[:12]]
    _assert_same(merged(singles), whole, "singletons")  # the fold is Merge with leaves
    _assert_same(merged([ctx.across_moments_windows_host(recs[:5], b, c, 2)[0]] + singles[5:]), whole, "5 + singletons")
    # more than 64 streams: sub-lists of 64, 64 and 2, by the model's merge bit for bit
    parts = [ctx.across_moments_windows_host(r, b, c, 2)[0] for r in (recs, recs[::-1], recs[3:5])]
    got = merged(parts)
    _assert_same(got, M.merge_records(parts), "130 streams")
    assert np.all(got["count"] + got["nans"] == 130) and got["count"].max() == 130


def _ptrs(values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _raw_host(A, ctx, bufs, rg, s, n_streams=None, null_list=False, null_entry=None, n_out=16, misalign=False):
    out = np.full(3 * n_out + 1, SENT, dtype=np.uint64)
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    ptr = [x.ctypes.data for x in bufs]
    if null_entry is not None:
        ptr[null_entry] = None
    lens = np.array([len(x) for x in bufs], dtype=np.uint64)
    flags = np.zeros(max(len(bufs), 1), dtype=np.int32)
    rc = A.capi.lib().atsc_across_moments_windows(
        ctx._h, len(bufs) if n_streams is None else n_streams, None if null_list else _ptrs(ptr), lens.ctypes.data_as(p),
        flags.ctypes.data_as(C.POINTER(C.c_int32)), len(rg), b.ctypes.data_as(p), c.ctypes.data_as(p), s,
        C.c_void_p(out.ctypes.data + (4 if misalign else 0)))
    return rc, out


def _raw_dev(A, ctx, torch, dps, bodies, rg, s, n_streams=None, null_list=False, null_entry=None, misalign=False):
    d = torch.full((128,), SENT, dtype=torch.int64, device="cuda")
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    plans, ptr = [x._h.value for x in dps], [x.data_ptr() for x in bodies]
    if null_entry is not None:
        plans[null_entry] = None
    rc = A.capi.lib().atsc_across_moments_windows_dev(
        ctx._h, len(dps) if n_streams is None else n_streams, None if null_list else _ptrs(plans), _ptrs(ptr), len(rg),
        b.ctypes.data_as(p), c.ctypes.data_as(p), s, C.c_void_p(d.data_ptr() + (4 if misalign else 0)),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool((d == SENT).all())


def test_errors_leave_the_result_untouched(A, ctx, torch):
    rng = np.random.default_rng(7)
    Ec = A.capi
    lens = (9000, 9000, 6000)  # only stream 2 of 3 is too short for a range past 6000
    recs = [_comp(A, ctx, rng.normal(0, 1, n), H.frame_offsets(n, 1024), A.NOOP, False, 0.0) for n in lens]
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in recs]
    # every case of the across call
    cases = [dict(rg=[(0, 10)], s=1, n_streams=0), dict(rg=[(0, 10)], s=1, n_streams=65), dict(rg=[(0, 10)], s=1, null_list=True),
             dict(rg=[(0, 10)], s=1, null_entry=1), dict(rg=[(0, 10)], s=0), dict(rg=[(0, 2 ** 33)], s=1),
             dict(rg=[(0, 2 ** 32 - 1), (0, 5)], s=1), dict(rg=[(0, 7000)], s=1), dict(rg=[(0, 10), (5999, 2)], s=1),
             dict(rg=[(0, 10), (6001, 0)], s=1), dict(rg=[(2 ** 63, 2 ** 63)], s=1), dict(rg=[(2 ** 64 - 1, 2)], s=3)]
    # and the result pointer's
    cases += [dict(rg=[(0, 2)], s=1, misalign=True), dict(rg=[(0, 2)], s=2, misalign=True)]
    for kw in cases:
        rc, out = _raw_host(A, ctx, bufs, **kw)
        assert rc == Ec.E_INVALID and np.all(out == SENT), (kw, rc)
    ctx2 = A.Context(0)
    dps = [A.DPlan(ctx, r) for r in recs]
    bodies = [torch.from_numpy(x.copy()).to("cuda") for x in bufs]
    other = A.DPlan(ctx2, recs[0])
    try:
        for kw in cases:
            rc, untouched = _raw_dev(A, ctx, torch, dps, bodies, **kw)
            assert rc == Ec.E_INVALID and untouched, (kw, rc)
        rc, untouched = _raw_dev(A, ctx, torch, [dps[0], other, dps[1]], [bodies[0], bodies[0], bodies[1]], [(0, 10)], 1)
        assert rc == Ec.E_INVALID and untouched  # plans of different contexts
        sa, sb = A.CompressedStream.from_bytes(ctx, A.bro_prefix(9) + recs[0]), A.CompressedStream.from_bytes(ctx2, A.bro_prefix(9) + recs[0])
        with pytest.raises(A.AtscError) as ei:
            sa.across_moments_windows([sb], [0], [10])  # streams of different contexts
        assert ei.value.rc == Ec.E_INVALID
        with pytest.raises(A.AtscError) as ei:
            sa.across_moments_windows([sa], [0], [10], 0)  # stride 0
        assert ei.value.rc == Ec.E_INVALID
        del sa, sb
        # the two good streams alone hold the range; within all three, n_windows == 0 and empty ranges write nothing
        rc, untouched = _raw_dev(A, ctx, torch, dps[:2], bodies[:2], [(0, 7000)], 1000)
        assert rc == 0 and not untouched
        rc, untouched = _raw_dev(A, ctx, torch, dps, bodies, [], 1)
        assert rc == 0 and untouched
        rc, untouched = _raw_dev(A, ctx, torch, dps, bodies, [(5, 0), (6000, 0)], 1)
        assert rc == 0 and untouched
    finally:
        other.close()
        for dp in dps:
            dp.close()
        ctx2.close()
    rc, out = _raw_host(A, ctx, bufs[:2], [(0, 7000)], 1000)  # 7 records of 3 words
    assert rc == 0 and np.all(out[21:] == SENT) and not np.any(out[:21] == SENT)
    rc, out = _raw_host(A, ctx, bufs, [], 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufs, [(5, 0), (6000, 0)], 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufs, [(5999, 1)], 1)  # the shortest stream's last sample
    assert rc == 0 and np.all(out[3:] == SENT)
    x = np.array([ctx.decompress_window_host(r, 5999, 1)[0] for r in recs])
    _assert_same(out[:3].view(M.dtype), M.records(x[:, None]), "last sample")


def test_malformed_payload_in_one_stream_of_three(A, ctx, torch):
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
        got, _ = ctx.across_moments_windows_host(lst, b, c, s)
        _assert_same(got, M.across_moments(good, b, c, s)[0], ("outside", s))
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in lst]
    for rg in ([(3 * n, 20)], [(0, nf * n)], [(0, 40), (3 * n - 19, 20)], [(4 * n - 20, 20), (6 * n, 50)]):
        for s in (1, 300):
            rc, out = _raw_host(A, ctx, bufs, rg, s, n_out=nf * n)
            assert rc == A.capi.E_FORMAT and np.all(out == SENT), (rg, s, rc)
    # The device call sets the status word of the plan whose stream holds the frame.  The word has no accessor in the C
    # ABI or the Python surface (see tests/test_gpu_histogram.py): the host call above, which is the device call on plans
    # of the touched records followed by a read of every plan's word, is what shows it, and the same ranges over the two
    # good streams alone give no error.  The device call itself returns ATSC_OK, finishes, writes every record, and gives
    # the ranges beside the bad frame their right records.
    rc, out = _raw_host(A, ctx, [bufs[0], bufs[2]], [(3 * n, 20)], 1, n_out=nf * n)
    assert rc == 0
    dps = [A.DPlan(ctx, r) for r in lst]
    bodies = [torch.from_numpy(x.copy()).to("cuda") for x in bufs]
    try:
        rg = [(0, 3 * n), (3 * n + 7, 20), (4 * n, 100)]
        want, off = M.across_moments(good, [w[0] for w in rg], [w[1] for w in rg], 1)
        d = torch.full((3 * len(want),), SENT, dtype=torch.int64, device="cuda")
        rows, _ = dps[0].across_moments_windows(bodies[0], dps[1:], bodies[1:], [w[0] for w in rg], [w[1] for w in rg], d, 1,
                                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = rows.cpu().numpy().view(M.dtype).reshape(-1)
        assert not (d.cpu().numpy().view(np.uint64) == SENT).any()
        clean = np.r_[0: int(off[1]), int(off[2]): int(off[3])]
        _assert_same(got[clean], want[clean], "dev, beside the bad frame")
    finally:
        for dp in dps:
            dp.close()


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
    header = "offset,count,min,min_at,max,max_at,sum,mean"
    new = ["nonnan", "avg", "stdvar", "stddev"]
    for n, (b0, c0), s, more in ((2, (0, total), None, []), (3, (7, 1000), 15, ["--across-quantiles", "0.5,0.9", "--across-extremes", 2]),
                                 (3, (total - 1, 1), 4, [])):
        listed = ",".join(str(p) for p in paths[1:n])
        front = (["--across-stride", s] if s else []) + more
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--across", listed, *front, "--across-moments", paths[0])
        with_flag = (tmp_path / "uptime.across.csv").read_bytes()
        lines = with_flag.decode().split("\n")
        nf = len(lines[0].split(",")) - 4  # the columns in front
        assert lines[0].split(",")[nf:] == new and nf == 8 + (2 + 1 + 4 * 2 if more else 0)
        rows = [l.split(",") for l in lines[1:] if l]
        s = s or 1
        want, _ = A.across_moments_data_windows(ctx, bros[:n], [b0], [c0], s)
        fit = A.across_moments_fit(want)
        assert len(rows) == len(want) == AM.outputs(c0, s) > 0 and all(len(r) == nf + 4 for r in rows)
        for r, w, f in zip(rows, want, fit):
            cells = r[nf:]
            if w["count"] == 0:
                assert cells == ["", "", "", ""]
                continue
            assert int(cells[0]) == w["count"] == int(r[1])
            got = np.array([float(v) for v in cells[1:]])
            assert got.tobytes() == np.array([f["mean"], f["variance"], f["stddev"]]).tobytes(), (r, w, f)
        # without the option the file is what it was: the columns in front, byte for byte
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--across", listed, *front, paths[0])
        plain = (tmp_path / "uptime.across.csv").read_bytes()
        assert plain.decode().split("\n")[0].startswith(header) and (plain.decode().split("\n")[0] == header) == (not more)
        assert plain == "\n".join(",".join(l.split(",")[:nf]) if l else l for l in lines).encode()
