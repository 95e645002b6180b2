"""Windowed across histograms on the GPU: every row of every case against the NumPy model of the contract
(tests/across_histogram_model.py) applied to the GPU's own full decodes -- integers, compared exactly, no position left
out.  The streams are the across moments' (tests/test_gpu_across_moments.py): five short streams (NaN runs, +-Inf, zeros
of both signs, a constant series, one series twice, three framings) for N = 1, 2, 3, 5; 64 plans over eight Noop series
with NaN holes for N = 8 .. 64.  Edge lists hold +-Inf and values equal to samples; n_edges around a wavefront's 64
counters and at every n_edges where the rows a wavefront counts at a time change; ranges, strides and result
alignments at which the kernel or the host takes another path; N = 1 against the listed one-sample windows, N = 5
against the sum of them, the NaN counter against the across' count, one position through different ranges and strides,
a permuted list; budgets that cut a range into pieces, also shared 64 ways; the host, device, stream and image calls;
every error of the contract with the result untouched; a malformed payload in one stream of three; the atsc command
line."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import across_histogram_model as M
from tests import across_model as AM
from tests import helpers as H

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A5A5A5A5A
NAN = float("nan")
LEFT, RIGHT = M.LEFT_CLOSED, M.RIGHT_CLOSED
# the first 24 samples of each of the five streams, as Constant records: every stream NaN at 0 .. 7; zeros of both signs
# at 8 .. 15; +Inf with -Inf at 16 .. 19 (streams 0 and 1 are one series: stream 2 brings the -Inf)
ZONES = [[(NAN, 8), (-0.0, 4), (0.0, 4), (np.inf, 4), (1.0, 4)],
         [(NAN, 8), (NAN, 4), (0.0, 2), (-0.0, 2), (-np.inf, 4), (1.0, 4)],
         [(NAN, 8), (-0.0, 8), (NAN, 4), (0.5, 4)],
         [(NAN, 8), (NAN, 8), (np.inf, 4), (1.0, 4)]]
LONG = 200000
TASK = 512  # positions per task of the position kernel (ACR_TASK)
WIDE = [62, 63, 64, 255, 256, 1024]  # row lengths around a wavefront's 64 counters; the largest


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
    # 0 and 1: one series, 256-sample frames under auto at 5 %
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


def _edges(fulls, n_edges, seed=0):
    """n_edges ascending edges that are samples of the streams (0.0 among them where a stream holds a zero), with -Inf
    and +Inf at the ends from three edges on"""
    v = np.unique(np.concatenate([f[np.isfinite(f)] for f in fulls]))
    v = v[v != 0.0]
    rng = np.random.default_rng(1000 * n_edges + seed)
    ends = n_edges >= 3
    k = n_edges - (2 if ends else 0) - (1 if n_edges >= 2 else 0)
    assert len(v) >= k
    inner = list(rng.choice(v, size=k, replace=False)) + ([0.0] if n_edges >= 2 else [])
    e = np.array(([-np.inf] if ends else []) + sorted(inner) + ([np.inf] if ends else []))
    assert len(e) == n_edges and np.all(e[1:] > e[:-1])
    return e


def _assert_same(got, want, label):
    assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape, (label, got.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere((got != want).any(axis=1))[:, 0]
        assert False, (label, len(bad), int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


def _ranges(total):
    """ranges that begin odd and even, overlap, come unsorted, are empty, have count == 1, end at the shortest stream's last
    sample and (last) span the whole of it"""
    return [(2048, 1500), (1, 2051), (2500, 1000), (777, 0), (3001, 1), (2047, 2050), (total - 1235, 1235), (total, 0),
            (0, 40), (9, 10), (0, total)]


def test_the_edges_meet_the_samples(five, many):
    recs, fulls, total = five
    x = np.array([f[:total] for f in fulls])
    for n_edges in (2, 13, 64, 1024):
        e = _edges(fulls, n_edges)
        assert np.isin(x, e[np.isfinite(e)]).sum() > 100 and 0.0 in e  # samples on the edges; -0.0 and 0.0 against 0.0
        assert (n_edges < 3) or (np.isneginf(e[0]) and np.isposinf(e[-1]))
    assert np.isinf(x).any() and np.isnan(x).any() and np.isnan(x[:, :8]).all()
    assert (x[:, 8:16] == 0.0).any() and np.signbit(x[:, 8:16]).any()
    e = _edges(many[1], 13)
    assert np.isin(np.array(many[1]), e[np.isfinite(e)]).sum() > 50


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_every_row_matches_the_model(A, ctx, five, n):
    recs, fulls, total = five
    rg = _ranges(total)
    b, c = [x[0] for x in rg], [x[1] for x in rg]
    for n_edges in (1, 2, 13):
        edges = _edges(fulls, n_edges, n)
        for closed in (LEFT, RIGHT):
            for s in (1, 2, 7, 5000):
                got, off = ctx.across_histogram_windows_host(recs[:n], b, c, edges, s, closed)
                want, woff = M.across_histogram(fulls[:n], b, c, edges, s, closed)
                assert off.tolist() == woff.tolist() == A.across_offsets(c, s).tolist()
                assert off[3] == off[4] and off[5] - off[4] == 1 and off[7] == off[8]  # empty: none; count == 1: one
                _assert_same(got, want, (n, n_edges, closed, s))
                assert np.all(got.sum(axis=1) == n)
    # the zone where every stream is NaN
    z, _ = ctx.across_histogram_windows_host(recs[:n], [0], [24], [0.0, 1.0])
    assert z[:8].tolist() == [[0, 0, 0, n]] * 8


@pytest.mark.parametrize("n_edges", WIDE + M.pass_boundaries()[:2] + M.pass_boundaries()[-2:])
def test_wide_rows_three_streams(A, ctx, five, n_edges):
    recs, fulls, total = five
    b, c = [1, 2048, 0], [700, 131, 24]
    edges = _edges(fulls, n_edges)
    for closed, s in ((LEFT, 1), (RIGHT, 1), (LEFT, 3)):
        got, _ = ctx.across_histogram_windows_host(recs[2:5], b, c, edges, s, closed)
        _assert_same(got, M.across_histogram(fulls[2:5], b, c, edges, s, closed)[0], (n_edges, closed, s))


def test_every_n_edges_at_which_the_rows_of_a_pass_change(A, ctx, five):
    recs, fulls, total = five
    bounds = M.pass_boundaries()
    assert bounds[:2] == [218, 219] and len(bounds) > 40 and {M.rows_a_pass(e) for e in bounds} >= {64, 62, 32, 16, 13}
    for i, n_edges in enumerate(bounds):
        edges = _edges(fulls, n_edges)
        got, _ = ctx.across_histogram_windows_host(recs[2:5], [1001], [200], edges, 1, i % 2)
        _assert_same(got, M.across_histogram(fulls[2:5], [1001], [200], edges, 1, i % 2)[0], n_edges)


@pytest.mark.parametrize("n", [8, 9, 17, 33, 63, 64])
def test_many_streams(A, ctx, many, n):
    recs, fulls = many
    recs, fulls = recs[:n], fulls[:n]
    b, c = [0, 1, 2001], [3000, 1500, 999]
    for n_edges in (1, 2, 13):
        edges = _edges(fulls, n_edges, n)
        for closed, s in ((LEFT, 1), (RIGHT, 1), (RIGHT, 3)):
            got, off = ctx.across_histogram_windows_host(recs, b, c, edges, s, closed)
            want, woff = M.across_histogram(fulls, b, c, edges, s, closed)
            assert off.tolist() == woff.tolist()
            _assert_same(got, want, (n, n_edges, closed, s))
            # the NaN counter against the across' own count
            acr, aoff = ctx.across_windows_host(recs, b, c, s)
            assert aoff.tolist() == off.tolist() and np.array_equal(got[:, -1], n - acr["count"].astype(np.uint64))
            assert (got[:, -1] > 0).any() and (got[:, -1] == 0).any() and np.all(got.sum(axis=1) == n)


@pytest.mark.parametrize("n_edges", WIDE + M.pass_boundaries()[:2] + M.pass_boundaries()[-2:])
def test_wide_rows_sixty_four_streams(A, ctx, many, n_edges):
    recs, fulls = many
    b, c = [1100, 2], [300, 77]  # a NaN hole inside
    edges = _edges(fulls, n_edges)
    for closed, s in ((LEFT, 1), (RIGHT, 2)):
        got, _ = ctx.across_histogram_windows_host(recs, b, c, edges, s, closed)
        _assert_same(got, M.across_histogram(fulls, b, c, edges, s, closed)[0], (n_edges, closed, s))
        assert np.all(got.sum(axis=1) == 64)


def _dev_rows(A, torch, dps, bodies, b, c, edges, s, closed, shift):
    """the device call into a sentinel-filled buffer that begins 8 * shift bytes behind a multiple of 16, with guard words
    behind the last row -> the rows as a NumPy array"""
    m, rows = int(AM.offsets(c, s)[-1]), len(edges) + 2
    d = torch.full((shift + m * rows + 8,), SENT, dtype=torch.int64, device="cuda")
    assert (d.data_ptr() + 8 * shift) % 16 == 8 * shift
    view, off = dps[0].across_histogram_windows(bodies[0], dps[1:], bodies[1:], b, c, edges, d[shift:], s, closed,
                                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = d.cpu().numpy().view(np.uint64)
    assert np.all(h[:shift] == SENT) and np.all(h[shift + m * rows:] == SENT)  # the guards
    assert not np.any(h[shift: shift + m * rows] == SENT)  # every counter is overwritten
    assert tuple(view.shape) == (m, rows) and off.tolist() == AM.offsets(c, s).tolist()
    return h[shift: shift + m * rows].reshape(m, rows).copy()


def test_shapes_where_the_kernel_takes_another_path(A, ctx, torch, five):
    """ranges with an odd and an even first sample of every length around a wavefront, a task and two tasks; strides on
    both sides of a wavefront and beyond a range; results at a multiple of 16 bytes and 8 bytes off one, with an odd row
    length (successive rows alternate in 16-byte alignment) and an even one"""
    recs, fulls, total = five
    lengths = [0, 1, 63, 64, 65, TASK - 1, TASK, TASK + 1, 2 * TASK + 1]
    rg = [(b0, n) for b0 in (1001, 1000) for n in lengths]
    rg += [(1000, 65), (1010, 3), (total - TASK - 1, TASK + 1), (total, 0), (2047, 2), (1, 700)]  # overlapping, unordered, empty
    b, c = [x[0] for x in rg], [x[1] for x in rg]
    bodies = [torch.from_numpy(np.frombuffer(r, dtype=np.uint8).copy()).to("cuda") for r in recs]
    dps = [A.DPlan(ctx, r) for r in recs]
    try:
        for n_edges, closed in ((13, LEFT), (2, RIGHT)):
            edges = _edges(fulls, n_edges)
            for s in (1, 2, 3, 7, 64, 2 * TASK + 7):
                want, woff = M.across_histogram(fulls, b, c, edges, s, closed)
                host, off = ctx.across_histogram_windows_host(recs, b, c, edges, s, closed)
                assert off.tolist() == woff.tolist()
                _assert_same(host, want, ("host", n_edges, s))
                for shift in (0, 1):
                    got = _dev_rows(A, torch, dps, bodies, b, c, edges, s, closed, shift)
                    assert got.tobytes() == host.tobytes(), (n_edges, s, shift)
    finally:
        for dp in dps:
            dp.close()


def test_against_the_listed_one_sample_windows(A, ctx, five):
    recs, fulls, total = five
    b, c, s = [3, 2000], [900, 301], 3
    pos = np.concatenate([b0 + s * np.arange(AM.outputs(c0, s)) for b0, c0 in zip(b, c)])
    for n_edges, closed in ((1, RIGHT), (13, LEFT), (64, RIGHT)):
        edges = _edges(fulls, n_edges)
        singles = [ctx.histogram_windows_host(r, pos, np.ones(len(pos), dtype=np.uint64), edges, closed) for r in recs]
        for j in (2, 4):  # N = 1: byte for byte the listed windows' rows
            one, _ = ctx.across_histogram_windows_host([recs[j]], b, c, edges, s, closed)
            assert one.dtype == singles[j].dtype and one.tobytes() == singles[j].tobytes(), (n_edges, j)
        allfive, _ = ctx.across_histogram_windows_host(recs, b, c, edges, s, closed)  # N = 5: the sum of them
        assert allfive.tobytes() == sum(singles).astype(np.uint64).tobytes(), n_edges
        # rows of sub-lists add to the whole list's; a permuted list gives the same bytes
        front, _ = ctx.across_histogram_windows_host(recs[:2], b, c, edges, s, closed)
        back, _ = ctx.across_histogram_windows_host(recs[2:], b, c, edges, s, closed)
        assert (front + back).tobytes() == allfive.tobytes()
        perm, _ = ctx.across_histogram_windows_host([recs[k] for k in (3, 0, 4, 2, 1)], b, c, edges, s, closed)
        assert perm.tobytes() == allfive.tobytes()
        acr, _ = ctx.across_windows_host(recs, b, c, s)
        assert np.array_equal(allfive[:, -1], 5 - acr["count"].astype(np.uint64))


def test_one_position_through_different_ranges_and_strides(A, ctx, five):
    recs, fulls, total = five
    edges = _edges(fulls, 13)
    for q in (1234, 17, 4096):
        ref, _ = ctx.across_histogram_windows_host(recs, [q], [1], edges)
        assert ref.shape == (1, 15)
        _assert_same(ref, M.across_histogram(fulls, [q], [1], edges)[0], q)
        for b, c, s in ((q - 14 if q >= 14 else q % 7, 100, 7), (q % 500, total - q % 500, 500), (q, total - q, 2),
                        (1, total - 1, q - 1), (q - 1, 2, 1), (q % 2, q + 2, 2), (q - 1, 3, 1), (q, 700, 1), (q - 513, 600, 1)):
            if b < 0:
                continue
            got, off = ctx.across_histogram_windows_host(recs, [0, b, 2048], [3, c, 30], edges, s)
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
    edges = _edges(fulls, 13)
    b, c = [0, 90001], [LONG, 30000]  # the second range begins odd and crosses the least budget's piece end at 131072
    far = 70001  # a stride longer than a piece of the least budget
    want, _ = M.across_histogram(fulls, b, c, edges, 1, RIGHT)
    want7, _ = M.across_histogram(fulls, b, c, edges, 7, RIGHT)
    wantfar, _ = M.across_histogram(fulls, b, c, edges, far, RIGHT)
    ref, _ = ctx.across_histogram_windows_host(recs, b, c, edges, 1, RIGHT)
    _assert_same(ref, want, "default")
    # 64 plans share the budget: every stream sixteen times, ranges across the least budget's piece ends
    many_recs, many_fulls = [recs[j % 4] for j in range(64)], [fulls[j % 4] for j in range(64)]
    b64, c64 = [60001, 130000, 5], [12000, 2100, 0]
    want64, _ = M.across_histogram(many_fulls, b64, c64, edges, 1, LEFT)
    ref64, _ = ctx.across_histogram_windows_host(many_recs, b64, c64, edges, 1, LEFT)
    _assert_same(ref64, want64, "64, default")
    two, least = 8 * (4 * 100352 + 2 * 131072), 1
    assert _pieces(LONG, 8 * (2 ** 24 + 2 * 131072), 4, 1) == 1 and _pieces(LONG, two, 4, 1) == 2 and _pieces(LONG, least, 4, 1) == 4
    assert _pieces(LONG, least, 64, 16) == 4 and far > 65536
    try:
        for budget in (two, least):
            ctx.set_aggregate_scratch(budget)
            got, _ = ctx.across_histogram_windows_host(recs, b, c, edges, 1, RIGHT)
            assert got.tobytes() == ref.tobytes(), budget
            _assert_same(ctx.across_histogram_windows_host(recs, b, c, edges, 7, RIGHT)[0], want7, (budget, 7))
            _assert_same(ctx.across_histogram_windows_host(recs, b, c, edges, far, RIGHT)[0], wantfar, (budget, far))
            got64, _ = ctx.across_histogram_windows_host(many_recs, b64, c64, edges, 1, LEFT)
            assert got64.tobytes() == ref64.tobytes(), budget
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
    edges = _edges(fulls, 13)
    try:
        for s, closed in ((1, LEFT), (7, RIGHT)):
            b, c = [10001, 5000, 19000], [7000, 6001, 100]  # begins far into the streams: the host call uploads a part
            want, woff = M.across_histogram(fulls, b, c, edges, s, closed)
            via_bro, off = A.across_histogram_data_windows(ctx, bros, b, c, edges, s, closed)
            _assert_same(via_bro, want, s)
            assert off.tolist() == woff.tolist()
            host, _ = ctx.across_histogram_windows_host([bro[9:] for bro in bros], b, c, edges, s, closed, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), s
            plain, _ = ctx.across_histogram_windows_host([bro[p:] for bro, p in zip(bros, p0)], b, c, edges, s, closed)
            assert plain.tobytes() == via_bro.tobytes(), s
            assert sts[0].across_histogram_windows(sts[1:], b, c, edges, s, closed)[0].tobytes() == via_bro.tobytes(), s
            for shift in (0, 1):
                assert _dev_rows(A, torch, dps, bodies, b, c, edges, s, closed, shift).tobytes() == via_bro.tobytes(), (s, shift)
        # the same plan and the same stream twice in a list
        twice = M.across_histogram([fulls[0], fulls[1], fulls[0]], [15000], [100], edges)[0]
        got = _dev_rows(A, torch, [dps[0], dps[1], dps[0]], [bodies[0], bodies[1], bodies[0]], [15000], [100], edges, 1, LEFT, 0)
        _assert_same(got, twice, "twice")
        _assert_same(sts[0].across_histogram_windows([sts[1], sts[0]], [15000], [100], edges)[0], twice, "twice, streams")
    finally:
        for dp in dps:
            dp.close()


def _ptrs(values):
    return (C.c_void_p * max(len(values), 1))(*values)


GOOD_EDGES = (-1.0, 0.0, 2.5)


def _edge_args(edges, n_edges, null_edges):
    e = np.array(edges, dtype=np.float64)
    return e, len(e) if n_edges is None else n_edges, None if null_edges else e.ctypes.data_as(C.POINTER(C.c_double))


def _raw_host(A, ctx, bufs, rg, s, n_streams=None, null_list=False, null_entry=None, n_out=16, misalign=False,
              edges=GOOD_EDGES, n_edges=None, null_edges=False, closed=LEFT):
    out = np.full(5 * n_out + 1, SENT, dtype=np.uint64)
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    ptr = [x.ctypes.data for x in bufs]
    if null_entry is not None:
        ptr[null_entry] = None
    lens = np.array([len(x) for x in bufs], dtype=np.uint64)
    flags = np.zeros(max(len(bufs), 1), dtype=np.int32)
    e, ne, pe = _edge_args(edges, n_edges, null_edges)
    rc = A.capi.lib().atsc_across_histogram_windows(
        ctx._h, len(bufs) if n_streams is None else n_streams, None if null_list else _ptrs(ptr), lens.ctypes.data_as(p),
        flags.ctypes.data_as(C.POINTER(C.c_int32)), len(rg), b.ctypes.data_as(p), c.ctypes.data_as(p), s, ne, pe, closed,
        C.c_void_p(out.ctypes.data + (4 if misalign else 0)))
    return rc, out


def _raw_dev(A, ctx, torch, dps, bodies, rg, s, n_streams=None, null_list=False, null_entry=None, misalign=False,
             edges=GOOD_EDGES, n_edges=None, null_edges=False, closed=LEFT, n_out=None):
    d = torch.full((128,), SENT, dtype=torch.int64, device="cuda")
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    plans, ptr = [x._h.value for x in dps], [x.data_ptr() for x in bodies]
    if null_entry is not None:
        plans[null_entry] = None
    e, ne, pe = _edge_args(edges, n_edges, null_edges)
    rc = A.capi.lib().atsc_across_histogram_windows_dev(
        ctx._h, len(dps) if n_streams is None else n_streams, None if null_list else _ptrs(plans), _ptrs(ptr), len(rg),
        b.ctypes.data_as(p), c.ctypes.data_as(p), s, ne, pe, closed, C.c_void_p(d.data_ptr() + (4 if misalign else 0)),
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
    # every case of the histograms' edge checks
    cases += [dict(rg=[(0, 10)], s=1, n_edges=0), dict(rg=[(0, 10)], s=1, edges=np.arange(1025.0), n_edges=1025),
              dict(rg=[(0, 10)], s=1, null_edges=True), dict(rg=[(0, 10)], s=1, edges=(0.0, NAN, 1.0)),
              dict(rg=[(0, 10)], s=1, edges=(NAN,)), dict(rg=[(0, 10)], s=1, edges=(0.0, -0.0)),
              dict(rg=[(0, 10)], s=1, edges=(1.0, 1.0)), dict(rg=[(0, 10)], s=1, edges=(2.0, 1.0)),
              dict(rg=[(0, 10)], s=1, closed=2), dict(rg=[(0, 10)], s=1, closed=-1)]
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
            sa.across_histogram_windows([sb], [0], [10], [0.0])  # streams of different contexts
        assert ei.value.rc == Ec.E_INVALID
        with pytest.raises(A.AtscError) as ei:
            sa.across_histogram_windows([sa], [0], [10], [0.0], 0)  # stride 0
        assert ei.value.rc == Ec.E_INVALID
        with pytest.raises(A.AtscError) as ei:
            sa.across_histogram_windows([sa], [0], [10], [0.0, -0.0])  # equal edges
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
    rc, out = _raw_host(A, ctx, bufs[:2], [(0, 7000)], 1000)  # 7 rows of 5 counters
    assert rc == 0 and np.all(out[35:] == SENT) and not np.any(out[:35] == SENT) and np.all(out[:35].reshape(7, 5).sum(axis=1) == 2)
    rc, out = _raw_host(A, ctx, bufs, [], 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufs, [(5, 0), (6000, 0)], 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufs, [(5999, 1)], 1)  # the shortest stream's last sample
    assert rc == 0 and np.all(out[5:] == SENT)
    x = np.array([ctx.decompress_window_host(r, 5999, 1)[0] for r in recs])
    _assert_same(out[:5].reshape(1, 5), M.rows(x[:, None], GOOD_EDGES), "last sample")


def test_the_counter_index_limit(A, ctx, torch):
    """positions x (n_edges + 2) must be below 2^32 - 1: a constant stream of 86 records of 100000 samples and 1024 edges,
    so that the check is reached with nothing large allocated; 4186127 positions are the last that pass it (not run:
    34 GB of rows), 4186128 the first that do not"""
    over = 4186128
    assert (over - 1) * 1026 < 2 ** 32 - 1 <= over * 1026
    recs = _const_record(A, ctx, 1.5, 100000) * 86
    buf = np.frombuffer(recs, dtype=np.uint8)
    edges = np.arange(1024.0)
    for rg, s in (([(0, over)], 1), ([(0, over - 1), (7, 1)], 1), ([(1, 2 * over - 1)], 2), ([(0, 4300000)], 1)):
        rc, out = _raw_host(A, ctx, [buf, buf], rg, s, edges=edges)
        assert rc == A.capi.E_INVALID and np.all(out == SENT), (rg, s, rc)
        msg = A.capi.lib().atsc_ctx_last_error(ctx._h).decode()
        assert msg == "across_histogram_windows: positions x (n_edges + 2) is not below 2^32 - 1 counters", msg
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(buf.copy()).to("cuda")
    try:
        rc, untouched = _raw_dev(A, ctx, torch, [dp, dp], [body, body], [(0, over)], 1, edges=edges)
        assert rc == A.capi.E_INVALID and untouched
        # the same range passes with fewer edges per row, at a stride that keeps the result small
        rc, untouched = _raw_dev(A, ctx, torch, [dp, dp], [body, body], [(0, over)], 1000000, edges=edges[:10])
        assert rc == 0 and not untouched
    finally:
        dp.close()


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
    edges = _edges(good, 3)
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 20, 20), (5 * n + 3, 100), (3 * n + 5, 0)]
    b, c = [w[0] for w in outside], [w[1] for w in outside]
    for s in (1, 3):
        got, _ = ctx.across_histogram_windows_host(lst, b, c, edges, s)
        _assert_same(got, M.across_histogram(good, b, c, edges, s)[0], ("outside", s))
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in lst]
    for rg in ([(3 * n, 20)], [(0, nf * n)], [(0, 40), (3 * n - 19, 20)], [(4 * n - 20, 20), (6 * n, 50)]):
        for s in (1, 300):
            rc, out = _raw_host(A, ctx, bufs, rg, s, n_out=nf * n, edges=edges)
            assert rc == A.capi.E_FORMAT and np.all(out == SENT), (rg, s, rc)
    # The device call sets the status word of the plan whose stream holds the frame.  The word has no accessor in the C
    # ABI or the Python surface (see tests/test_gpu_histogram.py): the host call above, which is the device call on plans
    # of the touched records followed by a read of every plan's word, is what shows it, and the same ranges over the two
    # good streams alone give no error.  The device call itself returns ATSC_OK, finishes, writes every row, and gives
    # the ranges beside the bad frame their right rows.
    rc, out = _raw_host(A, ctx, [bufs[0], bufs[2]], [(3 * n, 20)], 1, n_out=nf * n, edges=edges)
    assert rc == 0
    dps = [A.DPlan(ctx, r) for r in lst]
    bodies = [torch.from_numpy(x.copy()).to("cuda") for x in bufs]
    try:
        rg = [(0, 3 * n), (3 * n + 7, 20), (4 * n, 100)]
        want, off = M.across_histogram(good, [w[0] for w in rg], [w[1] for w in rg], edges)
        got = _dev_rows(A, torch, dps, bodies, [w[0] for w in rg], [w[1] for w in rg], edges, 1, LEFT, 0)
        clean = np.r_[0: int(off[1]), int(off[2]): int(off[3])]
        _assert_same(got[clean], want[clean], "dev, beside the bad frame")
        assert np.all(got.sum(axis=1) == 3)
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
    fulls = [A.decompress_data(ctx, b) for b in bros]
    total = min(len(f) for f in fulls)
    assert total > 1000
    paths = [tmp_path / (name + ".bro") for name in names]
    header = "offset,count,min,min_at,max,max_at,sum,mean"
    lo, hi = float(np.floor(min(np.nanmin(f) for f in fulls))), float(np.ceil(max(np.nanmax(f) for f in fulls))) + 1.0
    mid = float(np.nanmedian(fulls[0]))
    specs = (("%r" % mid, [mid]), ("%r:%r:8" % (lo, hi), A.histogram_edges_uniform(lo, hi, 8)), ("-inf,%r,inf" % mid, [-np.inf, mid, np.inf]))
    for (n, (b0, c0), s, more), (spec, edges), side in zip(
            ((2, (0, total), None, []), (3, (7, 1000), 15, ["--across-quantiles", "0.5,0.9", "--across-moments"]),
             (3, (total - 1, 1), 4, [])), specs, (None, "right", "left")):
        listed = ",".join(str(p) for p in paths[1:n])
        front = (["--across-stride", s] if s else []) + more
        closed = ["--histogram-closed", side] if side else []
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--across", listed, *front, "--across-histogram", spec, *closed, paths[0])
        lines = (tmp_path / "uptime.across.csv").read_text().split("\n")
        new = ["h%d" % k for k in range(len(edges) + 1)] + ["hnan"]
        nf = len(lines[0].split(",")) - len(new)  # the columns in front
        assert lines[0].split(",")[nf:] == new and nf == 8 + (2 + 4 if more else 0)
        rows = [l.split(",") for l in lines[1:] if l]
        s = s or 1
        want, _ = A.across_histogram_data_windows(ctx, bros[:n], [b0], [c0], edges, s, RIGHT if side == "right" else LEFT)
        assert len(rows) == len(want) == AM.outputs(c0, s) > 0 and all(len(r) == nf + len(new) for r in rows)
        got = np.array([[int(v) for v in r[nf:]] for r in rows], dtype=np.uint64)
        _assert_same(got, want, spec)
        assert np.all(got.sum(axis=1) == n) and np.array_equal(got[:, -1], n - np.array([int(r[1]) for r in rows], dtype=np.uint64))
        # without the option the file is what it was: the columns in front, byte for byte
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--across", listed, *front, paths[0])
        plain = (tmp_path / "uptime.across.csv").read_text()
        assert plain.split("\n")[0].startswith(header) and (plain.split("\n")[0] == header) == (not more)
        assert plain == "\n".join(",".join(l.split(",")[:nf]) if l else l for l in lines)
