"""Windowed across value counts on the GPU: every record of every case against the NumPy model of the contract
(tests/across_values_model.py) applied to the GPU's own full decodes -- value bits and integers, compared exactly, no
position left out.  The streams are built as the across histograms' (tests/test_gpu_across_histogram.py): five short
streams (NaN runs, +-Inf, zeros of both signs, a constant series, one series twice, three framings) for N = 1, 2, 3, 5; 64
plans over eight Noop series of few distinct values with NaN holes for N = 4 .. 64; 64 different short series for
columns of more than 32 distinct values.  N at every power of two and one past it; k 1, 2, 3, 31, 32; `above` NaN, a
sample's value, either zero, +-Inf; ranges, strides and result alignments at which the kernel or the host takes another
path; N = 1 against the listed one-sample windows, N = 5 against atsc_values_merge of them, the across' count and min, the
across histograms' bins, reversed and permuted lists, sub-lists of 32 merged to 64, paging; budgets that cut a range into
pieces, also shared 64 ways; the host, device, stream and image calls; every error of the contract with the result
untouched; a malformed payload in one stream of three; the atsc command line."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import across_model as AM
from tests import across_values_model as M
from tests import helpers as H

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A5A5A5A5A
NAN, INF = float("nan"), float("inf")
# the first 24 samples of each of the five streams, as Constant records: every stream NaN at 0 .. 7; zeros of both signs
# at 8 .. 15; +Inf with -Inf at 16 .. 19 (streams 0 and 1 are one series: stream 2 brings the -Inf)
ZONES = [[(NAN, 8), (-0.0, 4), (0.0, 4), (INF, 4), (1.0, 4)],
         [(NAN, 8), (NAN, 4), (0.0, 2), (-0.0, 2), (-INF, 4), (1.0, 4)],
         [(NAN, 8), (-0.0, 8), (NAN, 4), (0.5, 4)],
         [(NAN, 8), (NAN, 8), (INF, 4), (1.0, 4)]]
LONG = 200000
TASK = 512  # positions per task of the position kernel (ACR_TASK)
KS = [1, 2, 3, 31, 32]


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
    # 2: a few levels around 1e9 in 256-sample frames, kept exactly (RLE)
    recs.append(zone[1] + _comp(A, ctx, 1e9 + rng.integers(0, 3, 5200) * 1e-3, H.frame_offsets(5200, 256), A.RLE, False, 0.0))
    # 3: a constant series in 4096-sample frames
    recs.append(zone[2] + _comp(A, ctx, np.full(5300, 1234.5678), H.frame_offsets(5300, 4096), A.CONSTANT, False, 0.0))
    # 4: hand-built Constant records of any length: NaN runs, +-Inf, zeros of both signs, stream 3's constant
    values = [1.0, NAN, -0.0, 2.5, INF, -7.0, -INF, 0.0, 1234.5678, NAN, -0.0, 0.0]
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
    """-> (records of 64 streams, their full decodes): eight Noop series of 3000 samples, the rounded values of slow waves
    (few distinct values: columns repeat), with Constant-NaN holes, in five framings, each listed eight times"""
    rng = np.random.default_rng(64)
    n = 3000
    recs, fulls = [], []
    # (Noop stores rounded integers, a NaN among them as 0: the holes are Constant records of NaN between the Noop frames)
    holes = {m: _const_record(A, ctx, NAN, m) for m in (1, 5, 37)}
    t = np.arange(n)
    for k in range(8):
        x = np.rint(2.5 * np.sin(t / (150.0 + 40 * k) + k) + 0.3 * rng.normal(0, 1, n)) + 0.0
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


@pytest.fixture(scope="module")
def wide(A, ctx):
    """-> (records of 64 different Noop series of 700 samples, their full decodes): stream j holds j - 32, from sample
    200 on plus a slow rounded wave: a column holds 64 distinct values in front, both signs and zero among them, and
    behind that fewer, some of them twice"""
    n = 700
    t = np.arange(n)
    recs, fulls = [], []
    for j in range(64):
        x = (j - 32.0) + np.where(t >= 200, np.rint(3.0 * np.sin(t / 90.0 + 0.37 * j)), 0.0) + 0.0
        recs.append(_comp(A, ctx, x, H.frame_offsets(n, 256), A.NOOP, False, 0.0))
        fulls.append(ctx.decompress_host(recs[-1]))
        assert len(fulls[-1]) == n
    return recs, fulls


def _assert_same(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        g, w = M.words(got), M.words(want)
        bad = np.argwhere((g != w).any(axis=1))[:, 0]
        at = int(bad[0]) if len(bad) else -1  # (-1: the records differ in a NaN's bits alone)
        assert False, (label, len(bad), at, got[at], want[at])


def _ranges(total):
    """ranges that begin odd and even, overlap, come unsorted, are empty, have count == 1, end at the shortest stream's last
    sample and (last) span the whole of it"""
    return [(2048, 1500), (1, 2051), (2500, 1000), (777, 0), (3001, 1), (2047, 2050), (total - 1235, 1235), (total, 0),
            (0, 40), (9, 10), (0, total)]


def test_the_streams_hold_what_the_cases_need(five, many, wide):
    recs, fulls, total = five
    x = np.array([f[:total] for f in fulls])
    assert np.isinf(x).any() and np.isnan(x).any() and np.isnan(x[:, :8]).all()
    assert (x[:, 8:16] == 0.0).any() and np.signbit(x[:, 8:16]).any()
    assert (x[3] == x[4]).sum() > 100  # two different streams agree on a value
    m = np.array(many[1])
    d = [len(np.unique(c[~np.isnan(c)])) for c in m.T]
    assert min(d) <= 3 and 4 <= max(d) <= 8 and len(np.unique(m[~np.isnan(m)])) < 12  # columns repeat
    assert (m == 0.0).any() and not np.signbit(m[m == 0.0]).any()
    w = np.array(wide[1])
    d = [len(np.unique(c)) for c in w.T]
    assert d[:200] == [64] * 200 and 32 < min(d[200:]) and max(d[200:]) < 64


# (k, above) so that every k and every kind of `above` occurs; 1234.5678, 1.0 and 2.0 are samples' values
CASES = [(1, NAN), (2, 1234.5678), (3, 0.0), (31, -0.0), (32, INF), (4, -INF), (32, NAN), (3, 1.0)]


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_every_record_matches_the_model(A, ctx, five, n):
    recs, fulls, total = five
    rg = _ranges(total)
    b, c = [x[0] for x in rg], [x[1] for x in rg]
    for (k, above), s in [(ka, 1) for ka in CASES] + [(CASES[1], 2), (CASES[6], 7), (CASES[2], 5000)]:
        got, off = ctx.across_values_windows_host(recs[:n], b, c, k, s, above)
        want, woff = M.across_values(fulls[:n], b, c, k, s, above)
        assert off.tolist() == woff.tolist() == A.across_offsets(c, s).tolist()
        assert off[3] == off[4] and off[5] - off[4] == 1 and off[7] == off[8]  # empty: none; count == 1: one
        assert got.dtype == A.window_values_dtype(k) == M.dtype(k)
        _assert_same(got, want, (n, k, above, s))
        assert np.all(got["count"] == n)
    # the zone where every stream is NaN, then zeros of both signs as one class reported as +0.0
    z, _ = ctx.across_values_windows_host(recs[:n], [0], [24], 2)
    assert np.all(z["nans"][:8] == n) and np.all(z["distinct"][:8] == 0)
    zero = z["entry"]["value"][8:16][z["entry"]["value"][8:16] == 0.0]
    assert len(zero) and not np.signbit(zero).any()


@pytest.mark.parametrize("n", [4, 8, 9, 16, 17, 32, 33, 63, 64])
def test_many_streams(A, ctx, many, n):
    recs, fulls = many
    recs, fulls = recs[:n], fulls[:n]
    b, c = [0, 1, 2001], [3000, 1500, 999]
    pick = [8, 9, 16, 17, 32, 33, 63, 64, 4].index(n)
    for (k, above), s in ((CASES[pick % 8], 1), ((KS[pick % 5], 1.0), 1), ((KS[(pick + 2) % 5], NAN), 3)):
        got, off = ctx.across_values_windows_host(recs, b, c, k, s, above)
        want, woff = M.across_values(fulls, b, c, k, s, above)
        assert off.tolist() == woff.tolist()
        _assert_same(got, want, (n, k, above, s))
        assert np.all(got["count"] == n) and (got["nans"] > 0).any() and (got["nans"] == 0).any()
    # against the across' count and min, and the across histograms' bins (k above every column's distinct values)
    got, off = ctx.across_values_windows_host(recs, b, c, 8, 3)
    assert not got["more"].any() and (got["distinct"] > 1).any()
    acr, aoff = ctx.across_windows_host(recs, b, c, 3)
    assert aoff.tolist() == off.tolist() and np.array_equal(got["count"] - got["nans"], acr["count"].astype(np.uint64))
    some = acr["count"] > 0
    assert some.any() and np.array_equal(got["entry"]["value"][some, 0], acr["min"][some] + 0.0)
    edges = [-2.0, -0.5, 0.0, 1.0]
    rows, _ = ctx.across_histogram_windows_host(recs, b, c, edges, 3)
    bins = np.zeros_like(rows)
    ev, en = got["entry"]["value"], got["entry"]["n"]
    for j in range(8):
        ok = ~np.isnan(ev[:, j])
        np.add.at(bins, (np.nonzero(ok)[0], np.searchsorted(edges, ev[ok, j], side="right")), en[ok, j])
    bins[:, -1] = got["nans"]
    assert np.array_equal(bins, rows)


@pytest.mark.parametrize("n", [33, 63, 64])
def test_columns_of_more_than_32_distinct_values(A, ctx, wide, n):
    recs, fulls = wide
    recs, fulls = recs[:n], fulls[:n]
    b, c = [0, 601], [513, 65]
    for k, above, s in ((32, NAN, 1), (31, -1.0, 1), (32, 0.0, 2), (1, NAN, 1), (3, 5.0, 7)):
        got, _ = ctx.across_values_windows_host(recs, b, c, k, s, above)
        _assert_same(got, M.across_values(fulls, b, c, k, s, above)[0], (n, k, above, s))
    got, _ = ctx.across_values_windows_host(recs, b, c, 32)
    assert got["more"].any() and np.all(got["distinct"][got["more"] != 0] == 32)
    # paging: above = the last listed value walks a column in ceil(D / k) calls
    for k in (32, 20):
        col = np.array([f[100] for f in fulls])
        pages, above = [], NAN
        while True:
            r = ctx.across_values_windows_host(recs, [100], [1], k, 1, above)[0][0]
            pages.append(r)
            if not int(r["more"]):
                break
            above = float(r["entry"]["value"][int(r["distinct"]) - 1])
        want = M.pages(col, k)
        d = len(np.unique(col))
        assert len(pages) == len(want) == math.ceil(d / k) and d > 32
        _assert_same(np.array(pages), np.array(want), ("pages", n, k))
        listed = [float(v) for r in pages for v in r["entry"]["value"][: int(r["distinct"])]]
        assert listed == np.unique(col + 0.0).tolist()
        assert sum(int(e) for r in pages for e in r["entry"]["n"]) == n


def _dev_records(A, torch, dps, bodies, b, c, k, s, above, shift):
    """the device call into a sentinel-filled buffer that begins 8 * shift bytes behind a multiple of 16, with guard words
    behind the last record -> the records as a NumPy array"""
    m, w = int(AM.offsets(c, s)[-1]), 4 + 2 * k
    d = torch.full((shift + m * w + 8,), SENT, dtype=torch.int64, device="cuda")
    assert (d.data_ptr() + 8 * shift) % 16 == 8 * shift
    view, off = dps[0].across_values_windows(bodies[0], dps[1:], bodies[1:], b, c, k, d[shift:], s, above,
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = d.cpu().numpy().view(np.uint64)
    assert np.all(h[:shift] == SENT) and np.all(h[shift + m * w:] == SENT)  # the guards
    assert not np.any(h[shift: shift + m * w] == SENT)  # every word of every record is overwritten
    assert tuple(view.shape) == (m, 8 * w) and off.tolist() == AM.offsets(c, s).tolist()
    return h[shift: shift + m * w].copy().view(M.dtype(k))


def test_shapes_where_the_kernel_takes_another_path(A, ctx, torch, five):
    """ranges with an odd and an even first sample of every length around a wavefront, a task and two tasks; strides on
    both sides of a wavefront and beyond a range; results at a multiple of 16 bytes and 8 bytes off one"""
    recs, fulls, total = five
    lengths = [0, 1, 63, 64, 65, TASK - 1, TASK, TASK + 1, 2 * TASK + 1]
    rg = [(b0, n) for b0 in (1001, 1000) for n in lengths]
    rg += [(1000, 65), (1010, 3), (total - TASK - 1, TASK + 1), (total, 0), (2047, 2), (1, 700)]  # overlapping, unordered, empty
    b, c = [x[0] for x in rg], [x[1] for x in rg]
    bodies = [torch.from_numpy(np.frombuffer(r, dtype=np.uint8).copy()).to("cuda") for r in recs]
    dps = [A.DPlan(ctx, r) for r in recs]
    try:
        for (k, above), strides in (((3, NAN), (1, 2, 3, 7, 64, 2 * TASK + 7)), ((32, 0.0), (1, 7)), ((1, 1.0), (1, 2))):
            for s in strides:
                want, woff = M.across_values(fulls, b, c, k, s, above)
                host, off = ctx.across_values_windows_host(recs, b, c, k, s, above)
                assert off.tolist() == woff.tolist()
                _assert_same(host, want, ("host", k, s))
                for shift in (0, 1):
                    got = _dev_records(A, torch, dps, bodies, b, c, k, s, above, shift)
                    assert got.tobytes() == host.tobytes(), (k, s, shift)
    finally:
        for dp in dps:
            dp.close()


def test_against_the_listed_one_sample_windows(A, ctx, five, many):
    recs, fulls, total = five
    b, c, s = [3, 2000], [900, 301], 3
    pos = np.concatenate([b0 + s * np.arange(AM.outputs(c0, s)) for b0, c0 in zip(b, c)])
    for k, above in ((1, NAN), (3, 0.0), (32, 1.0)):
        singles = [ctx.values_windows_host(r, pos, np.ones(len(pos), dtype=np.uint64), k, above) for r in recs]
        for j in (2, 4):  # N = 1: byte for byte the listed windows' records
            one, _ = ctx.across_values_windows_host([recs[j]], b, c, k, s, above)
            assert one.dtype == singles[j].dtype and one.tobytes() == singles[j].tobytes(), (k, j)
        allfive, _ = ctx.across_values_windows_host(recs, b, c, k, s, above)  # N = 5: the merge of them
        merged = np.array([A.values_merge(np.array([x[p] for x in singles]), k) for p in range(len(pos))])
        assert allfive.tobytes() == merged.tobytes(), k
        # records of sub-lists merge to the whole list's; a reversed and a permuted list give the same bytes
        front, _ = ctx.across_values_windows_host(recs[:2], b, c, k, s, above)
        back, _ = ctx.across_values_windows_host(recs[2:], b, c, k, s, above)
        both = np.array([A.values_merge(np.array([front[p], back[p]]), k) for p in range(len(pos))])
        assert both.tobytes() == allfive.tobytes()
        for order in ((4, 3, 2, 1, 0), (3, 0, 4, 2, 1)):
            perm, _ = ctx.across_values_windows_host([recs[j] for j in order], b, c, k, s, above)
            assert perm.tobytes() == allfive.tobytes()
        acr, _ = ctx.across_windows_host(recs, b, c, s)
        assert np.array_equal(allfive["count"] - allfive["nans"], acr["count"].astype(np.uint64))
        mode = A.values_mode(allfive, k)
        assert np.array_equal(mode["n"], allfive["entry"]["n"].max(axis=1))
    # two sub-lists of 32 merge to the list of 64
    recs, fulls = many
    whole, _ = ctx.across_values_windows_host(recs, [1000], [400], 3)
    lo, _ = ctx.across_values_windows_host(recs[:32], [1000], [400], 3)
    hi, _ = ctx.across_values_windows_host(recs[32:], [1000], [400], 3)
    both = np.array([A.values_merge(np.array([lo[p], hi[p]]), 3) for p in range(400)])
    assert both.tobytes() == whole.tobytes() and whole["more"].any()
    assert ctx.across_values_windows_host(recs[::-1], [1000], [400], 3)[0].tobytes() == whole.tobytes()


def test_one_position_through_different_ranges_and_strides(A, ctx, five):
    recs, fulls, total = five
    for q in (1234, 17, 4096):
        ref, _ = ctx.across_values_windows_host(recs, [q], [1], 3)
        assert ref.shape == (1,)
        _assert_same(ref, M.across_values(fulls, [q], [1], 3)[0], q)
        for b, c, s in ((q - 14 if q >= 14 else q % 7, 100, 7), (q % 500, total - q % 500, 500), (q, total - q, 2),
                        (1, total - 1, q - 1), (q - 1, 2, 1), (q % 2, q + 2, 2), (q - 1, 3, 1), (q, 700, 1), (q - 513, 600, 1)):
            if b < 0:
                continue
            got, off = ctx.across_values_windows_host(recs, [0, b, 2048], [3, c, 30], 3, s)
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
        x = np.rint(rng.normal(0, 1.5, LONG)) + 0.0
        recs.append(_comp(A, ctx, x, H.frame_offsets(LONG, 4096), A.NOOP, False, 0.0))
    # the large-frame stream: an 8192-sample frame over [63488, 71680), across the least budget's first piece end at 65536
    x = np.rint(rng.normal(0, 1.5, LONG)) + 0.0
    r = _comp(A, ctx, x[:63488], H.frame_offsets(63488, 4096), A.NOOP, False, 0.0)
    r += _comp(A, ctx, H.synth_series(4130, 8192, klass=1), np.array([0, 8192], dtype=np.uint64), A.FFT, True, 0.01)
    r += _comp(A, ctx, x[71680:], H.frame_offsets(LONG - 71680, 4096), A.NOOP, False, 0.0)
    recs.append(r)
    fulls = [ctx.decompress_host(v) for v in recs]
    assert all(len(f) == LONG for f in fulls)
    k, above = 3, -1.0
    b, c = [0, 90001], [LONG, 30000]  # the second range begins odd and crosses the least budget's piece end at 131072
    far = 70001  # a stride longer than a piece of the least budget
    want7, _ = M.across_values(fulls, b, c, k, 7, above)
    wantfar, _ = M.across_values(fulls, b, c, k, far, above)
    ref, _ = ctx.across_values_windows_host(recs, b, c, k, 1, above)
    _assert_same(ref[::7][: len(want7) // 2], M.across_values(fulls, [0], [LONG], k, 7, above)[0][: len(want7) // 2], "default")
    _assert_same(ref[int(AM.outputs(LONG, 1)):], M.across_values(fulls, b[1:], c[1:], k, 1, above)[0], "default, second range")
    # 64 plans share the budget: every stream sixteen times, ranges across the least budget's piece ends
    many_recs, many_fulls = [recs[j % 4] for j in range(64)], [fulls[j % 4] for j in range(64)]
    b64, c64 = [60001, 130000, 5], [12000, 2100, 0]
    want64, _ = M.across_values(many_fulls, b64, c64, 4, 1, NAN)
    ref64, _ = ctx.across_values_windows_host(many_recs, b64, c64, 4, 1, NAN)
    _assert_same(ref64, want64, "64, default")
    two, least = 8 * (4 * 100352 + 2 * 131072), 1
    assert _pieces(LONG, 8 * (2 ** 24 + 2 * 131072), 4, 1) == 1 and _pieces(LONG, two, 4, 1) == 2 and _pieces(LONG, least, 4, 1) == 4
    assert _pieces(LONG, least, 64, 16) == 4 and far > 65536
    try:
        for budget in (two, least):
            ctx.set_aggregate_scratch(budget)
            got, _ = ctx.across_values_windows_host(recs, b, c, k, 1, above)
            assert got.tobytes() == ref.tobytes(), budget
            _assert_same(ctx.across_values_windows_host(recs, b, c, k, 7, above)[0], want7, (budget, 7))
            _assert_same(ctx.across_values_windows_host(recs, b, c, k, far, above)[0], wantfar, (budget, far))
            got64, _ = ctx.across_values_windows_host(many_recs, b64, c64, 4, 1, NAN)
            assert got64.tobytes() == ref64.tobytes(), budget
    finally:
        ctx.set_aggregate_scratch(0)


def test_host_device_stream_and_image_calls_agree(A, ctx, torch):
    bros, fulls = [], []
    for j in range(3):
        x = np.rint(H.synth_series(5140 + j, 20000 + 100 * j, block=7000) / 4.0) + 0.0
        bros.append(A.compress_data(ctx, x, A.NOOP, 3))
        fulls.append(A.decompress_data(ctx, bros[-1]))
    p0 = [H.varint_decode(bro, 9)[1] for bro in bros]
    bodies = [torch.from_numpy(np.frombuffer(bro[p:], dtype=np.uint8).copy()).to("cuda") for bro, p in zip(bros, p0)]
    dps = [A.DPlan(ctx, bro[p:]) for bro, p in zip(bros, p0)]
    sts = [A.CompressedStream.from_bytes(ctx, bro) for bro in bros]
    try:
        for s, k, above in ((1, 2, NAN), (7, 32, float(fulls[0][10001]))):
            b, c = [10001, 5000, 19000], [7000, 6001, 100]  # begins far into the streams: the host call uploads a part
            want, woff = M.across_values(fulls, b, c, k, s, above)
            via_bro, off = A.across_values_data_windows(ctx, bros, b, c, k, s, above)
            _assert_same(via_bro, want, s)
            assert off.tolist() == woff.tolist()
            host, _ = ctx.across_values_windows_host([bro[9:] for bro in bros], b, c, k, s, above, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), s
            plain, _ = ctx.across_values_windows_host([bro[p:] for bro, p in zip(bros, p0)], b, c, k, s, above)
            assert plain.tobytes() == via_bro.tobytes(), s
            assert sts[0].across_values_windows(sts[1:], b, c, k, s, above)[0].tobytes() == via_bro.tobytes(), s
            for shift in (0, 1):
                assert _dev_records(A, torch, dps, bodies, b, c, k, s, above, shift).tobytes() == via_bro.tobytes(), (s, shift)
        # the same plan and the same stream twice in a list
        twice = M.across_values([fulls[0], fulls[1], fulls[0]], [15000], [100], 2)[0]
        got = _dev_records(A, torch, [dps[0], dps[1], dps[0]], [bodies[0], bodies[1], bodies[0]], [15000], [100], 2, 1, NAN, 0)
        _assert_same(got, twice, "twice")
        _assert_same(sts[0].across_values_windows([sts[1], sts[0]], [15000], [100], 2)[0], twice, "twice, streams")
        assert np.all(twice["entry"]["n"].max(axis=1) >= 2)
    finally:
        for dp in dps:
            dp.close()


def _ptrs(values):
    return (C.c_void_p * max(len(values), 1))(*values)


def _raw_host(A, ctx, bufs, rg, s, n_streams=None, null_list=False, null_entry=None, n_out=16, misalign=False, k=2, above=NAN):
    out = np.full(8 * n_out + 1, SENT, dtype=np.uint64)
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    ptr = [x.ctypes.data for x in bufs]
    if null_entry is not None:
        ptr[null_entry] = None
    lens = np.array([len(x) for x in bufs], dtype=np.uint64)
    flags = np.zeros(max(len(bufs), 1), dtype=np.int32)
    rc = A.capi.lib().atsc_across_values_windows(
        ctx._h, len(bufs) if n_streams is None else n_streams, None if null_list else _ptrs(ptr), lens.ctypes.data_as(p),
        flags.ctypes.data_as(C.POINTER(C.c_int32)), len(rg), b.ctypes.data_as(p), c.ctypes.data_as(p), s, k, above,
        C.c_void_p(out.ctypes.data + (4 if misalign else 0)))
    return rc, out


def _raw_dev(A, ctx, torch, dps, bodies, rg, s, n_streams=None, null_list=False, null_entry=None, misalign=False, k=2, above=NAN,
             n_out=None):
    d = torch.full((128,), SENT, dtype=torch.int64, device="cuda")
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    plans, ptr = [x._h.value for x in dps], [x.data_ptr() for x in bodies]
    if null_entry is not None:
        plans[null_entry] = None
    rc = A.capi.lib().atsc_across_values_windows_dev(
        ctx._h, len(dps) if n_streams is None else n_streams, None if null_list else _ptrs(plans), _ptrs(ptr), len(rg),
        b.ctypes.data_as(p), c.ctypes.data_as(p), s, k, above, C.c_void_p(d.data_ptr() + (4 if misalign else 0)),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bool((d == SENT).all())


def test_errors_leave_the_result_untouched(A, ctx, torch):
    rng = np.random.default_rng(7)
    Ec = A.capi
    lens = (9000, 9000, 6000)  # only stream 2 of 3 is too short for a range past 6000
    recs = [_comp(A, ctx, np.rint(rng.normal(0, 1, n)) + 0.0, H.frame_offsets(n, 1024), A.NOOP, False, 0.0) for n in lens]
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in recs]
    # every case of the across call
    cases = [dict(rg=[(0, 10)], s=1, n_streams=0), dict(rg=[(0, 10)], s=1, n_streams=65), dict(rg=[(0, 10)], s=1, null_list=True),
             dict(rg=[(0, 10)], s=1, null_entry=1), dict(rg=[(0, 10)], s=0), dict(rg=[(0, 2 ** 33)], s=1),
             dict(rg=[(0, 2 ** 32 - 1), (0, 5)], s=1), dict(rg=[(0, 7000)], s=1), dict(rg=[(0, 10), (5999, 2)], s=1),
             dict(rg=[(0, 10), (6001, 0)], s=1), dict(rg=[(2 ** 63, 2 ** 63)], s=1), dict(rg=[(2 ** 64 - 1, 2)], s=3)]
    # k, with and without an `above`
    cases += [dict(rg=[(0, 10)], s=1, k=0), dict(rg=[(0, 10)], s=1, k=33), dict(rg=[(0, 10)], s=1, k=2 ** 32 - 1),
              dict(rg=[(0, 10)], s=1, k=0, above=1.0), dict(rg=[], s=1, k=33)]
    # and the result pointer's
    cases += [dict(rg=[(0, 2)], s=1, misalign=True), dict(rg=[(0, 2)], s=2, misalign=True)]
    for kw in cases:
        rc, out = _raw_host(A, ctx, bufs, **kw)
        assert rc == Ec.E_INVALID and np.all(out == SENT), (kw, rc)
    msg = A.capi.lib().atsc_ctx_last_error(ctx._h).decode()
    assert msg.startswith("across_values_windows: "), msg
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
            sa.across_values_windows([sb], [0], [10], 2)  # streams of different contexts
        assert ei.value.rc == Ec.E_INVALID
        with pytest.raises(A.AtscError) as ei:
            sa.across_values_windows([sa], [0], [10], 2, 0)  # stride 0
        assert ei.value.rc == Ec.E_INVALID
        for k in (0, 33):
            with pytest.raises(A.AtscError) as ei:
                sa.across_values_windows([sa], [0], [10], k)
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
    rc, out = _raw_host(A, ctx, bufs[:2], [(0, 7000)], 1000)  # 7 records of 8 words
    assert rc == 0 and np.all(out[56:] == SENT) and not np.any(out[:56] == SENT) and np.all(out[:56].reshape(7, 8)[:, 0] == 2)
    rc, out = _raw_host(A, ctx, bufs, [], 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufs, [(5, 0), (6000, 0)], 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, bufs, [(5999, 1)], 1)  # the shortest stream's last sample
    assert rc == 0 and np.all(out[8:] == SENT)
    x = np.array([ctx.decompress_window_host(r, 5999, 1)[0] for r in recs])
    _assert_same(out[:8].copy().view(M.dtype(2)), M.records(x[:, None], 2), "last sample")


def test_malformed_payload_in_one_stream_of_three(A, ctx, torch):
    n, nf = 256, 8
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs = [_comp(A, ctx, H.synth_series(920 + j, n * nf, klass=2), off, A.FFT, True, 0.05) for j in range(3)]
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
        got, _ = ctx.across_values_windows_host(lst, b, c, 3, s)
        _assert_same(got, M.across_values(good, b, c, 3, s)[0], ("outside", s))
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
        want, off = M.across_values(good, [w[0] for w in rg], [w[1] for w in rg], 3)
        got = _dev_records(A, torch, dps, bodies, [w[0] for w in rg], [w[1] for w in rg], 3, 1, NAN, 0)
        clean = np.r_[0: int(off[1]), int(off[2]): int(off[3])]
        _assert_same(got[clean], want[clean], "dev, beside the bad frame")
        assert np.all(got["count"] == 3)
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
        _run(atsc, "--compressor", "noop", src)
        bros.append((tmp_path / (name + ".bro")).read_bytes())
    fulls = [A.decompress_data(ctx, b) for b in bros]
    total = min(len(f) for f in fulls)
    assert total > 1000
    paths = [tmp_path / (name + ".bro") for name in names]
    header = "offset,count,min,min_at,max,max_at,sum,mean"
    mid = float(np.nanmedian(fulls[0]))
    for (n, (b0, c0), s, more), (spec, k, above) in zip(
            ((2, (0, total), None, []), (3, (7, 1000), 15, ["--across-quantiles", "0.5,0.9", "--across-moments"]),
             (3, (total - 1, 1), 4, [])), (("2", 2, NAN), ("3:%r" % mid, 3, mid), ("32:-inf", 32, -INF))):
        listed = ",".join(str(p) for p in paths[1:n])
        front = (["--across-stride", s] if s else []) + more
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--across", listed, *front, "--across-values", spec, paths[0])
        lines = (tmp_path / "uptime.across.csv").read_text().split("\n")
        new = ["vcount", "vnans", "vbelow", "vdistinct", "vmore"] + [t % e for e in range(k) for t in ("v%d", "n%d")]
        nf = len(lines[0].split(",")) - len(new)  # the columns in front
        assert lines[0].split(",")[nf:] == new and nf == 8 + (2 + 4 if more else 0)
        rows = [l.split(",") for l in lines[1:] if l]
        s = s or 1
        want, _ = A.across_values_data_windows(ctx, bros[:n], [b0], [c0], k, s, above)
        _assert_same(want, M.across_values(fulls[:n], [b0], [c0], k, s, above)[0], spec)
        assert len(rows) == len(want) == AM.outputs(c0, s) > 0 and all(len(r) == nf + len(new) for r in rows)
        got = np.zeros(len(rows), dtype=M.dtype(k))
        got["entry"]["value"] = NAN
        for i, r in enumerate(rows):
            v = r[nf:]
            got[i]["count"], got[i]["nans"], got[i]["below"], got[i]["distinct"], got[i]["more"] = (int(t) for t in v[:5])
            for e in range(k):
                assert (v[5 + 2 * e] == "") == (v[6 + 2 * e] == "") == (e >= got[i]["distinct"])
                if v[5 + 2 * e]:
                    got[i]["entry"][e] = (float(v[5 + 2 * e]), int(v[6 + 2 * e]))
        _assert_same(got, want, ("csv", spec))
        assert np.all(got["count"] == n)
        assert np.array_equal(got["count"] - got["nans"], np.array([int(r[1]) for r in rows], dtype=np.uint64))
        # without the option the file is what it was: the columns in front, byte for byte
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--across", listed, *front, paths[0])
        plain = (tmp_path / "uptime.across.csv").read_text()
        assert plain.split("\n")[0].startswith(header) and (plain.split("\n")[0] == header) == (not more)
        assert plain == "\n".join(",".join(l.split(",")[:nf]) if l else l for l in lines)
