"""Windowed rolling on the GPU: every record of every case against the NumPy model of the contract
(tests/rolling_model.py) applied to the GPU's own full decode -- count, min, max and sum bit for bit, any NaN equal to any
NaN, no tolerance.  The main stream holds every frame-length tier below the large one under every codec, one 8192-sample
frame of the large tier and Constant records of NaN, +-Inf and zeros of both signs; a long stream of Noop frames serves the
width across the 2^16 level and the budgets that cut a range into pieces.  Against atsc_aggregate_windows on the listed
windows; the same position through different ranges and strides; the host, device and stream calls; errors that leave the
result untouched; a malformed payload; both command lines."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import rolling_model as M

pytestmark = pytest.mark.gpu

LENS = [1, 7, 64, 128, 256, 300, 512, 513, 1024, 2048, 4096]
WIDTHS = [1, 2, 3, 63, 64, 65, 300, 2047, 2048, 2049, 4097]
CONSTANTS = [(1.0, 3), (np.nan, 5), (-0.0, 2), (2.5, 4), (np.nan, 3000), (-7.0, 2), (np.inf, 3), (1.0, 1), (-np.inf, 2),
             (np.nan, 1), (-0.0, 4), (0.0, 1), (3.0, 2), (0.0, 3), (-0.0, 2100), (0.0, 5), (-1.0, 1)]
LONG = 200000
SENT = 0x5A5A5A5A5A5A5A5A


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
    """a Constant record of n samples of `value` as it is (NaN, +-Inf, -0.0 included): the library's own 64-bit Constant
    record of a stand-in, with the stored double replaced"""
    r, _, _, _ = ctx.compress_host(np.full(n, 1.5), np.array([0, n], dtype=np.uint64), A.CONSTANT, False, 0.0, 0)
    assert r.endswith(struct.pack("<d", 1.5))
    return r[:-8] + struct.pack("<d", value)


@pytest.fixture(scope="module")
def main(A, ctx):
    """-> (records, full decode, model pyramid, first sample of the Constant records)"""
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
    return recs, full, M.Pyramid(full), at


@pytest.fixture(scope="module")
def long(A, ctx):
    """200000 samples of mixed magnitude with NaN holes in Noop frames of 4096: cheap to build and to decode"""
    rng = np.random.default_rng(23)
    x = np.round(rng.normal(0, 1, LONG) * 10.0 ** rng.integers(-3, 6, LONG), 6)
    x[rng.random(LONG) < 0.01] = np.nan
    recs = ctx.compress_host(x, H.frame_offsets(LONG, 4096), A.NOOP, False, 0.0, 0)[0]
    full = ctx.decompress_host(recs)
    assert len(full) == LONG
    return recs, full, M.Pyramid(full)


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


def _ranges(total, w, at):
    """ranges that begin at odd and at aligned indices, overlap, come unsorted, are shorter than w, equal w, empty, lie
    over the Constant records, and (last) span the whole stream"""
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
        got, off = ctx.rolling_windows_host(recs, b, c, w, s)
        want, woff = P.rolling(b, c, w, s)
        assert off.tolist() == woff.tolist() and got.dtype == A.WINDOW_ROLLING
        assert off[3] == off[4] == off[5] and off[3] - off[2] == 1  # shorter than w: none; equal w: one
        _assert_same(got, want, (w, s))


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
            d = torch.full((4 * len(want) + 8,), SENT, dtype=torch.int64, device="cuda")
            off = dp.rolling_windows(body, b, c, w, s, d, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            h = d.cpu().numpy()
            assert off.tolist() == woff.tolist() and np.all(h[4 * len(want):] == SENT)
            _assert_same(h[: 4 * len(want)].view(A.WINDOW_ROLLING), want, (w, s))
            host, _ = ctx.rolling_windows_host(recs, b, c, w, s)
            assert host.tobytes() == h[: 4 * len(want)].tobytes(), s
    finally:
        dp.close()


def test_against_the_aggregate_on_the_listed_windows(A, ctx, main):
    recs, full, P, at = main
    total = len(full)
    for w, s in ((1, 1), (3, 1), (300, 7), (2049, 5), (4097, 11)):
        rg = [(max(at - w - 40, 0), min(2 * w + 5300, total - max(at - w - 40, 0))), (1, min(w + 2000, total - 1))]
        b, c = [x[0] for x in rg], [x[1] for x in rg]
        got, off = ctx.rolling_windows_host(recs, b, c, w, s)
        lo = np.concatenate([rg[i][0] + s * np.arange(int(off[i + 1] - off[i])) for i in range(len(rg))])
        agg = ctx.aggregate_windows_host(recs, lo, np.full(len(lo), w))
        for k in ("count", "min", "max"):
            x, y = got[k].view(np.uint64), agg[k].view(np.uint64)
            same = (x == y) | (np.isnan(got[k].view(np.float64)) & np.isnan(agg[k].view(np.float64)) if k != "count" else False)
            assert np.all(same), (w, s, k, int(np.flatnonzero(~same)[0]))
        for i, b0 in enumerate(lo):
            v = full[b0:b0 + w]
            if not np.all(np.isfinite(v[~np.isnan(v)])):
                assert np.isnan(got["sum"][i]) == np.isnan(agg["sum"][i]) and (np.isnan(got["sum"][i]) or got["sum"][i] == agg["sum"][i])
                continue
            assert abs(got["sum"][i] - agg["sum"][i]) <= M.error_bound(v), (w, s, i)
    # zeros of both signs in one window: the extreme's sign is the aggregate's, wherever the window begins
    z = at + sum(n for _, n in CONSTANTS[:10])
    assert full[z] == 0.0 and np.signbit(full[z]) and not np.signbit(full[z + 4])
    mixed = 0
    for w in (5, 8, 2110):
        got, off = ctx.rolling_windows_host(recs, [z - 3], [w + 30], w, 1)
        lo = z - 3 + np.arange(len(got))
        agg = ctx.aggregate_windows_host(recs, lo, np.full(len(lo), w))
        assert got["min"].tobytes() == agg["min"].tobytes() and got["max"].tobytes() == agg["max"].tobytes()
        for i, b0 in enumerate(lo):
            v = full[b0:b0 + w]
            zero = v[v == 0.0]
            mixed += int(len(set(np.signbit(zero))) == 2 and (got["min"][i] == 0.0 or got["max"][i] == 0.0))
    assert mixed >= 3


def test_one_position_through_different_ranges(A, ctx, main):
    recs, full, P, at = main
    for w in (3, 65, 2049):
        lo = 40 * w + 77
        ref, _ = ctx.rolling_windows_host(recs, [lo], [w], w, 1)
        assert len(ref) == 1
        for b, c, s in ((lo - 7 * 5, 9 * 7 + w, 7), (lo - 3 * w, 5 * w, w), (1, len(full) - 1, lo - 1), (lo, len(full) - lo, 2 * w + 1)):
            got, off = ctx.rolling_windows_host(recs, [0, b, 2048], [w + 1, c, 3 * w], w, s)
            j = int(off[1]) + (lo - b) // s
            assert (lo - b) % s == 0 and got[j: j + 1].tobytes() == ref.tobytes(), (w, b, c, s)
        _assert_same(ref, P.records([lo], w), w)


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
        for w, s in ((300, 1), (64, 7), (4097, 3)):
            b, c = [30001, 20000, 47000], [15000, 12001, 100]  # begins far into the stream: the host call uploads a part
            want, woff = P.rolling(b, c, w, s)
            via_bro, off = A.rolling_data_windows(ctx, bro, b, c, w, s)
            _assert_same(via_bro, want, (w, s))
            assert off.tolist() == woff.tolist()
            host, _ = ctx.rolling_windows_host(bro[9:], b, c, w, s, has_count=True)
            assert host.tobytes() == via_bro.tobytes(), (w, s)
            assert st.rolling_windows(b, c, w, s)[0].tobytes() == via_bro.tobytes(), (w, s)
            d = torch.zeros(4 * len(want) + 1, dtype=torch.int64, device="cuda")
            dp.rolling_windows(body, b, c, w, s, d, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert d.cpu().numpy()[: 4 * len(want)].tobytes() == via_bro.tobytes(), (w, s)
    finally:
        dp.close()


def _pieces(n, budget, w):
    """the pieces of a range of n samples from sample 0 of a stream without large frames under a budget, by DESIGN.md's
    piece arithmetic: a region of Lr = max(65536, budget / 8 / 2 rounded down to 2048) samples, a piece of Lr - 3 * 2048,
    consecutive pieces overlapping by w - 1"""
    lp = max(65536, budget // 8 // 2 // 2048 * 2048) - 3 * 2048
    k, p = 1, 0
    while p + lp < n:
        p, k = p + lp - (w - 1), k + 1
    return k


def test_pieces_do_not_change_the_bytes(A, ctx, long, main):
    recs, full, P = long
    w = 3000
    b, c = [0, 90001], [LONG, 30000]
    ref, _ = ctx.rolling_windows_host(recs, b, c, w, 1)
    _assert_same(ref, P.rolling(b, c, w, 1)[0], "default")
    two, three = 2 * 110592 * 8, 1
    assert _pieces(LONG, two, w) == 2 and _pieces(LONG, three, w) >= 3
    try:
        for budget in (two, three):
            ctx.set_aggregate_scratch(budget)
            got, _ = ctx.rolling_windows_host(recs, b, c, w, 1)
            assert got.tobytes() == ref.tobytes(), budget
            got7, _ = ctx.rolling_windows_host(recs, b, c, w, 7)
            assert got7.tobytes() == ref[: LONG - w + 1][::7].tobytes() + ref[LONG - w + 1:][::7].tobytes(), budget
        # the main stream under the least budget: a large frame across the pieces' ends
        mrecs, mfull, MP, _ = main
        ctx.set_aggregate_scratch(1)
        got, _ = ctx.rolling_windows_host(mrecs, [0], [len(mfull)], w, 1)
    finally:
        ctx.set_aggregate_scratch(0)
    assert len(mfull) > 65536
    _assert_same(got, MP.rolling([0], [len(mfull)], w, 1)[0], "main, least budget")


def test_a_window_of_nan(A, ctx, main):
    recs, full, P, at = main
    z = at + 3 + 5 + 2 + 4  # the 3000 NaN samples
    assert np.isnan(full[z:z + 3000]).all() and not np.isnan(full[z - 1]) and not np.isnan(full[z + 3000])
    got, off = ctx.rolling_windows_host(recs, [z - 2], [3004], 300, 1)
    assert len(got) == 2705
    inside = got[2: 2 + 2701]
    assert np.all(inside["count"] == 0) and np.isnan(inside["min"]).all() and np.isnan(inside["max"]).all()
    assert np.all(inside["sum"].view(np.uint64) == 0)  # +0.0
    assert got["count"][1] == 1 and got["count"][-1] == 2 and got["min"][1] == 2.5


def _raw_host(A, ctx, buf, rg, w, s, n_out=16):
    out = np.full(4 * n_out, SENT, dtype=np.uint64)
    b = np.array([x[0] for x in rg], dtype=np.uint64)
    c = np.array([x[1] for x in rg], dtype=np.uint64)
    p = C.POINTER(C.c_uint64)
    rc = A.capi.lib().atsc_rolling_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(rg),
                                           b.ctypes.data_as(p), c.ctypes.data_as(p), w, s, C.c_void_p(out.ctypes.data))
    return rc, out


def test_errors_leave_the_result_untouched(A, ctx, torch, long):
    recs, full, P = long
    buf = np.frombuffer(recs, dtype=np.uint8)
    E = A.capi
    cases = [([(0, 100)], 0, 1, E.E_INVALID), ([(0, 100)], A.ROLLING_MAX_WIDTH + 1, 1, E.E_INVALID), ([(0, 100)], 10, 0, E.E_INVALID),
             ([(LONG - 50, 100)], 10, 1, E.E_INVALID), ([(0, 20), (LONG + 1, 0)], 10, 1, E.E_INVALID),
             ([(2 ** 63, 2 ** 63)], 10, 1, E.E_INVALID), ([(0, 2 ** 33)], 1, 1, E.E_INVALID)]
    for rg, w, s, want in cases:
        rc, out = _raw_host(A, ctx, buf, rg, w, s)
        assert rc == want and np.all(out == SENT), (rg, w, s, rc)
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(buf.copy()).to("cuda")
    try:
        for rg, w, s, want in cases:
            d = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
            b = np.array([x[0] for x in rg], dtype=np.uint64)
            c = np.array([x[1] for x in rg], dtype=np.uint64)
            p = C.POINTER(C.c_uint64)
            rc = E.lib().atsc_rolling_windows_dev(ctx._h, dp._h, C.c_void_p(body.data_ptr()), len(rg), b.ctypes.data_as(p),
                                                  c.ctypes.data_as(p), w, s, C.c_void_p(d.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            assert rc == want and bool((d == SENT).all()), (rg, w, s, rc)
        # a budget that cannot hold one window of the width
        ctx.set_aggregate_scratch(1)
        rc, out = _raw_host(A, ctx, buf, [(0, 70010)], 70001, 1)
        assert rc == E.E_CAPACITY and np.all(out == SENT)
        rc, out = _raw_host(A, ctx, buf, [(0, 59392 + 15)], 59392, 1)  # the widest that the least budget holds
        assert rc == 0 and np.all(out[64:] == SENT)
        _assert_same(out[:64].view(A.WINDOW_ROLLING), P.rolling([0], [59392 + 15], 59392, 1)[0], "widest")
    finally:
        ctx.set_aggregate_scratch(0)
        dp.close()
    rc, out = _raw_host(A, ctx, buf, [(0, 70010)], 70001, 1)  # the default budget holds any width
    assert rc == 0 and np.all(out[40:] == SENT) and not np.any(out[:40] == SENT)
    rc, out = _raw_host(A, ctx, buf, [], 5, 1)
    assert rc == 0 and np.all(out == SENT)
    rc, out = _raw_host(A, ctx, buf, [(5, 0), (LONG, 0), (7, 4)], 5, 1)  # no range holds a window: no record
    assert rc == 0 and np.all(out == SENT)


def test_malformed_payload(A, ctx):
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
    got, _ = ctx.rolling_windows_host(bad, b, c, 20, 3)
    _assert_same(got, P.rolling(b, c, 20, 3)[0], "outside")
    bb = np.frombuffer(bad, dtype=np.uint8)
    for rg in ([(3 * n, 20)], [(0, nf * n)], [(0, 40), (3 * n - 19, 20)], [(4 * n - 20, 20), (6 * n, 50)]):
        rc, out = _raw_host(A, ctx, bb, rg, 20, 1, n_out=nf * n)
        assert rc == A.capi.E_FORMAT and np.all(out == SENT), (rg, rc)


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def _back(A, rows):
    """the records that the rows of a .roll.csv parse back to"""
    back = np.zeros(len(rows), dtype=A.WINDOW_ROLLING)
    back["count"] = [int(r[1]) for r in rows]
    for k, name in ((2, "min"), (3, "max"), (4, "sum")):
        back[name] = [float(r[k]) for r in rows]
    return back


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
    for (t0, t1), spec, (w, s) in (((times[10], times[hi]), "20:3", (20, 3)), ((times[0], times[-1]), "5", (5, 1)),
                                   ((times[10], times[12]), "20", (20, 1))):
        for f in tmp_path.glob("win*"):
            f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--rolling", spec, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.roll.csv"]
        out = (tmp_path / "win.roll.csv").read_text().split("\n")
        assert out[0] == "timestamp,count,min,max,sum,mean"
        got = [l.split(",") for l in out[1:] if l]
        at = np.flatnonzero((times >= t0) & (times <= t1))
        b, c = int(at[0]), len(at)
        want, _ = A.rolling_data_windows(ctx, cbro, [b], [c], w, s)
        assert len(got) == len(want) == M.outputs(c, w, s)
        _assert_same(_back(A, got), want, spec)
        assert [int(r[0]) for r in got] == [int(times[b + j * s + w - 1]) for j in range(len(got))]  # the window's last sample
    r = subprocess.run([csvc, "-u", "--rolling", "5", str(tmp_path / "cpu.bro")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2


def test_command_line(A, ctx, golden_dir, tmp_path):
    atsc = os.path.join(os.path.dirname(A.__file__), "bin", "atsc")
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    for spec, (b0, c0), (w, s) in (("20", (0, len(full)), (20, 1)), ("300:15", (100, 1500), (300, 15)), ("64:64", (7, 1000), (64, 64))):
        _run(atsc, "-u", "--samples", "%d:%d" % (b0, c0), "--rolling", spec, tmp_path / "uptime.bro")
        lines = (tmp_path / "uptime.roll.csv").read_text().split("\n")
        assert lines[0] == "offset,count,min,max,sum,mean"
        rows = [l.split(",") for l in lines[1:] if l]
        want, _ = A.rolling_data_windows(ctx, bro, [b0], [c0], w, s)
        assert len(rows) == len(want) == M.outputs(c0, w, s) > 0
        assert [int(r[0]) for r in rows] == [j * s for j in range(len(rows))]
        _assert_same(_back(A, rows), want, spec)
        assert [float(r[5]) for r in rows] == [float(v["sum"]) / int(v["count"]) for v in want]
    for bad in (("-u", "--rolling", "5"), ("-u", "--samples", "0:10", "--rolling", "0"), ("-u", "--samples", "0:10", "--rolling", "5:0"),
                ("-u", "--samples", "0:10", "--buckets", "5", "--rolling", "5"), ("-u", "--samples", "0:10", "--rolling", "1048577")):
        r = subprocess.run([atsc, *bad, str(tmp_path / "uptime.bro")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, bad
