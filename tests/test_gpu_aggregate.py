"""Windowed aggregates on the GPU: count / min / max / first / last against NumPy on the full decode, sum bit for bit
against the NumPy model of the documented order (tests/agg_model.py) and within its error bound of math.fsum, over
every codec and frame-length tier; determinism across batches and budgets; NaN / Inf; validation; the dev, host, stream
and .bro entry points; a stream of 2^26 samples in many pieces; both command lines."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import agg_model as M
from tests import helpers as H
from tests.test_gpu_delta import _idw_record

pytestmark = pytest.mark.gpu

LENS = [1, 7, 64, 128, 256, 300, 512, 513, 1024, 4096, 4097, 6500, 8192, 20000, 65536, 131072]


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
def mixed(A, ctx):
    """every frame length of LENS under auto at e = 5 / 1 / 0 % and forced fft, polynomial, idw, rle, constant, noop;
    hand-built FFT records with 15 and 16 bins"""
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.uint64)
    modes = [(A.AUTO, True, 0.05), (A.AUTO, True, 0.01), (A.AUTO, True, 0.0), (A.FFT, True, 0.05),
             (A.POLYNOMIAL, True, 0.05), (A.IDW, True, 0.05), (A.RLE, False, 0.0), (A.CONSTANT, False, 0.0),
             (A.NOOP, False, 0.0)]
    recs = b""
    for m, (comp, bounded, me) in enumerate(modes):
        x = H.synth_series(700 + m, int(off[-1]), block=3000)
        if comp == A.RLE:
            x = np.round(x / 8.0) * 8.0
        r, _, _, _ = ctx.compress_host(x, off, comp, bounded, float(np.float32(me)), 0)
        recs += r
    rng = np.random.default_rng(3)
    for n in (128, 256, 1024, 2048, 4096):
        for k in (15, 16):
            recs += _fft_record(rng, n, k)
    return recs


@pytest.fixture(scope="module")
def grid(A, ctx):
    """a run of 131072-sample FFT frames (the large decoder's grid path)"""
    lens = [131072, 65536, 131072, 131072]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    x = H.synth_series(808, int(off[-1]), klass=1)
    r, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.01)), 0)
    return r


def _frame_lens(recs):
    return [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in H.parse_bro_body(recs, with_count=False)]


def _windows(lens, total, rng, n_random=120):
    w = {(0, total), (0, 0), (total, 0), (total - 1, 1), (0, 1)}
    for s in np.cumsum(lens)[:-1]:
        s = int(s)
        for b in (s - 1, s, s + 1):
            if b >= total:
                continue
            w.add((b, 1))
            w.add((max(b - 5, 0), min(11, total - max(b - 5, 0))))
    for _ in range(n_random):
        b = int(rng.integers(0, total))
        w.add((b, int(rng.integers(0, min(total - b, 300000) + 1))))
    return sorted(w)


def _bits(x):
    return np.float64(x).view(np.uint64)


def _check(full, wins, got, label=""):
    """count / min / max / first / last against NumPy, sum bit for bit against the model and within the bound"""
    assert len(got) == len(wins)
    for (b, c), r in zip(wins, got):
        v = full[b:b + c]
        ok = ~np.isnan(v)
        n, mn, mx, s, first, last = M.window_stats(full, b, c)
        assert int(r["count"]) == n == int(ok.sum()), (label, b, c)
        if n:
            assert r["min"] == np.nanmin(v) and r["max"] == np.nanmax(v), (label, b, c)
        else:
            assert np.isnan(r["min"]) and np.isnan(r["max"]), (label, b, c)
        if c:
            assert _bits(r["first"]) == _bits(v[0]) and _bits(r["last"]) == _bits(v[-1]), (label, b, c)
        else:
            assert np.isnan(r["first"]) and np.isnan(r["last"]), (label, b, c)
        assert _bits(r["sum"]) == _bits(s), (label, b, c, r["sum"], s)
        if n and np.all(np.isfinite(v[ok])):
            assert abs(float(r["sum"]) - math.fsum(v[ok])) <= M.error_bound(v), (label, b, c)


def _dev(A, ctx, torch, recs, wins):
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    d_stats = torch.full((max(len(wins), 1) * 6,), -1, dtype=torch.int64, device="cuda")
    dp.aggregate_windows(body, [w[0] for w in wins], [w[1] for w in wins], d_stats,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_stats.cpu().numpy().view(A.WINDOW_STATS)[: len(wins)].copy()
    dp.close()
    return out


def _host(ctx, recs, wins):
    return ctx.aggregate_windows_host(recs, [w[0] for w in wins], [w[1] for w in wins])


def _same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("which", ["mixed", "grid"])
def test_parity_with_full_decode(A, ctx, torch, mixed, grid, which):
    recs = mixed if which == "mixed" else grid
    full = ctx.decompress_host(recs)
    lens = _frame_lens(recs)
    assert sum(lens) == len(full)
    wins = _windows(lens, len(full), np.random.default_rng(19))
    got = _host(ctx, recs, wins)
    _check(full, wins, got, which)
    assert _same(_dev(A, ctx, torch, recs, wins), got)


def test_determinism(A, ctx, torch, mixed):
    full = ctx.decompress_host(mixed)
    total = len(full)
    rng = np.random.default_rng(29)
    probe = [(0, total), (5, 2043), (2047, 300000), (131071, 2), (total - 4097, 4097)]
    probe += [(int(b), int(rng.integers(1, 300000))) for b in rng.integers(0, total - 300000, 20)]
    alone = _host(ctx, mixed, probe)
    _check(full, probe, alone, "probe")
    others = []
    for _ in range(1000):
        c = int(rng.choice([1, 60, 2048, 5000, 40000]))
        others.append((int(rng.integers(0, total - c + 1)), c))
    batch = probe + others
    order = rng.permutation(len(batch))
    shuffled = [batch[i] for i in order]
    got = _host(ctx, mixed, shuffled)
    back = np.empty_like(got)
    back[order] = got
    assert _same(back[: len(probe)], alone)
    # overlapping batches: each probe window with its neighbours shifted by a few samples
    for b, c in probe[:6]:
        near = [(b, c), (max(b - 3, 0), c), (b, max(c - 7, 0)), (b + 1, max(c - 1, 0))]
        assert _same(_host(ctx, mixed, near)[:1], alone[probe.index((b, c)): probe.index((b, c)) + 1])
    # the least budget: many pieces, frames cut by piece boundaries
    ctx.set_aggregate_scratch(1)
    try:
        small = _host(ctx, mixed, shuffled)
        small_dev = _dev(A, ctx, torch, mixed, probe)
    finally:
        ctx.set_aggregate_scratch(0)
    assert _same(small, got)
    assert _same(small_dev, alone)
    assert _same(_host(ctx, mixed, probe), alone)  # repeated


def test_64_and_66_tiles_in_one_window(A, ctx, torch):
    """64 partials fill one combine group exactly, 65 and 66 need a second pass: windows of 64 and 66 tiles (135168
    samples) and their neighbours, on tile multiples and on odd slots, under the default budget and under the least one,
    whose pieces of 32 tiles cut every one of them"""
    T, nan = M.TILE, float("nan")
    n = 35 * 4096
    rng = np.random.default_rng(641)
    # decoding rounds to the fifth decimal, so the samples are placed on it; a sum of these depends on its order
    x = np.round(rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 7, n), 5)
    x[rng.integers(0, n, 300)] = nan
    recs = b"".join(_idw_record(x[k:k + 4096].tolist()) for k in range(0, n, 4096))
    full = ctx.decompress_host(recs)
    assert np.array_equal(np.isnan(full), np.isnan(x)) and np.array_equal(full[~np.isnan(x)], x[~np.isnan(x)])
    wins = [(2 * T, 64 * T), (2 * T - 1, 64 * T + 2), (T, 66 * T), (2 * T + 1, 66 * T - 1), (2 * T, 64 * T - 1),
            (2 * T + 1, 64 * T), (0, n), (T + 7, 65 * T), (3 * T, 64 * T), (2 * T, 65 * T), (5, 64 * T)]
    try:
        for budget in (0, 1):
            ctx.set_aggregate_scratch(budget)
            got = _host(ctx, recs, wins)
            _check(full, wins, got, "64 tiles, budget %d" % budget)
            assert _same(_dev(A, ctx, torch, recs, wins), got), budget
    finally:
        ctx.set_aggregate_scratch(0)


def test_non_finite_values(A, ctx):
    nan, inf = float("nan"), float("inf")
    parts = [(1.0, 3), (nan, 5), (-0.0, 2), (2.5, 4), (nan, 3000), (-7.0, 2), (inf, 3), (1.0, 1), (-inf, 2), (nan, 1),
             (-0.0, 4), (0.0, 1)]
    recs = b"".join(_const_record(A, ctx, v, n) for v, n in parts)
    full = ctx.decompress_host(recs)
    want = np.concatenate([np.full(n, v) for v, n in parts])
    assert np.array_equal(full.view(np.uint64), want.view(np.uint64))
    at = np.concatenate([[0], np.cumsum([n for _, n in parts])]).tolist()
    wins = [(0, at[4]), (at[1], 5), (at[1], 1), (at[4], 3000), (at[4] + 10, 100), (at[4] - 1, 3002), (at[6], 4),
            (at[6], 6), (at[8], 2), (at[6], 8), (at[10], 4), (at[10], 5), (at[9], 5), (0, at[-1]), (at[2], 0),
            (at[4] + 2047, 3)]
    got = _host(ctx, recs, wins)
    _check(full, wins, got, "nonfinite")
    r = dict(zip(wins, got))
    assert int(r[(0, at[4])]["count"]) == 9 and np.isnan(r[(at[1], 1)]["first"]) and int(r[(at[1], 1)]["count"]) == 0
    w = r[(at[4], 3000)]  # only NaNs, across two tiles: count 0, NaN extremes, sum +0.0, NaN first / last as stored
    assert int(w["count"]) == 0 and np.isnan(w["min"]) and np.isnan(w["max"])
    assert _bits(w["sum"]) == _bits(0.0) and np.isnan(w["first"]) and np.isnan(w["last"])
    assert np.isnan(r[(at[4] - 1, 3002)]["last"]) is np.False_ and np.isnan(r[(at[4] - 1, 3002)]["first"]) is np.False_
    assert int(r[(at[4] - 1, 3002)]["count"]) == 2
    assert r[(at[6], 4)]["sum"] == inf and r[(at[6], 4)]["max"] == inf
    assert np.isnan(r[(at[6], 6)]["sum"]) and r[(at[6], 6)]["min"] == -inf and r[(at[6], 6)]["max"] == inf
    assert _bits(r[(at[10], 4)]["sum"]) == _bits(-0.0) and int(r[(at[10], 4)]["count"]) == 4
    assert _bits(r[(at[10], 5)]["sum"]) == _bits(0.0)


def test_validation(A, ctx):
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
    outside = [(0, 3 * n), (4 * n, 4 * n), (3 * n - 10, 10), (5 * n + 3, 100), (0, 0), (3 * n + 5, 0)]
    _check(good, outside, _host(ctx, bad, outside), "outside")
    lib = A.capi.lib()
    bb = np.frombuffer(bad, dtype=np.uint8)
    gb = np.frombuffer(recs, dtype=np.uint8)

    def raw(buf, wins):
        out = np.full(max(len(wins), 1), 0, dtype=A.WINDOW_STATS)
        out["sum"] = 7.0
        b = np.array([w[0] for w in wins], dtype=np.uint64)
        c = np.array([w[1] for w in wins], dtype=np.uint64)
        p = C.POINTER(C.c_uint64)
        rc = lib.atsc_aggregate_windows(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), len(buf), 0, len(wins),
                                        b.ctypes.data_as(p), c.ctypes.data_as(p), C.c_void_p(out.ctypes.data))
        return rc, out

    for wins in ([(3 * n, 1)], [(0, nf * n)], [(0, 10), (3 * n - 1, 2)], [(4 * n - 1, 1), (6 * n, 5)]):
        rc, out = raw(bb, wins)
        assert rc == A.capi.E_FORMAT and np.all(out["sum"] == 7.0), (wins, rc)
    for wins in ([(nf * n - 2, 4)], [(0, 5), (nf * n + 1, 0)], [(2 ** 63, 2 ** 63)]):
        rc, out = raw(gb, wins)
        assert rc == A.capi.E_INVALID and np.all(out["sum"] == 7.0), (wins, rc)
    rc, _ = raw(gb, [])
    assert rc == 0
    e = _host(ctx, recs, [(5, 0), (nf * n, 0)])
    assert np.all(e["count"] == 0) and np.all(np.isnan(e["first"])) and np.all(e["sum"] == 0.0)
    assert len(_host(ctx, recs, [])) == 0


def test_entry_points_agree(A, ctx, torch, oracle, golden_dir):
    rng = np.random.default_rng(37)
    for name in ("go_gc_heap_goal_bytes", "memory_used", "uptime"):
        x = H.read_wbro(os.path.join(golden_dir, "wbros", name + ".wbro"))
        for comp, err in ((oracle.AUTO, 3), (oracle.FFT, 1), (oracle.POLYNOMIAL, 5), (oracle.RLE, 0), (oracle.NOOP, 0)):
            bro = oracle.compress_data(x, comp, err)
            full = A.decompress_data(ctx, bro)
            _, frames = H.parse_bro(bro)
            lens = [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in frames]
            wins = _windows(lens, len(full), rng, n_random=15)
            b = [w[0] for w in wins]
            c = [w[1] for w in wins]
            via_bro = A.aggregate_data_windows(ctx, bro, b, c)
            _check(full, wins, via_bro, name)
            records = bro[9:]  # with the frame-count varint
            assert _same(ctx.aggregate_windows_host(records, b, c, has_count=True), via_bro), (name, comp)
            s = A.CompressedStream.from_bytes(ctx, bro)
            assert _same(s.aggregate_windows(b, c), via_bro), (name, comp)
            n0, p0 = H.varint_decode(bro, 9)
            assert n0 == len(frames)
            assert _same(_dev(A, ctx, torch, bro[p0:], wins), via_bro), (name, comp)


def test_scale_many_pieces(A, ctx, torch):
    n = (1 << 26) + 12345
    x = H.synth_series(515, n, block=65536)
    bro = A.compress_data(ctx, x, A.AUTO, 3)
    full = A.decompress_data(ctx, bro)
    assert len(full) == n
    ctx.set_aggregate_scratch(64 << 20)
    try:
        whole = A.aggregate_data_windows(ctx, bro, [0], [n])
        bb, bc = A.bucket_windows(0, n, 100000)
        buckets = A.aggregate_data_windows(ctx, bro, bb, bc)
    finally:
        ctx.set_aggregate_scratch(0)
    assert n > 8 * ((64 << 20) // 8)  # at least 8 pieces under the budget
    _check(full, [(0, n)], whole, "whole")
    wins = list(zip(bb.tolist(), bc.tolist()))
    _check(full, wins, buckets, "buckets")
    assert _same(A.aggregate_data_windows(ctx, bro, [0], [n]), whole)  # default budget: fewer pieces, same bytes


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def _rows(path):
    lines = open(path).read().split("\n")
    return lines[0], [l.split(",") for l in lines[1:] if l]


def _row_bits(r):
    return [int(r[1])] + [_bits(float(v)) for v in r[2:]]


def _rec_bits(s):
    return [int(s["count"])] + [_bits(s[k]) for k in ("min", "max", "sum", "first", "last")]


def test_command_lines(A, ctx, golden_dir, tmp_path):
    from oracle import vsri_oracle as VO

    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    for extra, (b0, c0) in (((), (0, len(full))), (("--samples", "100:1500"), (100, 1500))):
        for nb in (60, 1000, len(full) + 1):
            _run(atsc, "-u", "--buckets", nb, *extra, tmp_path / "uptime.bro")
            head, rows = _rows(tmp_path / "uptime.agg.csv")
            assert head == "begin,count,min,max,sum,first,last"
            bb, bc = A.bucket_windows(b0, c0, nb)
            want = A.aggregate_data_windows(ctx, bro, bb, bc)
            assert [int(r[0]) for r in rows] == bb.tolist()
            assert [_row_bits(r) for r in rows] == [_rec_bits(s) for s in want], (extra, nb)
    for bad in (("-u", "--buckets", "0"), ("--buckets", "5"), ("-u", "--buckets", "x")):
        r = subprocess.run([atsc, *bad, str(tmp_path / "uptime.bro")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2, bad
    # csv-compressor -u --from --to --step on the reference's cpu_utilization values and times
    lines = open(os.path.join(golden_dir, "csv", "cpu_utilization.csv")).read().split("\n")[1:]
    rows = [l.split(",") for l in lines if l]
    ts = [int(t) * 1000 for t, _ in rows]
    vals = [float(v) for _, v in rows]
    m = tmp_path / "cpu.csv"
    m.write_text(VO.samples_to_csv_text(ts, vals))
    _run(csvc, "--output-vsri", "--compressor", "fft", "-e", "3", m)
    _run(csvc, "-u", "-o", tmp_path / "all", tmp_path / "cpu.bro")
    all_rows = [r for r in (tmp_path / "all.csv").read_text().split("\n")[1:] if r]
    all_vals = A.wbro_read(tmp_path / "all.wbro")
    times = np.array([int(r.split(",")[0]) for r in all_rows])
    cbro = (tmp_path / "cpu.bro").read_bytes()
    index = A.Vsri.load(str(tmp_path / "cpu.vsri"))
    for t0, t1, step in ((times[0], times[-1], 600), (times[10], times[50], 7), (times[10] + 1, times[50] - 1, 60),
                         (times[0] - 1000, times[3], 100), (times[-1] - 50, times[-1] + 500, 1000)):
        for f in tmp_path.glob("win*"):
            f.unlink()
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.agg.csv"]
        head, got = _rows(tmp_path / "win.agg.csv")
        assert head == "timestamp,count,min,max,sum,first,last"
        wb, wc = index.step_windows(int(t0), int(t1), int(step))
        assert [int(r[0]) for r in got] == list(range(int(t0), int(t1) + 1, int(step)))
        want = A.aggregate_data_windows(ctx, cbro, wb, wc)
        assert [_row_bits(r) for r in got] == [_rec_bits(s) for s in want], (t0, t1, step)
        for r, b, c in zip(got, wb.tolist(), wc.tolist()):
            a = int(r[0])
            sel = (times >= a) & (times <= min(a + step - 1, t1))
            v = all_vals[sel]
            assert int(sel.sum()) == c and (c == 0 or np.array_equal(v, all_vals[b:b + c])), (t0, t1, step, a)
            n, mn, mx, s, first, last = M.window_stats(all_vals, b, c)
            assert _row_bits(r) == [n] + [_bits(q) for q in (mn, mx, s, first, last)], (t0, t1, step, a)
    r = subprocess.run([csvc, "-u", "--step", "5", str(tmp_path / "cpu.bro")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2
