"""Windowed quantiles on the GPU: bit for bit against the NumPy model of the contract (tests/quantile_model.py) run on
the full decode, and as values against numpy.nanquantile on finite windows, over every codec and frame-length tier,
every selection tier and its thresholds, all four methods; radix-select stress data (duplicates, shared high bits,
signed zeros, subnormals, infinities, NaN); independence from the batch, the levels and the budget; validation; the
dev, host, stream and .bro entry points; both command lines; a stream of 2^26 samples."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import quantile_model as M

pytestmark = pytest.mark.gpu

LENS = [1, 7, 64, 128, 256, 300, 512, 513, 1024, 4096, 4097, 6500, 8192, 20000, 65536, 131072]
LEVELS = [0.0, 0.01, 0.25, 0.5, 0.9, 0.99, 1.0]
METHODS = [M.LINEAR, M.LOWER, M.HIGHER, M.NEAREST]
SHORT_MAX, MEDIUM_MAX = 256, 8192  # the tier thresholds (atsc_internal.h QNT_SHORT_MAX / QNT_MEDIUM_MAX)


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
    """a Constant record of n samples of `value` as it is (NaN, +-Inf, -0.0 included)"""
    r, _, _, _ = ctx.compress_host(np.full(n, 1.5), np.array([0, n], dtype=np.uint64), A.CONSTANT, False, 0.0, 0)
    assert r.endswith(struct.pack("<d", 1.5))
    return r[:-8] + struct.pack("<d", value)


def _const_records(A, ctx, values, lens, cache):
    """one Constant record per (value, length): short runs of arbitrary doubles, exactly as given"""
    out = []
    for v, n in zip(values, lens):
        n = int(n)
        if n not in cache:
            cache[n] = _const_record(A, ctx, 1.5, n)[:-8]
        out.append(cache[n] + struct.pack("<d", float(v)))
    return b"".join(out)


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


def _shapes(lens, total, rng, n_random=40):
    """windows of 0, 1, 2 samples, each tier threshold +-1, across frame boundaries, inside one frame, the whole stream"""
    w = {(0, total), (0, 0), (total, 0), (total - 1, 1), (0, 1), (0, 2), (total - 2, 2)}
    for c in (SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1, MEDIUM_MAX - 1, MEDIUM_MAX, MEDIUM_MAX + 1, 16384, 100000):
        if c <= total:
            w.add((0, c))
            w.add((total - c, c))
            b = int(rng.integers(0, total - c + 1))
            w.add((b, c))
    starts = np.cumsum(lens)[:-1]
    for s in starts[:: max(1, len(starts) // 24)]:
        s = int(s)
        for b, c in ((s - 1, 2), (s - 100, 300), (s - 3000, 9000), (s - 40, 60)):
            if 0 <= b and b + c <= total:
                w.add((b, c))
    at = 0
    for n in lens:  # inside one frame
        if n >= 20:
            w.add((at + 3, n - 6))
        at += n
    for _ in range(n_random):
        c = int(rng.choice([3, 60, 200, 1000, 5000, 30000]))
        if c <= total:
            w.add((int(rng.integers(0, total - c + 1)), c))
    return sorted(w)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _eq(got, want):
    """bit for bit; NaN compared as NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(np.all((_bits(got) == _bits(want)) | both_nan))


def _host(ctx, recs, wins, levels, method=M.LINEAR):
    return ctx.quantile_windows_host(recs, [w[0] for w in wins], [w[1] for w in wins], levels, method)


def _dev(A, ctx, torch, recs, wins, levels, method=M.LINEAR):
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    d_out = torch.full((max(len(wins), 1) * len(levels),), 7.0, dtype=torch.float64, device="cuda")
    dp.quantile_windows(body, [w[0] for w in wins], [w[1] for w in wins], levels, d_out, method,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()[: len(wins) * len(levels)].reshape(len(wins), len(levels)).copy()
    dp.close()
    return out


def _check(full, wins, levels, method, got, label=""):
    want = M.windows(full, [w[0] for w in wins], [w[1] for w in wins], levels, method)
    for i, (b, c) in enumerate(wins):
        assert _eq(got[i], want[i]), (label, b, c, method, got[i], want[i])
        v = full[b:b + c]
        v = v[~np.isnan(v)]
        if len(v) and np.all(np.isfinite(v)):
            with np.errstate(over="ignore", invalid="ignore"):
                ref = np.quantile(v, levels, method=M.METHOD_NAMES[method])
            assert np.array_equal(got[i], ref), (label, b, c, method, got[i], ref)


@pytest.mark.parametrize("which", ["mixed", "grid"])
def test_parity_with_full_decode(A, ctx, torch, mixed, grid, which):
    recs = mixed if which == "mixed" else grid
    full = ctx.decompress_host(recs)
    lens = _frame_lens(recs)
    assert sum(lens) == len(full)
    rng = np.random.default_rng(19)
    wins = _shapes(lens, len(full), rng)
    for method in METHODS:
        got = _host(ctx, recs, wins, LEVELS, method)
        _check(full, wins, LEVELS, method, got, which)
        assert _eq(_dev(A, ctx, torch, recs, wins, LEVELS, method), got), (which, method)
    # one level, and 64 levels
    q64 = np.concatenate([[0.0, 1.0, 0.5, 1.0 / 3.0], rng.random(60)])
    for levels in ([0.37], q64):
        got = _host(ctx, recs, wins, levels, M.LINEAR)
        _check(full, wins, levels, M.LINEAR, got, which)
    got = _host(ctx, recs, wins[:20], q64, M.NEAREST)
    _check(full, wins[:20], q64, M.NEAREST, got, which)


@pytest.fixture(scope="module")
def stress(A, ctx):
    """long and medium windows for the radix select: all equal, long runs of duplicates (RLE / Constant), values that
    share their top 48 bits, both signs, signed zeros, subnormals, +-Inf, NaN"""
    rng = np.random.default_rng(5)
    cache = {}
    parts = []  # (records, samples)

    def runs(values, lens):
        parts.append((_const_records(A, ctx, values, lens, cache), np.repeat(np.asarray(values, dtype=np.float64), lens)))

    # 0. shared top 48 bits: +-(1.0 + k ulp), k < 2^16, in short runs
    k = rng.integers(0, 1 << 16, 2000).astype(np.uint64)
    v = (np.float64(1.0).view(np.uint64) + k).view(np.float64)
    v[::3] *= -1.0
    runs(v, rng.integers(1, 21, len(v)))
    # 1. signed zeros, subnormals, tiny and huge values mixed, in short runs
    pool = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 1e300, -1e300, 1.0, -1.0])
    runs(pool[rng.integers(0, len(pool), 1500)], rng.integers(1, 21, 1500))
    # 2. long runs of duplicates: an RLE frame
    x = np.repeat(rng.normal(0, 10, 40).round(1), rng.integers(100, 2000, 40))
    r, _, _, _ = ctx.compress_host(x, np.array([0, len(x)], dtype=np.uint64), A.RLE, False, 0.0, 0)
    parts.append((r, x))
    # 3.. large Constant runs: 3.25, -0.0, +0.0, +Inf, -Inf, NaN, 2.0, NaN, -1.0
    for v, n in ((3.25, 50000), (-0.0, 9000), (0.0, 9000), (np.inf, 300), (-np.inf, 300), (np.nan, 20000), (2.0, 70000),
                 (np.nan, 500), (-1.0, 1)):
        runs([v], [n])
    recs = b"".join(p[0] for p in parts)
    want = np.concatenate([p[1] for p in parts])
    return recs, want, np.concatenate([[0], np.cumsum([len(p[1]) for p in parts])]).tolist()


def test_radix_select_stress(A, ctx, stress):
    recs, want, at = stress
    full = ctx.decompress_host(recs)
    assert _eq(full, want)
    total = len(full)
    L0, L1, L2 = at[1] - at[0], at[2] - at[1], at[3] - at[2]
    wins = [(at[0], L0), (at[0], L0 // 2), (at[0] + 5, 9000), (at[1], L1), (at[1] + 100, 8193), (at[1] + 7, 8192),
            (at[1] + 3, 300), (at[0], L0 + L1), (at[2], L2), (at[2] + 50, 12000),
            (at[3], 50000), (at[3] + 10, 20000), (at[3], 68000),  # all equal; ranks inside long runs
            (at[4], 18000), (at[5] - 5, 10), (at[6], 600), (at[6] - 100, 700), (at[6], 20600),  # +-0, +-Inf, NaN
            (at[8], 20000), (at[8], 10000), (at[8], 200), (at[8] - 1, 20001),  # all NaN; NaN and one -Inf
            (at[9] - 10000, 30000), (at[9], 70000), (at[9] + 69000, 1501), (at[11], 1), (0, total)]
    for method in METHODS:
        got = _host(ctx, recs, wins, LEVELS, method)
        _check(full, wins, LEVELS, method, got, "stress")
    got = _host(ctx, recs, [(at[8], 20000), (at[8], 10000), (at[8], 1)], LEVELS)
    assert np.all(np.isnan(got))
    # the signed zeros in total order: -0.0 below +0.0
    got = _host(ctx, recs, [(at[4], 18000)], [0.0, 0.49, 0.51, 1.0], M.LOWER)[0]
    assert list(_bits(got)) == list(_bits([-0.0, -0.0, 0.0, 0.0]))
    assert np.all(_host(ctx, recs, [(at[8] - 1, 20001)], LEVELS)[0] == -np.inf)


def test_independence(A, ctx, torch, mixed):
    full = ctx.decompress_host(mixed)
    total = len(full)
    rng = np.random.default_rng(29)
    probe = [(0, total), (5, 2043), (2047, 100000), (131071, 2), (total - 4097, 4097), (10, 257), (99, 8193), (3, 0)]
    probe += [(int(b), int(c)) for b, c in zip(rng.integers(0, total - 40000, 12), rng.integers(1, 40000, 12))]
    alone = np.array([_host(ctx, mixed, [w], LEVELS)[0] for w in probe])
    _check(full, probe, LEVELS, M.LINEAR, alone, "probe")
    others = []
    for _ in range(600):
        c = int(rng.choice([1, 60, 300, 2048, 9000, 40000]))
        others.append((int(rng.integers(0, total - c + 1)), c))
    batch = probe + others
    order = rng.permutation(len(batch))
    shuffled = [batch[i] for i in order]
    got = _host(ctx, mixed, shuffled, LEVELS)
    back = np.empty_like(got)
    back[order] = got
    assert _eq(back[: len(probe)], alone)
    # each level alone equals the level within the set
    for j, q in enumerate(LEVELS):
        assert _eq(_host(ctx, mixed, probe, [q])[:, 0], alone[:, j]), q
    # the least budget (pieces of 65536 samples): many overlapping pieces, spill slots across the 131072-sample frames
    fit = [i for i, w in enumerate(shuffled) if w[1] <= 65536]
    pfit = [i for i, w in enumerate(probe) if w[1] <= 65536]
    ctx.set_aggregate_scratch(1)
    try:
        small = _host(ctx, mixed, [shuffled[i] for i in fit], LEVELS)
        small_dev = _dev(A, ctx, torch, mixed, [probe[i] for i in pfit], LEVELS)
        with pytest.raises(A.AtscError) as e:
            _host(ctx, mixed, [(0, total)], LEVELS)
        assert e.value.rc == A.capi.E_CAPACITY
    finally:
        ctx.set_aggregate_scratch(0)
    assert _eq(small, got[fit])
    assert _eq(small_dev, alone[pfit])


def test_validation(A, ctx, torch):
    n, nf = 256, 8
    x = H.synth_series(909, n * nf, klass=2)
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.05)), 0)
    good = ctx.decompress_host(recs)
    lib = A.capi.lib()
    gb = np.frombuffer(recs, dtype=np.uint8)

    def raw(wins, levels, method=0, nq=None):
        q = np.ascontiguousarray(levels, dtype=np.float64)
        nq = len(q) if nq is None else nq
        out = np.full(max(len(wins) * max(nq, 1), 1), 7.0)
        b = np.array([w[0] for w in wins], dtype=np.uint64)
        c = np.array([w[1] for w in wins], dtype=np.uint64)
        p = C.POINTER(C.c_uint64)
        rc = lib.atsc_quantile_windows(ctx._h, gb.ctypes.data_as(C.POINTER(C.c_uint8)), len(gb), 0, len(wins),
                                       b.ctypes.data_as(p), c.ctypes.data_as(p), nq,
                                       q.ctypes.data_as(C.POINTER(C.c_double)), method,
                                       out.ctypes.data_as(C.POINTER(C.c_double)))
        return rc, out

    ok = [(0, 10), (300, 600)]
    for wins, levels, method, nq in (([(nf * n - 2, 4)], [0.5], 0, None), ([(0, 5), (nf * n + 1, 0)], [0.5], 0, None),
                                     ([(2 ** 63, 2 ** 63)], [0.5], 0, None), (ok, [0.5], 0, 0),
                                     (ok, np.linspace(0, 1, 65), 0, None), (ok, [0.5, np.nan], 0, None),
                                     (ok, [-0.01], 0, None), (ok, [1.0000001], 0, None), (ok, [np.inf], 0, None),
                                     (ok, [0.5], 4, None), (ok, [0.5], -1, None)):
        rc, out = raw(wins, levels, method, nq)
        assert rc == A.capi.E_INVALID and np.all(out == 7.0), (wins, levels, method, rc)
    rc, out = raw([], [0.5])
    assert rc == 0 and np.all(out == 7.0)
    rc, out = raw(ok, [0.5], 0)
    assert rc == 0
    # the dev call validates the same way and writes nothing
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(gb.copy()).to("cuda")
    d_out = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    for wins, levels, method in (([(nf * n, 1)], [0.5], 0), (ok, [2.0], 0), (ok, [0.5], 9)):
        with pytest.raises(A.AtscError) as e:
            dp.quantile_windows(body, [w[0] for w in wins], [w[1] for w in wins], levels, d_out, method)
        assert e.value.rc == A.capi.E_INVALID
    torch.cuda.synchronize()
    assert bool((d_out == 7.0).all())
    dp.close()
    # a malformed payload inside a window: ATSC_E_FORMAT, nothing written; outside every window: not looked at
    frames = H.parse_bro_body(recs, with_count=False)
    pos = sum(len(_rec(f[1], f[2], f[3])) for f in frames[:3])
    rec3 = _rec(frames[3][1], frames[3][2], frames[3][3])
    pay = pos + len(rec3) - len(frames[3][3])
    assert recs[pay] == 15 and recs[pay + 1] < 200
    bad = bytearray(recs)
    bad[pay + 1] = 250
    bad = bytes(bad)
    with pytest.raises(A.AtscError) as e:
        ctx.quantile_windows_host(bad, [3 * n], [1], [0.5])
    assert e.value.rc == A.capi.E_FORMAT
    outside = [(0, 3 * n), (4 * n, 4 * n), (0, 0)]
    _check(good, outside, LEVELS, M.LINEAR, ctx.quantile_windows_host(bad, [w[0] for w in outside],
                                                                       [w[1] for w in outside], LEVELS), "outside")
    e = ctx.quantile_windows_host(recs, [5, nf * n], [0, 0], LEVELS)
    assert e.shape == (2, len(LEVELS)) and np.all(np.isnan(e))
    assert ctx.quantile_windows_host(recs, [], [], LEVELS).shape == (0, len(LEVELS))


def test_entry_points_agree(A, ctx, torch, oracle, golden_dir):
    rng = np.random.default_rng(37)
    for name in ("go_gc_heap_goal_bytes", "memory_used", "uptime"):
        x = H.read_wbro(os.path.join(golden_dir, "wbros", name + ".wbro"))
        for comp, err in ((oracle.AUTO, 3), (oracle.FFT, 1), (oracle.RLE, 0), (oracle.NOOP, 0)):
            bro = oracle.compress_data(x, comp, err)
            full = A.decompress_data(ctx, bro)
            _, frames = H.parse_bro(bro)
            lens = [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in frames]
            wins = _shapes(lens, len(full), rng, n_random=10)
            b = [w[0] for w in wins]
            c = [w[1] for w in wins]
            via_bro = A.quantile_data_windows(ctx, bro, b, c, LEVELS, A.QUANTILE_HIGHER)
            _check(full, wins, LEVELS, M.HIGHER, via_bro, name)
            records = bro[9:]  # with the frame-count varint
            assert _eq(ctx.quantile_windows_host(records, b, c, LEVELS, A.QUANTILE_HIGHER, has_count=True), via_bro)
            s = A.CompressedStream.from_bytes(ctx, bro)
            assert _eq(s.quantile_windows(b, c, LEVELS, A.QUANTILE_HIGHER), via_bro), (name, comp)
            n0, p0 = H.varint_decode(bro, 9)
            assert _eq(_dev(A, ctx, torch, bro[p0:], wins, LEVELS, M.HIGHER), via_bro), (name, comp)


def test_scale_many_pieces(A, ctx):
    n = (1 << 26) + 12345
    x = H.synth_series(515, n, block=65536)
    bro = A.compress_data(ctx, x, A.AUTO, 3)
    full = A.decompress_data(ctx, bro)
    assert len(full) == n
    levels = [0.0, 0.5, 0.9, 0.99, 1.0]
    bb, bc = A.bucket_windows(0, n, 100000)
    ctx.set_aggregate_scratch(64 << 20)
    try:
        small = A.quantile_data_windows(ctx, bro, bb, bc, levels)
    finally:
        ctx.set_aggregate_scratch(0)
    default = A.quantile_data_windows(ctx, bro, bb, bc, levels)
    assert _eq(small, default)
    sel = list(range(0, len(bb), 37)) + [len(bb) - 1]
    _check(full, [(int(bb[i]), int(bc[i])) for i in sel], levels, M.LINEAR, default[sel], "buckets")
    # one whole-stream window: more than a default piece holds
    lib = A.capi.lib()
    b = np.frombuffer(bro, dtype=np.uint8)[9:]
    one = np.array([0], dtype=np.uint64)
    cnt = np.array([n], dtype=np.uint64)
    q = np.array(levels)
    out = np.full(len(levels), 7.0)
    p = C.POINTER(C.c_uint64)
    rc = lib.atsc_quantile_windows(ctx._h, b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), 1, 1, one.ctypes.data_as(p),
                                   cnt.ctypes.data_as(p), len(levels), q.ctypes.data_as(C.POINTER(C.c_double)), 0,
                                   out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == A.capi.E_CAPACITY and np.all(out == 7.0)
    msg = lib.atsc_ctx_last_error(ctx._h).decode()
    need = int(msg.split("budget of ")[1].split(" bytes")[0])
    assert need >= n * 8, msg
    ctx.set_aggregate_scratch(need)
    try:
        whole = A.quantile_data_windows(ctx, bro, [0], [n], levels)
    finally:
        ctx.set_aggregate_scratch(0)
    _check(full, [(0, n)], levels, M.LINEAR, whole, "whole")


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def _rows(path):
    lines = open(path).read().split("\n")
    return lines[0], [l.split(",") for l in lines[1:] if l]


def test_command_lines(A, ctx, golden_dir, tmp_path):
    from oracle import vsri_oracle as VO

    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    full = A.decompress_data(ctx, bro)
    names = ["0.5", "0.9", "0.99", "0", "1", "1e-1"]
    levels = [float(v) for v in names]
    for nb in (60, 1000):
        _run(atsc, "-u", "--buckets", nb, tmp_path / "uptime.bro")
        base_head, base_rows = _rows(tmp_path / "uptime.agg.csv")
        for method, mname in ((M.LINEAR, None), (M.NEAREST, "nearest")):
            extra = ("--quantile-method", mname) if mname else ()
            _run(atsc, "-u", "--buckets", nb, "--quantiles", ",".join(names), *extra, tmp_path / "uptime.bro")
            head, rows = _rows(tmp_path / "uptime.agg.csv")
            assert head == base_head + "," + ",".join("q" + s for s in names)
            assert [r[:7] for r in rows] == base_rows
            bb, bc = A.bucket_windows(0, len(full), nb)
            want = M.windows(full, bb, bc, levels, method)
            got = np.array([[float(v) for v in r[7:]] for r in rows])
            assert _eq(got, want), (nb, method)
    # csv-compressor -u --from --to --step --quantiles
    lines = open(os.path.join(golden_dir, "csv", "cpu_utilization.csv")).read().split("\n")[1:]
    rows = [l.split(",") for l in lines if l]
    ts = [int(t) * 1000 for t, _ in rows]
    vals = [float(v) for _, v in rows]
    m = tmp_path / "cpu.csv"
    m.write_text(VO.samples_to_csv_text(ts, vals))
    _run(csvc, "--output-vsri", "--compressor", "fft", "-e", "3", m)
    _run(csvc, "-u", "-o", tmp_path / "all", tmp_path / "cpu.bro")
    all_rows = [r for r in (tmp_path / "all.csv").read_text().split("\n")[1:] if r]
    times = np.array([int(r.split(",")[0]) for r in all_rows])
    cfull = A.decompress_data(ctx, (tmp_path / "cpu.bro").read_bytes())
    index = A.Vsri.load(str(tmp_path / "cpu.vsri"))
    for t0, t1, step in ((times[0], times[-1], 600), (times[10], times[50], 7)):
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "-o", tmp_path / "base", tmp_path / "cpu.bro")
        base_head, base_rows = _rows(tmp_path / "base.agg.csv")
        _run(csvc, "-u", "--from", t0, "--to", t1, "--step", step, "--quantiles", "0.5,0.95", "--quantile-method",
             "lower", "-o", tmp_path / "win", tmp_path / "cpu.bro")
        assert sorted(p.name for p in tmp_path.glob("win*")) == ["win.agg.csv"]
        head, got = _rows(tmp_path / "win.agg.csv")
        assert head == base_head + ",q0.5,q0.95"
        assert [r[:7] for r in got] == base_rows
        wb, wc = index.step_windows(int(t0), int(t1), int(step))
        want = M.windows(cfull, wb, wc, [0.5, 0.95], M.LOWER)
        assert _eq(np.array([[float(v) for v in r[7:]] for r in got]).reshape(want.shape), want)
        for f in tmp_path.glob("win*"):
            f.unlink()
