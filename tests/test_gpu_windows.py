"""Window decode on the GPU: samples [begin, begin + count) of a stream, bit for bit the slice of the full decode
(compared as uint64), over every codec, frame-length tier and decoder path; foreign streams; batches against single
calls; frames outside a window are not decoded; the stream / .bro entry points and both command lines."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as H

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


def _rec(n, tag, payload):
    def v(x):
        if x < 251:
            return bytes([x])
        if x < 1 << 16:
            return b"\xfb" + struct.pack("<H", x)
        return b"\xfc" + struct.pack("<I", x)
    return v(41) + v(n) + v(tag) + v(len(payload)) + payload


def _fft_record(rng, n, k):
    """a hand-built FFT record of n samples with k stored bins (positions below n / 2, so below L / 2)"""
    p = bytes([15]) + bytes([k])
    for pos in rng.choice(np.arange(1, n // 2), size=k, replace=False):
        pos = int(pos)
        p += (bytes([pos]) if pos < 251 else b"\xfb" + struct.pack("<H", pos))
        p += struct.pack("<ff", *rng.normal(0, 50 * n, 2).astype(np.float32))
    p += struct.pack("<ff", 400.0, -400.0)
    return _rec(n, 1, p)


@pytest.fixture(scope="module")
def mixed(A, ctx):
    """one stream: every frame length of LENS under auto at e = 5 / 1 / 0 % and forced fft, polynomial, idw, rle,
    constant, noop; hand-built FFT records with 15 and 16 bins; a run of FFT frames for the large grid path"""
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
    """FFT frames of the chunker's power-of-two lengths only (the large decoder's grid path)"""
    lens = [131072, 65536, 131072, 131072]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    x = H.synth_series(808, int(off[-1]), klass=1)
    r, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.01)), 0)
    return r


def _frame_lens(A, ctx, recs):
    return [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in H.parse_bro_body(recs, with_count=False)]


def _windows(lens, total, rng, n_random=300):
    w = {(0, total), (0, 0), (total, 0), (total - 1, 1)}
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


def _eq(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _batch(A, ctx, torch, recs, wins, out_off=None):
    dp = A.DPlan(ctx, recs)
    body = torch.from_numpy(np.frombuffer(recs, dtype=np.uint8).copy()).to("cuda")
    begins = np.array([w[0] for w in wins], dtype=np.uint64)
    counts = np.array([w[1] for w in wins], dtype=np.uint64)
    if out_off is None:
        out_off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    total = int(max((int(o) + int(c) for o, c in zip(out_off, counts)), default=0))
    d_out = torch.full((max(total, 1),), float("nan"), dtype=torch.float64, device="cuda")
    dp.decompress_windows(body, begins, counts, d_out, out_off, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    dp.close()
    return [out[int(o):int(o) + int(c)] for o, c in zip(out_off, counts)]


@pytest.mark.parametrize("which", ["mixed", "grid"])
def test_windows_bit_identical_to_full_decode(A, ctx, torch, mixed, grid, which):
    recs = mixed if which == "mixed" else grid
    full = ctx.decompress_host(recs)
    lens = _frame_lens(A, ctx, recs)
    assert sum(lens) == len(full)
    wins = _windows(lens, len(full), np.random.default_rng(17))
    for b, c in wins:
        got = ctx.decompress_window_host(recs, b, c)
        assert len(got) == c and _eq(got, full[b:b + c]), (which, b, c)
    for (b, c), got in zip(wins, _batch(A, ctx, torch, recs, wins)):
        assert _eq(got, full[b:b + c]), (which, "batch", b, c)


def test_foreign_streams(A, ctx, oracle, golden_dir):
    rng = np.random.default_rng(23)
    for name in ("go_gc_heap_goal_bytes", "memory_used", "uptime"):
        x = H.read_wbro(os.path.join(golden_dir, "wbros", name + ".wbro"))
        for comp, err in ((oracle.AUTO, 3), (oracle.FFT, 1), (oracle.POLYNOMIAL, 5), (oracle.IDW, 5),
                          (oracle.RLE, 0), (oracle.NOOP, 0), (oracle.CONSTANT, 0)):
            bro = oracle.compress_data(x, comp, err)
            full = A.decompress_data(ctx, bro)
            ref = oracle.decompress_data(bro)
            assert len(full) == len(ref)
            if comp in (oracle.RLE, oracle.NOOP, oracle.CONSTANT, oracle.POLYNOMIAL):
                assert _eq(full, ref), (name, comp)
            else:
                assert np.allclose(full, ref, rtol=1e-4, atol=1e-2), (name, comp)
            _, frames = H.parse_bro(bro)
            lens = [f[1] if f[2] != 0 else H.varint_decode(f[3], 1)[0] for f in frames]
            for b, c in _windows(lens, len(full), rng, n_random=20):
                got = A.decompress_data_window(ctx, bro, b, c)
                assert _eq(got, full[b:b + c]), (name, comp, b, c)


def test_batch_equals_single_calls(A, ctx, torch, mixed):
    full = ctx.decompress_host(mixed)
    total = len(full)
    rng = np.random.default_rng(29)
    wins = []
    for _ in range(1000):
        c = int(rng.choice([1, 17, 300, 5000, 40000]))
        b = int(rng.integers(0, total - c + 1))
        wins.append((b, c))
    rng.shuffle(wins)
    counts = np.array([c for _, c in wins], dtype=np.uint64)
    gaps = rng.integers(0, 64, len(wins)).astype(np.uint64)
    order = rng.permutation(len(wins))  # the windows' places in d_out: not in call order, with gaps between them
    out_off = np.zeros(len(wins), dtype=np.uint64)
    at = 0
    for i in order:
        at += int(gaps[i])
        out_off[i] = at
        at += int(counts[i])
    got = _batch(A, ctx, torch, mixed, wins, out_off)
    for (b, c), g in zip(wins, got):
        single = ctx.decompress_window_host(mixed, b, c)
        assert _eq(g, single) and _eq(g, full[b:b + c]), (b, c)


def test_untouched_frames_are_not_decoded(A, ctx):
    import ctypes as C

    n, nf = 256, 8
    x = H.synth_series(909, n * nf, klass=2)
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.05)), 0)
    good = ctx.decompress_host(recs)
    frames = H.parse_bro_body(recs, with_count=False)
    # frame 3: a stored-bin count above the transform's bins; the record walk stays valid
    pos = 0
    for f in frames[:3]:
        pos += len(_rec(f[1], f[2], f[3]))
    rec3 = _rec(frames[3][1], frames[3][2], frames[3][3])
    pay = pos + len(rec3) - len(frames[3][3])
    assert recs[pay] == 15 and recs[pay + 1] < 200
    bad = bytearray(recs)
    bad[pay + 1] = 250
    bad = bytes(bad)
    with pytest.raises(A.AtscError) as e:
        ctx.decompress_host(bad)
    assert e.value.rc == A.capi.E_FORMAT
    for b, c in ((0, 3 * n), (4 * n, 4 * n), (3 * n - 10, 10), (5 * n + 3, 100)):
        assert _eq(ctx.decompress_window_host(bad, b, c), good[b:b + c]), (b, c)
    for b, c in ((3 * n, 1), (0, nf * n), (3 * n - 1, 2), (4 * n - 1, 1)):
        out = np.full(c, 7.0)
        on = C.c_uint64(12345)
        bb = np.frombuffer(bad, dtype=np.uint8)
        rc = A.capi.lib().atsc_decompress_window(ctx._h, bb.ctypes.data_as(C.POINTER(C.c_uint8)), len(bb), 0, b, c,
                                                 out.ctypes.data_as(C.POINTER(C.c_double)), c, C.byref(on))
        assert rc == A.capi.E_FORMAT and on.value == 0, (b, c, rc)
    # argument errors: nothing is written
    out = np.full(4, 7.0)
    on = C.c_uint64(12345)
    gb = np.frombuffer(recs, dtype=np.uint8)
    rc = A.capi.lib().atsc_decompress_window(ctx._h, gb.ctypes.data_as(C.POINTER(C.c_uint8)), len(gb), 0, nf * n - 2, 4,
                                             out.ctypes.data_as(C.POINTER(C.c_double)), 4, C.byref(on))
    assert rc == A.capi.E_INVALID and on.value == 0 and np.all(out == 7.0)
    rc = A.capi.lib().atsc_decompress_window(ctx._h, gb.ctypes.data_as(C.POINTER(C.c_uint8)), len(gb), 0, 0, 4,
                                             out.ctypes.data_as(C.POINTER(C.c_double)), 3, C.byref(on))
    assert rc == A.capi.E_CAPACITY and on.value == 0
    assert len(ctx.decompress_window_host(recs, 5, 0)) == 0


def test_stream_and_bro_entry_points(A, ctx):
    x = H.synth_series(4242, 300000)
    bro = A.compress_data(ctx, x, A.AUTO, 3)
    full = A.decompress_data(ctx, bro)
    s = A.CompressedStream.from_bytes(ctx, bro)
    _, frames = H.parse_bro(bro)
    lens = [f[1] for f in frames]
    assert len(set(lens)) > 1  # the chunker's framing: mixed tiers
    for b, c in _windows(lens, len(full), np.random.default_rng(31), n_random=30):
        assert _eq(s.decompress_window(b, c), full[b:b + c]), (b, c)
        assert _eq(A.decompress_data_window(ctx, bro, b, c), full[b:b + c]), (b, c)
    with pytest.raises(A.AtscError) as e:
        s.decompress_window(len(full), 1)
    assert e.value.rc == A.capi.E_INVALID


def _run(*args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stdout, r.stderr)
    return r


def test_command_lines(A, ctx, golden_dir, tmp_path):
    from oracle import vsri_oracle as VO

    bindir = os.path.join(os.path.dirname(A.__file__), "bin")
    atsc, csvc = os.path.join(bindir, "atsc"), os.path.join(bindir, "csv-compressor")
    # atsc -u --samples
    src = tmp_path / "uptime.wbro"
    src.write_bytes(open(os.path.join(golden_dir, "wbros", "uptime.wbro"), "rb").read())
    _run(atsc, "--compressor", "fft", "-e", "1", src)
    bro = (tmp_path / "uptime.bro").read_bytes()
    _run(atsc, "-u", tmp_path / "uptime.bro")
    whole = (tmp_path / "uptime.wbro").read_bytes()
    full = A.decompress_data(ctx, bro)
    assert whole == A.wbro_to_bytes(full)  # without the flag: what -u always wrote
    for b, c in ((0, len(full)), (100, 1), (2047, 2), (500, 1500), (len(full) - 1, 1), (7, 0)):
        _run(atsc, "-u", "--samples", "%d:%d" % (b, c), tmp_path / "uptime.bro")
        part = A.wbro_read(tmp_path / "uptime.wbro")
        assert _eq(part, full[b:b + c]), (b, c)
    r = subprocess.run([atsc, "-u", "--samples", "%d:1" % len(full), str(tmp_path / "uptime.bro")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    # csv-compressor -u --from / --to on the reference's cpu_utilization values and times
    lines = open(os.path.join(golden_dir, "csv", "cpu_utilization.csv")).read().split("\n")[1:]
    rows = [l.split(",") for l in lines if l]
    ts = [int(t) * 1000 for t, _ in rows]
    vals = [float(v) for _, v in rows]
    m = tmp_path / "cpu.csv"
    m.write_text(VO.samples_to_csv_text(ts, vals))
    _run(csvc, "--output-vsri", "--compressor", "fft", "-e", "3", m)
    _run(csvc, "-u", "-o", tmp_path / "all", tmp_path / "cpu.bro")
    all_rows = (tmp_path / "all.csv").read_text().split("\n")[1:]
    all_rows = [r for r in all_rows if r]
    all_vals = A.wbro_read(tmp_path / "all.wbro")
    times = [int(r.split(",")[0]) for r in all_rows]
    assert len(times) == len(vals) == len(all_vals)
    for t0, t1 in ((times[0], times[-1]), (times[10], times[50]), (times[10] + 1, times[50] - 1),
                   (times[-1], times[-1] + 100), (times[0] - 1000, times[3]), (times[-1] + 1, times[-1] + 5)):
        _run(csvc, "-u", "--from", t0, "--to", t1, "-o", tmp_path / "win", tmp_path / "cpu.bro")
        want = [r for r, t in zip(all_rows, times) if t0 <= t <= t1]
        got = (tmp_path / "win.csv").read_text().split("\n")[1:] if want else []
        if want:
            assert [r for r in got if r] == want, (t0, t1)
        sel = np.array([t0 <= t <= t1 for t in times])
        assert _eq(A.wbro_read(tmp_path / "win.wbro"), all_vals[sel]), (t0, t1)


# what each query's calls say of a null argument, of a window beyond the stream and of a misaligned result (device call)
MESSAGES = {
    "aggregate": ("aggregate_windows: null argument", "aggregate_windows: window beyond the stream",
                  "aggregate_windows: d_stats is not 8-byte aligned"),
    "moments": ("moments_windows: null argument", "moments_windows: window beyond the stream",
                "moments_windows: d_out is not 8-byte aligned"),
    "delta": ("delta_windows: null argument", "delta_windows: window beyond the stream",
              "delta_windows: d_out is not 8-byte aligned"),
    "runs": ("runs_windows: null argument", "runs_windows: window beyond the stream",
             "runs_windows: d_out is not 8-byte aligned"),
    "quantile": ("quantile_windows: null argument", "quantile_windows: window beyond the stream",
                 "quantile_windows: d_out is not 8-byte aligned"),
    "histogram": ("histogram_windows: null argument", "histogram_windows: window beyond the stream",
                  "histogram_windows: d_out is not 8-byte aligned"),
}


def test_messages_by_query(A, ctx, torch):
    """Every query's host and device call over one stream of 8 frames x 256 samples: a null argument, a window that
    ends one sample beyond the stream, a result pointer off by 4 bytes (device call) and the query's bad parameters.
    Each fails with E_INVALID and leaves exactly its message in atsc_ctx_last_error; nothing is enqueued and the
    result buffers keep their fill."""
    import ctypes as C

    n, nf = 256, 8
    x = H.synth_series(1912, n * nf, klass=2)
    off = np.arange(nf + 1, dtype=np.uint64) * n
    recs, _, _, _ = ctx.compress_host(x, off, A.FFT, True, float(np.float32(0.05)), 0)
    lib = A.capi.lib()
    gb = np.frombuffer(recs, dtype=np.uint8)
    dp = A.DPlan(ctx, recs)
    assert dp.n_samples == n * nf
    body = torch.from_numpy(gb.copy()).to("cuda")
    d_out = torch.full((64,), -1, dtype=torch.int64, device="cuda")
    h_out = np.full(512, 0xA5, dtype=np.uint8)
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)

    def f64(*v):
        a = np.array(v, dtype=np.float64)
        return a, a.ctypes.data_as(f64p)

    levels, p_levels = f64(0.5, 0.9)
    high, p_high = f64(0.5, 1.5)
    edges, p_edges = f64(0.0, 1.0, 2.0)
    desc, p_desc = f64(2.0, 1.0, 0.0)
    good = {"aggregate": (), "moments": (), "delta": (), "runs": (A.RUNS_GT, 0.0),
            "quantile": (2, p_levels, A.QUANTILE_LINEAR), "histogram": (3, p_edges, A.HIST_LEFT_CLOSED)}
    bad = {"runs": [((6, 0.0), "runs_windows: unknown op"), ((A.RUNS_GT, float("nan")), "runs_windows: limit is NaN")],
           "quantile": [((0, p_levels, A.QUANTILE_LINEAR), "quantile_windows: n_q outside [1, 64]"),
                        ((2, p_high, A.QUANTILE_LINEAR), "quantile_windows: a level is NaN or outside [0, 1]"),
                        ((2, p_levels, 9), "quantile_windows: unknown method")],
           "histogram": [((3, p_desc, A.HIST_LEFT_CLOSED), "histogram_windows: edges are not strictly ascending"),
                         ((3, p_edges, 7), "histogram_windows: unknown closed")]}
    inside = (np.array([0], dtype=np.uint64), np.array([10], dtype=np.uint64))
    beyond = (np.array([n * nf - 9], dtype=np.uint64), np.array([10], dtype=np.uint64))  # ends at n_samples + 1

    def host(q, wins, params, out):
        fn = getattr(lib, "atsc_%s_windows" % q)
        po = None if out is None else out.ctypes.data_as(fn.argtypes[-1])
        return fn(ctx._h, gb.ctypes.data_as(C.POINTER(C.c_uint8)), len(gb), 0, 1, wins[0].ctypes.data_as(u64p),
                  wins[1].ctypes.data_as(u64p), *params, po)

    def dev(q, wins, params, ptr):
        fn = getattr(lib, "atsc_%s_windows_dev" % q)
        return fn(ctx._h, dp._h, C.c_void_p(body.data_ptr()), 1, wins[0].ctypes.data_as(u64p), wins[1].ctypes.data_as(u64p),
                  *params, C.c_void_p(ptr), None)

    def failed(rc, text):
        assert rc == A.capi.E_INVALID, (rc, text)
        assert lib.atsc_ctx_last_error(ctx._h).decode() == text

    for q, (null, past, misaligned) in MESSAGES.items():
        failed(host(q, inside, good[q], None), null)
        failed(host(q, beyond, good[q], h_out), past)
        failed(dev(q, inside, good[q], 0), null)
        failed(dev(q, beyond, good[q], d_out.data_ptr()), past)
        failed(dev(q, inside, good[q], d_out.data_ptr() + 4), misaligned)
        for params, text in bad.get(q, []):
            failed(host(q, inside, params, h_out), text)
        for params, text in bad.get(q, []):
            failed(dev(q, inside, params, d_out.data_ptr()), text)
    torch.cuda.synchronize()
    assert bool((d_out == -1).all())
    assert np.all(h_out == 0xA5)
    dp.close()
