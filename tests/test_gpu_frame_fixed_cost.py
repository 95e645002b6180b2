"""k_compress's fixed cost at a frame's start and end, fixed-length one-wavefront kernels (128, 256, 512 samples): the
few-runs RLE records built from the run-start flags the samples left in registers (and, at an odd sample offset, by the
walk over LDS), the sorted record a lane keeps from the sizing to the emitter when a ladder overwrites the records in
between, the FFT emitter without the offset scan (one-byte positions) and with it (512 samples, a bin at 251 or above),
and the payload assembled in LDS and stored in 16-byte pieces -- each batch held against the oracle through
tests/parity.py, against the table-driven instantiation, and through the cost-ordered chained entry point."""
import functools

import numpy as np
import pytest

from tests import extreme_cases as X
from tests import parity as P

pytestmark = pytest.mark.gpu

ME5 = float(np.float32(5) / np.float32(100))
LENGTHS = (128, 256, 512)
FFT_FIRST = {128: 1 + 1 + 9 * 3 + 8, 256: 1 + 1 + 9 * 3 + 8, 512: 1 + 1 + 9 * 5 + 8}  # payload of the ladder's first trip
FFT_CAP = {128: 25, 256: 25, 512: 44}  # bins after the ladder's 23rd trip: mf + 17 dk1 + 5 dk2


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    c = atsc_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def A():
    import atsc_amd

    return atsc_amd


def _fetch(outs):
    rec_off = outs["rec_off"].cpu().numpy().astype(np.uint64)
    total = int(rec_off[-1])
    return (outs["body"][:total].cpu().numpy().tobytes(), rec_off, outs["chosen"].cpu().numpy().copy(),
            outs["err"].cpu().numpy().copy())


class _DeviceCalls:
    """What parity.compare_batch asks of a context, answered through a plan and the device-pointer entry point: the
    frames' sample offsets are then the caller's own (the host-pointer entry point rebases them to zero)."""

    def __init__(self, ctx):
        self._ctx = ctx

    def enable_diag(self, on):
        self._ctx.enable_diag(on)

    def compress_host(self, x, off, compressor, bounded, me, level):
        import torch

        dev = torch.device("cuda:0")
        plan = self._ctx.plan(off)
        try:
            d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
            outs = plan.alloc_outputs(torch, dev)
            plan.compress(d_x, outs, compressor, bounded, me, level, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return _fetch(outs)
        finally:
            plan.close()


def _exact(s, nf, what):
    """Every frame byte-identical to the oracle's."""
    print(what, "exact=%d tol=%d tie=%r boundary=%r fail=%r codecs=%r" % (
        s["exact"], s["tol"], s["tie_frames"], s["boundary_frames"], s["fail"][:4], s["codecs"]))
    assert not s["fail"], (what, s["fail"][:4])
    assert s["exact"] == nf, (what, s["exact"], s["tol"], s["tie_frames"], s["boundary_frames"])


# ---- run-length frames ------------------------------------------------------------------------------------------
# level sets: integers of each bit depth (u8, i16, i32, beyond i32 = f64) and fractional ones
LEVELS = {
    "u8": lambda k: float((k % 2) * 180 + 4 * k + 3),
    "i16": lambda k: float(((-1) ** k) * (300 + 977 * k)),
    "i32": lambda k: float(((-1) ** k) * (70000 + 1234567 * k)),
    "f64int": lambda k: float(((-1) ** k) * (3000000000 + 1000000003 * k)),
    "frac": lambda k: ((-1) ** k) * (1000.5 + 370.25 * k + 0.001 * (k % 7)),
}


def _starts(n, r, seed):
    """r run starts: 0, then sample 1, an odd and an even index inside a lane's pair (37, 60), both sides of every chunk
    wrap (128 m: lane 63 of one chunk to lane 0 of the next), 251 (the index varint widens), then seeded others."""
    must = [0, 1, 37, 60] + [j for m in range(1, n // 128) for j in (128 * m, 128 * m + 1)] + ([251] if n > 251 else [])
    rng = np.random.default_rng(seed)
    rest = [int(j) for j in rng.permutation(np.arange(2, n)) if int(j) not in must]
    return sorted((must + rest)[:r])


def _staircase(n, starts, level, repeat=0):
    """Runs from `starts`; run k takes level(k), or, with repeat = p > 0, level(k % p): values come back, groups form."""
    x = np.empty(n, dtype=np.float64)
    ends = list(starts[1:]) + [n]
    for k, (a, b) in enumerate(zip(starts, ends)):
        x[a:b] = level(k % repeat if repeat else k)
    return x


def _runs_of(f):
    return int(np.count_nonzero(f[1:] != f[:-1])) + 1


@functools.lru_cache(maxsize=None)
def _few_runs_batch(n):
    fr = []
    for name, level in LEVELS.items():
        fr.append(np.full(n, level(3)))                                   # 1 run
        for r in (15, 16, 17):
            fr.append(_staircase(n, _starts(n, r, 100 + r), level))        # all values distinct
            fr.append(_staircase(n, _starts(n, r, 200 + r), level, 5))     # five values, repeated
    # two runs, the one boundary at each of the marked places
    for k, b in enumerate(sorted(set(_starts(n, 64, 1)[1:8] + [n - 1]))):
        fr.append(_staircase(n, [0, b], list(LEVELS.values())[k % len(LEVELS)]))
    assert len(fr) <= 96
    return tuple(fr)


@pytest.mark.parametrize("n", LENGTHS)
def test_few_runs_from_register_flags(ctx, A, oracle, n):
    fr = _few_runs_batch(n)
    runs = sorted(set(_runs_of(f) for f in fr))
    assert runs == [1, 2, 15, 16, 17], runs
    x, off = X.pack(list(fr))
    s = P.compare_batch(oracle, ctx, x, off, A.AUTO, True, ME5)
    _exact(s, len(fr), "few runs n=%d" % n)
    assert s["codecs"].get(A.RLE, 0) == len(fr) - len(LEVELS), s["codecs"]  # (1 run: Constant)


@pytest.mark.parametrize("n", LENGTHS)
def test_few_runs_at_an_odd_sample_offset(ctx, A, oracle, n):
    """The same batch one sample into the caller's buffer: no statistics or flags from registers, the walk over LDS."""
    fr = _few_runs_batch(n)
    x, off = X.pack(list(fr))
    x1 = np.concatenate([[12345.678], x])
    off1 = (off + np.uint64(1)).astype(np.uint64)
    assert int(off1[0]) == 1
    s = P.compare_batch(oracle, _DeviceCalls(ctx), x1, off1, A.AUTO, True, ME5)
    _exact(s, len(fr), "few runs, odd offset n=%d" % n)


@functools.lru_cache(maxsize=None)
def _rebuilt_batch(n):
    """At most 16 runs of far-apart integer levels, u8 and i16: the polynomial's first payload (4 .. 7 points) is smaller
    than the FFT's and the RLE's, so its first trip runs, in AB, over the sorted run records -- and fails: a spline
    through a few points of a staircase of jumps.  RLE then wins and is emitted after the overwrite."""
    u8 = lambda k: float((k % 2) * 200 + 3 * k + 5)
    i16 = lambda k: float(((-1) ** k) * (2000 + 400 * k))
    fr = []
    for r in (10, 13, 16):
        fr.append(_staircase(n, _starts(n, r, 300 + r), u8))
        fr.append(_staircase(n, _starts(n, r, 400 + r), i16))
        fr.append(_staircase(n, _starts(n, r, 500 + r), u8, 6))
    return tuple(fr)


@pytest.mark.parametrize("n", LENGTHS)
def test_few_runs_emitted_after_a_ladder_overwrote_the_records(ctx, A, oracle, n):
    fr = _rebuilt_batch(n)
    for f in fr:
        assert _runs_of(f) <= 16
        first = len(oracle.polynomial(f))          # the ladder's first trip stores the baseline points
        _, _, trips = oracle.polynomial_allowed_error(f, ME5)
        payload, chosen, _ = oracle.compress_best(f, ME5, 0)
        assert first < FFT_FIRST[n] and first <= len(payload), (first, len(payload))  # the polynomial goes first, unpruned
        assert trips >= 2, trips                   # ... and its first trip fails at the bound
        assert chosen == A.RLE
    x, off = X.pack(list(fr))
    s = P.compare_batch(oracle, ctx, x, off, A.AUTO, True, ME5)
    _exact(s, len(fr), "rebuilt at emit n=%d" % n)


# ---- FFT frames ---------------------------------------------------------------------------------------------------
def _tones(n, base, amps, bins, L):
    j = np.arange(n, dtype=np.float64)
    x = np.full(n, float(base))
    for k, (a, b) in enumerate(zip(amps, bins)):
        x += a * np.sin(2.0 * np.pi * b * j / L + 0.7 * k)
    return x


@functools.lru_cache(maxsize=None)
def _fft_batch(n):
    """Frames whose FFT wins at the ladder's first trip (two or three tones well inside the bound) and frames that take
    all 23 trips (a long row of tones, each 15 % below the one before, scaled so that the error passes at the cap
    only); at 512 samples also tones at bin 260 and above, whose positions take a three-byte varint."""
    L = {128: 144, 256: 288, 512: 576}[n]
    fr = [_tones(n, 1000.0, (30.0, 20.0), (5, 11), L),
          _tones(n, 1000.0, (40.0, 25.0, 15.0), (3, 17, 29), L),
          _tones(n, -500.0, (12.0, 9.0), (7, 23), L),
          _tones(n, 2000.0, (70.0, 50.0), (2, 9), L)]
    if n == 512:  # (the first trip takes five bins: four tones, so that no leakage bin is among them)
        fr = [_tones(n, 1000.0, (30.0, 22.0, 16.0, 11.0), (5, 11, 40, 71), L),
              _tones(n, 1000.0, (40.0, 25.0, 15.0, 10.0), (3, 17, 29, 90), L),
              _tones(n, -500.0, (12.0, 9.0, 7.0, 5.0), (7, 23, 55, 120), L),
              _tones(n, 2000.0, (70.0, 50.0, 35.0, 25.0), (2, 9, 33, 64), L),
              _tones(n, 1000.0, (30.0, 20.0, 14.0, 10.0), (260, 11, 100, 30), L),
              _tones(n, 1000.0, (40.0, 30.0, 22.0, 16.0), (255, 270, 283, 60), L)]
    for scale, seed in CAP_FRAMES[n]:
        fr.append(_cap_frame(n, scale, seed))
    return tuple(fr)


def _cap_frame(n, scale, seed):
    L = {128: 144, 256: 288, 512: 576}[n]
    cap = FFT_CAP[n]
    rng = np.random.default_rng(seed)
    bins = rng.permutation(np.arange(2, L // 2 - 2))[: cap + 12]
    amps = scale * (0.9 if n == 512 else 0.85) ** np.arange(len(bins))
    return _tones(n, 1000.0, amps, bins, L)


# (scale, seed) of the frames that walk to the cap: found on the CPU with the oracle (the first scale, in steps of
# 0.5 %, at which the ladder stops with FFT_CAP bins and every decision value is clear of its threshold).  512 samples:
# 44 tones 10 % apart span two decades and the weakest drown in the pad's leakage; no such frame was found.
CAP_FRAMES = {128: ((259.64845247443367, 3),), 256: ((187.7550921055645, 3),), 512: ()}


def _clear_of_ties_and_thresholds(oracle, f):
    """On the CPU: neither candidate's error sits next to a decision threshold, and no two of the stored bins' norms
    are close (1e-4 of the largest; parity's tie verdict takes 4e-6)."""
    payload, e_fft, _ = oracle.fft_allowed_error(f, ME5)
    _, e_poly, _ = oracle.polynomial_allowed_error(f, ME5)
    assert not P._near_threshold(e_fft, ME5) and not P._near_threshold(e_poly, ME5), (e_fft, e_poly)
    from tests import helpers as H

    freqs = H.parse_fft_payload(payload)[0]
    norms = np.sort(np.array([np.hypot(r, i) for _, r, i in freqs]))
    assert len(norms) < 2 or np.min(np.diff(norms)) > 1e-4 * norms[-1], norms
    return freqs


@pytest.mark.parametrize("n", LENGTHS)
def test_fft_emit(ctx, A, oracle, n):
    fr = _fft_batch(n)
    ks = []
    for f in fr:
        freqs = _clear_of_ties_and_thresholds(oracle, f)
        _, chosen, _ = oracle.compress_best(f, ME5, 0)
        assert chosen == A.FFT
        ks.append(len(freqs))
    mf = 5 if n == 512 else 3
    assert ks.count(mf) >= 4 and ks.count(FFT_CAP[n]) >= len(CAP_FRAMES[n]) >= (0 if n == 512 else 1), ks
    if n == 512:
        from tests import helpers as H

        assert any(p >= 251 for f in fr for p, _, _ in H.parse_fft_payload(oracle.fft_allowed_error(f, ME5)[0])[0])
    x, off = X.pack(list(fr))
    s = P.compare_batch(oracle, ctx, x, off, A.AUTO, True, ME5)
    print(P.assert_summary(s, len(fr), "fft emit n=%d K=%r" % (n, ks)))
    assert not s["tie_frames"] and not s["boundary_frames"]


# ---- polynomial frames --------------------------------------------------------------------------------------------
WAVE_SEEDS = {128: (1,), 256: (1, 2), 512: (1, 18)}


def _waves(n, seed, depth_scale):
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.float64)
    x = np.full(n, 128.0)
    for p, ph in zip(rng.uniform(14, 40, 10), rng.uniform(0, 6.28, 10)):
        x += 9.0 * np.sin(2 * np.pi * j / p + ph)
    return np.floor(depth_scale * x)


@functools.lru_cache(maxsize=None)
def _poly_batch(n):
    j = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(77 + n)
    fr = []
    # smooth integer ramps: the ladder's first trips (a handful of points), at the u8, i16, i32 and f64 depths
    fr.append(np.floor(10.0 + 200.0 * j / n))
    fr.append(np.floor(-3000.0 + 9000.0 * j / n))
    fr.append(np.floor(-3000000.0 + 9000000.0 * j / n))
    fr.append(np.floor(5.0e9 + 9.0e9 * j / n))
    fr.append(1000.0 + 300.0 * j / n + 0.25)
    # ten slow waves (periods of 14 .. 40 samples) around 128: too many bins for the FFT, and a spline needs a point
    # every four samples -- more than 64 points (seeds found on the CPU with the oracle), at the u8 and wider depths
    for seed in WAVE_SEEDS[n]:
        for depth_scale in (1.0, 100.0, 100000.0):
            fr.append(_waves(n, seed, depth_scale))
    # the ladder's last resort, every sample stored: fractional noise around zero
    fr.append(rng.standard_normal(n) * 10.0)
    fr.append(rng.standard_normal(n) * 1.0e-3 + 0.5e-3)
    return tuple(fr)


@pytest.mark.parametrize("n", LENGTHS)
def test_polynomial_emit(ctx, A, oracle, n):
    """Winners of a handful of points, of more than 64 and of all n (the largest payload there is, 8 n + 22 bytes: the
    staging region holds it at every length, so there is no frame that would take another path)."""
    from tests import helpers as H

    fr = _poly_batch(n)
    ks, depths = [], set()
    for f in fr:
        payload, chosen, err = oracle.compress_best(f, ME5, 0)
        if chosen == A.POLYNOMIAL:
            p = H.parse_poly_payload(payload)
            ks.append(p["npoints"])
            depths.add(p["bitdepth"])
            if p["npoints"] == n:
                assert err == 0.0
    print("polynomial winners n=%d: points %r depths %r" % (n, ks, sorted(depths)))
    assert min(ks) <= 8 and (n == 128 or any(64 < k < n for k in ks)) and n in ks, ks  # (128: 65 points never win)
    assert depths == {0, 1, 2, 3}, depths
    x, off = X.pack(list(fr))
    s = P.compare_batch(oracle, ctx, x, off, A.AUTO, True, ME5)
    # (a polynomial payload that differs from the oracle's by a byte is a failure; the FFT winners among the frames
    # are held to parity's bars)
    print(P.assert_summary(s, len(fr), "polynomial emit n=%d" % n))
    assert not s["tie_frames"] and not s["boundary_frames"]
    assert s["codecs"].get(A.POLYNOMIAL, 0) == len(ks), (s["codecs"], ks)
    assert s["exact"] >= len(ks)


# ---- the same batches through the table-driven kernel, and in cost order --------------------------------------------
def _all_batches(n):
    return list(_few_runs_batch(n)) + list(_rebuilt_batch(n)) + list(_fft_batch(n)) + list(_poly_batch(n))


@pytest.mark.parametrize("n", LENGTHS)
def test_fixed_against_generic(ctx, A, monkeypatch, n):
    """ATSC_NO_UNIFORM forces the table-driven instantiation, as test_fixed_length_instantiation_matches_generic does:
    same bytes, same codecs, same errors."""
    import torch

    dev = torch.device("cuda", 0)
    ctx.enable_diag(False)
    x, off = X.pack(_all_batches(n))
    d_x = torch.from_numpy(x).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    got = []
    for generic in (False, True):
        if generic:
            monkeypatch.setenv("ATSC_NO_UNIFORM", "1")
        plan = ctx.plan(off)
        o = plan.alloc_outputs(torch, dev)
        plan.compress(d_x, o, A.AUTO, True, ME5, 0, stream)
        torch.cuda.synchronize()
        got.append(_fetch(o))
        plan.close()
    assert got[0][0] == got[1][0]
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])
    assert np.array_equal(got[0][3], got[1][3], equal_nan=True)


def test_adaptive_order_is_positional(ctx, A):
    """Cost order through the chained entry point: the second call walks the class in the order of ids[]; every
    result still sits at its frame's own position."""
    import torch

    dev = torch.device("cuda:0")
    x, off = X.pack(_all_batches(256))
    st = torch.cuda.current_stream().cuda_stream
    plan = ctx.plan(off)
    try:
        d_x = torch.from_numpy(x).to(dev)
        o = plan.alloc_outputs(torch, dev)
        plan.compress(d_x, o, A.AUTO, True, ME5, 0, st)
        torch.cuda.synchronize()
        ref = _fetch(o)
        ctx.set_adaptive_order(True)
        ctx.set_chains(1)  # one chain: the second call finds the clocks the first one left
        outs = [plan.alloc_outputs(torch, dev) for _ in range(3)]
        for q in outs:
            plan.compress(d_x, q, A.AUTO, True, ME5, 0, st, pipelined=True)
            plan.join(st)
            torch.cuda.synchronize()
        for k, q in enumerate(outs):
            got = _fetch(q)
            assert got[0] == ref[0], "cost-ordered call %d: bytes differ" % k
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3], equal_nan=True)
    finally:
        ctx.set_adaptive_order(False)
        ctx.set_chains(2)
        plan.close()
