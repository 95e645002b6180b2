"""k_compress's frame walks: the twiddle table fetched at a frame's start (and fetched again when the RLE sizing has
used its LDS region since), the odd-offset sample path, the reciprocal weights in straight-line code with one
wavefront-wide divide side, the spread dealing's remainder by reciprocal, and the chained entry point -- each held
against the oracle through tests/parity.py on small seeded batches."""
import functools

import numpy as np
import pytest

from tests import extreme_cases as X
from tests import helpers as H
from tests import parity as P

pytestmark = pytest.mark.gpu

ME5 = float(np.float32(5) / np.float32(100))


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


def _check(s, nf, what):
    """No frame fails, and at most one frame of the batch is a `tie` or a `boundary`."""
    odd = list(s["tie_frames"]) + list(s["boundary_frames"])
    print(what, "exact=%d tol=%d tie=%r boundary=%r fail=%r codecs=%r" % (
        s["exact"], s["tol"], s["tie_frames"], s["boundary_frames"], s["fail"][:4], s["codecs"]))
    assert len(odd) <= 1, (what, odd)
    return P.assert_summary(s, nf, what, allow_tie=odd, allow_boundary=odd)


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


def _fetch(outs):
    rec_off = outs["rec_off"].cpu().numpy().astype(np.uint64)
    total = int(rec_off[-1])
    return (outs["body"][:total].cpu().numpy().tobytes(), rec_off, outs["chosen"].cpu().numpy().copy(),
            outs["err"].cpu().numpy().copy())


def _run_frame(rng, n, lo, hi):
    """lo..hi runs of distinct fractional levels, the cuts drawn without replacement."""
    r = int(rng.integers(lo, hi + 1))
    cuts = np.sort(rng.choice(np.arange(1, n), size=r - 1, replace=False)) if r > 1 else np.array([], dtype=np.int64)
    levels = 1000.0 + 300.0 * rng.standard_normal(r) + rng.random(r)
    assert len(np.unique(levels)) == r
    lens = np.diff(np.concatenate([[0], cuts, [n]]))
    return np.repeat(levels, lens).astype(np.float64)


def _noisy(rng, n):
    return 1000.0 + 300.0 * rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def _flag_batch(n):
    """48 frames whose RLE sizing (17 .. 64 runs) uses the twiddle region before the FFT candidate, and 16 each that
    leave it alone: at most 16 runs, constant, noisy.  Shuffled, so that both states meet in every stretch of the launch."""
    rng = np.random.default_rng(20260 + n)
    fr = [_run_frame(rng, n, 17, 64) for _ in range(48)]
    fr += [_run_frame(rng, n, 2, 16) for _ in range(16)]
    fr += [np.full(n, 1000.0 + 300.0 * rng.standard_normal() + rng.random()) for _ in range(16)]
    fr += [_noisy(rng, n) for _ in range(16)]
    order = rng.permutation(len(fr))
    return tuple(fr[i] for i in order)


@pytest.mark.parametrize("n", [128, 256, 512])
def test_region_overwritten_before_the_fft(ctx, A, oracle, n):
    fr = _flag_batch(n)
    runs = [int(np.count_nonzero(np.diff(f)) + 1) for f in fr]
    assert sum(1 for r in runs if 17 <= r <= 64) == 48 and sum(1 for r in runs if r == 1) == 16
    x, off = X.pack(list(fr))
    s = P.compare_batch(oracle, ctx, x, off, A.AUTO, True, ME5)
    _check(s, len(fr), "flag batch n=%d" % n)


@pytest.mark.parametrize("n", [128, 256, 512])
def test_odd_sample_offset(ctx, A, oracle, n):
    """The same batches one sample into the caller's buffer: every frame starts on an odd sample (8-byte loads, no
    statistics from registers)."""
    fr = _flag_batch(n)
    x, off = X.pack(list(fr))
    x1 = np.concatenate([[12345.678], x])
    off1 = (off + np.uint64(1)).astype(np.uint64)
    assert int(off1[0]) == 1
    s = P.compare_batch(oracle, _DeviceCalls(ctx), x1, off1, A.AUTO, True, ME5)
    _check(s, len(fr), "odd offset n=%d" % n)


SPECIALS = (0.0, 1e-300, -1e-300, -1e-310, 1e300)


def _recip_frames(n):
    """Ordinary frames with a few samples outside the fast reciprocal's range (1e-290, 1e290) at chosen (lane, slice)
    places of the padded signal -- sample i sits at j = i + pre, lane j % 64 of slice j // 64; the last sample is also
    the right pad, i.e. the lanes of the slice that runs past L -- and frames with no sample inside the range."""
    L = {256: 288, 512: 576}[n]
    pre = (L - n) // 2
    i = np.arange(n, dtype=np.float64)
    base = 1000.0 + 50.0 * np.sin(2.0 * np.pi * i / 37.0)
    last_slice = (L - 1) // 64
    fr = []
    # one special value alone, each in another lane and slice
    for k, v in enumerate(SPECIALS):
        f = base.copy()
        sl = (k * 2 + 1) % (last_slice + 1)
        lane = (11 + 13 * k) % 64
        f[min(max(sl * 64 + lane - pre, 0), n - 1)] = v
        fr.append(f)
    # several in one wavefront: different lanes, different slices, the last slice and the pads (first and last sample)
    f = base.copy()
    f[0] = -1e-310
    f[70 - pre] = 0.0
    f[64 * 2 + 5 - pre] = 1e-300
    f[64 * 3 + 40 - pre] = -1e-300
    f[n - 1] = 1e-300
    fr.append(f)
    f = base.copy()
    f[last_slice * 64 + 3 - pre] = 1e300
    f[n - 1] = 1e300
    f[33 - pre if 33 >= pre else 0] = 0.0
    fr.append(f)
    # the same lane in every slice
    f = base.copy()
    for sl in range(last_slice + 1):
        j = sl * 64 + 17
        if pre <= j < pre + n:
            f[j - pre] = (-1e-310, 1e-300, 0.0)[sl % 3]
    fr.append(f)
    # no sample inside the range
    fr.append(1e-300 * (1.0 + i / n))
    fr.append(-1e-310 * (1.0 + i))
    fr.append(1e300 * (1.0 + i / n))
    fr.append(np.where(i % 2 == 0, 1e-300, -1e-300) * (1.0 + i / n))
    # from the extreme-magnitude cases
    fr += [X.tiny_straddling(n), X.with_tiny_sample(n, 0.0, n // 3),
           X.with_tiny_sample(n, float(np.ldexp(1.0, -1060)), n // 2),
           X.with_tiny_sample(n, -float(np.ldexp(1.0, -1074)), n - 1),
           X.scaled(n, 0, -1040), X.scaled(n, 0, -1000), X.scaled(n, 0, 1000)]
    return fr


@pytest.mark.parametrize("n", [256, 512])
def test_reciprocal_paths_inside_one_wavefront(ctx, A, oracle, n):
    fr = _recip_frames(n)
    x, off = X.pack(fr)
    s = P.compare_batch(oracle, ctx, x, off, A.AUTO, True, ME5)
    _check(s, len(fr), "reciprocal paths n=%d" % n)


SPREAD_COUNTS = (4096, 4099, 6000)


@functools.lru_cache(maxsize=None)
def _spread_reference():
    """The oracle's records of 6000 distinct noisy 128-sample frames; frames are coded one by one, so a shorter batch's
    reference is a prefix."""
    from oracle import oracle as orc

    nf, n = max(SPREAD_COUNTS), 128
    x = _noisy(np.random.default_rng(4096), nf * n)
    off = H.frame_offsets(len(x), n)
    bro, chosen, _ = orc.stream_compress(x, off, orc.AUTO, True, ME5, 0)
    import atsc_amd

    body_off, cnt = atsc_amd.bro_open(bro)
    assert cnt == nf
    return x, H.parse_bro_body(bro[body_off:], with_count=False), np.asarray(chosen[:nf])


@pytest.mark.parametrize("count", SPREAD_COUNTS)
def test_spread_dealing(ctx, A, oracle, count):
    """Uniform classes of 4096 frames and more are dealt with a stride: workgroup b takes frame (b * spread) % count.
    Every frame of the batch must come out at its own place with the oracle's codec, length and bytes."""
    x, ref_frames, ref_chosen = _spread_reference()
    n = 128
    off = H.frame_offsets(count * n, n)
    rec, rec_off, chosen, _ = ctx.compress_host(x[: count * n], off, A.AUTO, True, ME5, 0)
    got = H.parse_bro_body(rec, with_count=False)
    assert len(got) == count
    wrong_codec = int(np.count_nonzero(chosen != ref_chosen[:count]))
    wrong_len = sum(1 for i in range(count) if len(got[i][3]) != len(ref_frames[i][3]))
    wrong_bytes = [i for i in range(count) if got[i] != ref_frames[i]]
    print("spread count=%d: codec differs in %d frames, length in %d, bytes in %d %r" % (
        count, wrong_codec, wrong_len, len(wrong_bytes), wrong_bytes[:8]))
    assert wrong_codec == 0 and wrong_len == 0 and not wrong_bytes


def test_pipelined_and_plain_calls_agree(ctx, A):
    """The 256-sample flag batch through the chained entry point, once per scratch set and round again, against the
    plain call's bytes."""
    import torch

    dev = torch.device("cuda:0")
    x, off = X.pack(list(_flag_batch(256)))
    st = torch.cuda.current_stream().cuda_stream
    ctx.set_chains(4)
    try:
        plan = ctx.plan(off)
        d_x = torch.from_numpy(x).to(dev)
        o = plan.alloc_outputs(torch, dev)
        plan.compress(d_x, o, A.AUTO, True, ME5, 0, st)
        torch.cuda.synchronize()
        ref = _fetch(o)
        outs = [plan.alloc_outputs(torch, dev) for _ in range(8)]
        for q in outs:
            plan.compress(d_x, q, A.AUTO, True, ME5, 0, st, pipelined=True)
        plan.join(st)
        torch.cuda.synchronize()
        for k, q in enumerate(outs):
            got = _fetch(q)
            assert got[0] == ref[0], "chained call %d: bytes differ" % k
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
        plan.close()
    finally:
        ctx.set_chains(2)
