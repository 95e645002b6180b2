"""The FFT ladder's f32 error screen in the fixed-length one-wavefront kernels (128, 256 and 512 samples; DESIGN.md
section 3, "The ladder's error screen").  The table-driven instantiation has no screen and is the in-tree reference:
body bytes, rec_off, chosen and err must be equal array for array (ATSC_NO_UNIFORM forces it, as
test_gpu_parity.py::test_fixed_length_instantiation_matches_generic does), and the fixed-length kernels are held
against the oracle through tests/parity.py.  Small batches: at most 512 frames."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import parity as P

pytestmark = pytest.mark.gpu

FLENS = [128, 256, 512]


def me_of(percent_tenths):
    """The CLI's error bound for percent_tenths / 10 percent, as the reference forms it (f32 / 100)."""
    return float(np.float32(percent_tenths / 10.0) / np.float32(100))


ME5, ME1 = me_of(50), me_of(10)


@pytest.fixture(scope="module")
def ctx():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    c = atsc_amd.Context(0)
    c.enable_diag(False)  # (a diagnostics record routes uniform batches to the table-driven kernels)
    yield c
    c.close()


@pytest.fixture(scope="module")
def A():
    import atsc_amd

    return atsc_amd


class _Device:
    """A batch resident on the device, compressed through plans over the caller's own sample offsets: one plan for the
    fixed-length kernels and one, made under ATSC_NO_UNIFORM, for the table-driven instantiation."""

    def __init__(self, ctx, monkeypatch, x, off):
        import torch

        self.torch, self.dev = torch, torch.device("cuda:0")
        self.d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(self.dev)
        monkeypatch.delenv("ATSC_NO_UNIFORM", raising=False)
        self.fixed = ctx.plan(off)
        monkeypatch.setenv("ATSC_NO_UNIFORM", "1")
        self.generic = ctx.plan(off)
        monkeypatch.delenv("ATSC_NO_UNIFORM")

    def run(self, plan, A, me):
        outs = plan.alloc_outputs(self.torch, self.dev)
        plan.compress(self.d_x, outs, A.AUTO, True, me, 0, self.torch.cuda.current_stream().cuda_stream)
        self.torch.cuda.synchronize()
        rec_off = outs["rec_off"].cpu().numpy().astype(np.uint64)
        return (outs["body"][:int(rec_off[-1])].cpu().numpy().tobytes(), rec_off, outs["chosen"].cpu().numpy().copy(),
                outs["err"].cpu().numpy().copy())

    def assert_same(self, A, me, what):
        f, g = self.run(self.fixed, A, me), self.run(self.generic, A, me)
        assert f[0] == g[0], "%s: body bytes differ" % (what,)
        assert np.array_equal(f[1], g[1]), "%s: rec_off differs" % (what,)
        assert np.array_equal(f[2], g[2]), "%s: chosen differs" % (what,)
        assert np.array_equal(f[3], g[3], equal_nan=True), "%s: err differs" % (what,)
        return f

    def close(self):
        self.fixed.close()
        self.generic.close()


class _Calls:
    """What parity.compare_batch asks of a context, answered by the fixed-length plan of a _Device."""

    def __init__(self, device, A):
        self._d, self._A = device, A

    def enable_diag(self, on):
        assert not on

    def compress_host(self, x, off, compressor, bounded, me, level):
        assert compressor == self._A.AUTO and bounded and level == 0
        return self._d.run(self._d.fixed, self._A, me)


def _check(s, nf, what):
    """No frame fails, and at most one frame of the batch is a `tie` or a `boundary`."""
    odd = list(s["tie_frames"]) + list(s["boundary_frames"])
    print(what, "exact=%d tol=%d tie=%r boundary=%r fail=%r codecs=%r" % (
        s["exact"], s["tol"], s["tie_frames"], s["boundary_frames"], s["fail"][:4], s["codecs"]))
    assert len(odd) <= 1, (what, odd)
    return P.assert_summary(s, nf, what, allow_tie=odd, allow_boundary=odd)


def _pack(frames):
    x = np.concatenate(frames)
    n = len(frames[0])
    assert all(len(f) == n for f in frames)
    return x, H.frame_offsets(len(x), n)


# ---------------------------------------------------------------------------------------
# the exit on every trip: eight class-1 frames, max_error from 0.1 % to 20 % in 0.1 % steps
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flen", FLENS)
def test_max_error_sweep(ctx, A, oracle, monkeypatch, flen):
    x = H.synth_series(61, 8 * flen, klass=1)
    off = H.frame_offsets(len(x), flen)
    d = _Device(ctx, monkeypatch, x, off)
    try:
        exits = set()
        for tenth in range(1, 201):
            me = me_of(tenth)
            d.assert_same(A, me, "sweep n=%d e=%.1f%%" % (flen, tenth / 10.0))
            s = P.compare_batch(oracle, _Calls(d, A), x, off, A.AUTO, True, me)
            _check(s, 8, "sweep n=%d e=%.1f%%" % (flen, tenth / 10.0))
            for f in range(8):
                exits.add(oracle.fft_allowed_error(x[f * flen:(f + 1) * flen], me)[2])
        print("ladder exits seen (oracle trips):", sorted(exits))
        assert exits == set(range(1, 24)), sorted(exits)  # the exit lands on every trip, the cap included
    finally:
        d.close()


# ---------------------------------------------------------------------------------------
# where the band is wide, tiny, infinite; the frame that fails at the cap
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed(flen):
    rng = np.random.default_rng(7100 + flen)
    i = np.arange(flen, dtype=np.float64)
    fr = []
    # magnitudes 1e-3 .. 1e-1 around zero: 1 / |g| is large, the band wide, nearly every trip evaluated exactly
    for k in range(24):
        amp = 10.0 ** rng.uniform(-3.0, -1.0)
        f = amp * (np.sin(2.0 * np.pi * i / rng.uniform(5.0, 60.0) + rng.uniform(0, 6.28))
                   + 0.4 * np.sin(2.0 * np.pi * i / rng.uniform(2.5, 9.0)) + 0.05 * rng.standard_normal(flen))
        fr.append(f + (amp * 0.5 if k % 3 == 0 else 0.0))
    # magnitude 1e6: a tiny band
    for k in range(16):
        fr.append(1e6 * H.synth_series(70 + k, flen, klass=k % 2))
    for k in range(8):
        fr.append(1e6 + 3e5 * rng.standard_normal(flen))
    # zeros: every seventh sample, one sample, the pads' sample
    for k in range(8):
        f = H.synth_series(90 + k, flen, klass=k % 2).copy()
        if k < 4:
            f[k::7] = 0.0
        elif k < 6:
            f[int(rng.integers(1, flen - 1))] = 0.0
        else:
            f[0 if k == 6 else flen - 1] = 0.0
        fr.append(f)
    # ordinary frames between them, the five classes
    for k in range(15):
        fr.append(H.synth_series(100 + k, flen, klass=k % 5))
    # white noise: the ladder runs all 23 trips and fails (asserted below through the oracle)
    fr.append(1000.0 + 300.0 * rng.standard_normal(flen))
    cap_frame = len(fr) - 1
    return tuple(fr), cap_frame


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "odd-offset"])
@pytest.mark.parametrize("flen", FLENS)
def test_bands_zeros_and_cap(ctx, A, oracle, monkeypatch, flen, shift):
    """shift = 1: the same batch one sample into the caller's buffer, every frame 8 bytes off a 16-byte boundary."""
    frames, cap_frame = _mixed(flen)
    x, off = _pack(list(frames))
    if shift:
        x = np.concatenate([[12345.678], x])
        off = (off + np.uint64(1)).astype(np.uint64)
    d = _Device(ctx, monkeypatch, x, off)
    try:
        for me in (ME5, ME1):
            d.assert_same(A, me, "mixed n=%d shift=%d me=%g" % (flen, shift, me))
            s = P.compare_batch(oracle, _Calls(d, A), x, off, A.AUTO, True, me)
            _check(s, len(frames), "mixed n=%d shift=%d me=%g" % (flen, shift, me))
            _, e, trips = oracle.fft_allowed_error(frames[cap_frame], me)
            assert trips == 23 and e > me, (trips, e)
            assert s["chosen"][cap_frame] != A.FFT
    finally:
        d.close()
