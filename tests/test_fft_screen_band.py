"""The FFT ladder's f32 error screen ("The ladder's error screen"), modelled in numpy.

k_compress's fixed-length one-wavefront kernels decide a failing ladder trip from an f32 estimate Q of the mean
error where that estimate clears the exit threshold by more than its band B.  This file holds a numpy model of the
screen (np.float32 arithmetic, the kernel's order of operations) and of the exact f64 evaluation, runs both on the
oracle's ladder -- the bins `FFT::compress` keeps at every trip's K -- and asserts on every trip

  * |Q - cur| <= B, and
  * "certainly fails" never fires on a trip that the exact test `max_err_m < (cur * 1000) as i32` passes,
    for every max_err_m from 0 to 400 (0 % to 40 %).

No GPU: the model is the arithmetic, not the kernel; tests/test_gpu_fft_screen.py holds the kernel to the
table-driven instantiation, which has no screen."""
import math

import numpy as np
import pytest

from tests import helpers as H

F32 = np.float32
TRIPS = 23


def ladder_ks(n, bins):
    """K at every trip: fft.rs:334-352 (mf = max(3, n / 100), +mf/2 for 17 trips, +mf/10 for 5 more)."""
    mf = max(3, n // 100)
    dk1, dk2 = max(mf // 2, 1), max(mf // 10, 1)
    ks, jump = [], 0
    for trip in range(1, TRIPS + 1):
        ks.append(min(mf + jump, bins))
        jump += dk1 if trip <= 17 else dk2
    return ks


def wave_sum_f32(lane):
    """64 lane values through the six DPP steps; every step is one f32 addition per lane."""
    v = np.asarray(lane, dtype=F32)
    assert v.shape == (64,)
    while len(v) > 1:
        v = (v[0::2] + v[1::2]).astype(F32)
    return F32(v[0])


def lanes(a, L, fill):
    """Sample j = lane + 64 m of the padded signal as [m, lane]; slots beyond L hold `fill`."""
    spl = (L + 63) // 64
    out = np.full(64 * spl, fill, dtype=a.dtype)
    out[:L] = a
    return out.reshape(spl, 64)


def lane_sum_f32(terms):
    s = np.zeros(64, dtype=F32)
    for m in range(terms.shape[0]):
        s = (s + terms[m]).astype(F32)
    return wave_sum_f32(s)


class Frame:
    """What the kernel holds when the ladder starts: g, 1 / |g| (f64), the f32 clamp bounds, the screen's scalar."""

    def __init__(self, g, mnf, mxf):
        self.L = len(g)
        self.g = lanes(np.asarray(g, dtype=np.float64), self.L, 1.0)
        with np.errstate(divide="ignore"):
            inv = 1.0 / np.abs(np.asarray(g, dtype=np.float64))
        self.inv = lanes(inv, self.L, 0.0)
        self.mnf, self.mxf = F32(mnf), F32(mxf)
        self.invLf = F32(1.0) / F32(self.L)
        with np.errstate(over="ignore", invalid="ignore"):
            minv = F32(lane_sum_f32(self.inv.astype(F32)) * self.invLf)
            delta = F32(F32(5.0005e-6) + F32(F32(2.0 ** -51) * max(abs(self.mnf), abs(self.mxf))))
            self.scr_abs = F32(F32(delta * minv) + F32(2.0 ** -23))

    def limit(self, max_err_m):
        thr = F32(max(F32(max_err_m) + F32(1.0), F32(0.0)) * F32(1.0e-3)) if max_err_m < (1 << 30) else F32(np.inf)
        with np.errstate(over="ignore", invalid="ignore"):
            lim = F32(F32(self.scr_abs + thr) * F32(1.001))
        return lim if lim < F32(1e30) else F32(np.inf)

    def screen(self, v):
        """Q of the reconstruction v (f32, [m, lane])."""
        with np.errstate(over="ignore", invalid="ignore"):
            c = np.minimum(np.maximum(v, self.mnf), self.mxf).astype(F32)
            d = np.abs((c - self.g.astype(F32)).astype(F32))
            t = (d * self.inv.astype(F32)).astype(F32)
            return F32(lane_sum_f32(t) * self.invLf)

    def band(self, q):
        """B: what the kernel's compare allows for -- 1.001 scr_abs, and 2^-19 of Q for the f32 roundings."""
        return 1.001 * float(self.scr_abs) + 2.0 ** -19 * float(q)

    def certainly_fails(self, q, max_err_m):
        with np.errstate(over="ignore", invalid="ignore"):
            return bool(F32(q * F32(1.0 - 2.0 ** -18)) > self.limit(max_err_m))

    def exact(self, v):
        """fft.rs:208-218 and utils/error.rs:104-116 in f64: the kernel's exact side."""
        x5 = v.astype(np.float64) * 100000.0
        o = np.trunc(x5 + np.copysign(0.5, x5)) / 100000.0
        o = np.minimum(np.maximum(o, float(self.mnf)), float(self.mxf))
        with np.errstate(invalid="ignore", over="ignore"):
            return float(np.sum(np.abs(o - self.g) * self.inv)) / self.L, o


def sat_i32(x):
    if x != x:
        return 0
    return int(min(max(math.trunc(x), -2 ** 31), 2 ** 31 - 1)) if math.isfinite(x) else (2 ** 31 - 1 if x > 0 else -2 ** 31)


def trip_reconstructions(oracle, x):
    """-> (Frame, [v per trip]): the padded signal, and per trip the f32 inverse transform of the bins the reference
    keeps at that trip's K, summed bin by bin as the kernel does (coefficient 2 / L folded in, DC apart)."""
    n = len(x)
    g = oracle.gibbs_sizing(x)
    L = len(g)
    j = np.arange(64 * ((L + 63) // 64), dtype=np.int64).reshape(-1, 64)
    frame, acc, dc, have, out = None, None, F32(0.0), 0, []
    for K in ladder_ks(n, L // 2 + 1):
        freqs, mx, mn = H.parse_fft_payload(oracle.fft_set(x, K))
        if frame is None:
            frame = Frame(g, mn, mx)
            acc = np.zeros(j.shape, dtype=F32)
        for pos, re, im in freqs[have:]:
            cf = (1.0 if (pos == 0 or 2 * pos == L) else 2.0) / L
            a, b = F32(cf * float(re)), F32(cf * float(im))
            if pos == 0:
                dc = a
                continue
            th = 2.0 * math.pi * ((pos * j) % L) / L
            with np.errstate(over="ignore", invalid="ignore"):
                acc = (acc + (a * np.cos(th).astype(F32)).astype(F32)).astype(F32)
                acc = (acc + (-b * np.sin(th).astype(F32)).astype(F32)).astype(F32)
        have = max(have, len(freqs))
        out.append((acc + dc).astype(F32))
    return frame, out


def series():
    """(name, samples): the five synthetic classes at three scales, a sign-straddling series and one with zeros."""
    out = []
    for klass in range(5):
        base = H.synth_series(20 + klass, 4096, klass=klass)
        for scale in (1e-3, 1.0, 1e6):
            out.append(("class%d x %g" % (klass, scale), base * scale))
    osc = H.synth_series(31, 4096, klass=1) - 1000.0
    out.append(("straddling zero", osc))
    out.append(("straddling zero, small", osc * 1e-4))
    z = H.synth_series(32, 4096, klass=0).copy()
    z[::7] = 0.0
    out.append(("every seventh sample zero", z))
    return out


MS = np.arange(0, 401)


@pytest.mark.parametrize("flen", [128, 256, 512])
def test_screen_band_and_decision(oracle, flen):
    frames = trips = fired = in_band_checked = 0
    for name, x in series():
        for f in range(min(len(x) // flen, 6)):
            fx = np.ascontiguousarray(x[f * flen:(f + 1) * flen])
            if fx.min() == fx.max():
                continue  # (Constant: no ladder)
            frame, recon = trip_reconstructions(oracle, fx)
            frames += 1
            for t, v in enumerate(recon):
                cur, o = frame.exact(v)
                q = frame.screen(v)
                trips += 1
                if np.isfinite(q) and np.isfinite(frame.scr_abs):
                    assert abs(float(q) - cur) <= frame.band(q), (name, f, t, float(q), cur, frame.band(q))
                    in_band_checked += 1
                goes_on = sat_i32(cur * 1000.0)
                for m in MS:
                    if frame.certainly_fails(q, int(m)):
                        fired += 1
                        assert int(m) < goes_on, (name, f, t, int(m), float(q), cur)
                if frame.certainly_fails(q, 2 ** 31 - 1):
                    raise AssertionError("a saturating bound was screened")
            if "zero" in name and "seventh" in name:
                assert not np.isfinite(frame.scr_abs)  # a zero sample: every trip takes the exact side
    assert frames >= 60 and in_band_checked > 500 and fired > 0, (frames, trips, in_band_checked, fired)


def test_model_reconstruction_is_the_oracles(oracle):
    """The model's per-trip reconstruction, rounded and clamped, against the oracle's decode of the same payload:
    two f32 transforms, held together by the decode tests' bar."""
    for klass, n in ((0, 256), (1, 256), (1, 128), (1, 512)):
        x = H.synth_series(40 + klass, n, klass=klass)
        frame, recon = trip_reconstructions(oracle, x)
        L, pre = frame.L, (frame.L - n) // 2
        for t, K in enumerate(ladder_ks(n, L // 2 + 1)):
            if t not in (0, 5, 22):
                continue
            _, o = frame.exact(recon[t])
            ref = oracle.decompress(oracle.FFT, oracle.fft_set(x, K), n)
            got = o.reshape(-1)[pre:pre + n]
            tol = (4 + np.log2(n)) * np.max(np.abs(ref)) * 2.0 ** -23 + 1.00001e-5
            assert np.max(np.abs(got - ref)) <= tol, (klass, n, t)


def test_non_finite_and_extreme_frames_are_never_screened():
    """A NaN or zero sample makes the limit NaN or +Inf; a Q that overflows is only trusted below a finite limit."""
    g = np.linspace(1.0, 2.0, 288)
    v = lanes(np.full(288, 50.0, dtype=F32), 288, F32(0.0))
    for bad in (0.0, np.nan):
        gb = g.copy()
        gb[17] = bad
        fr = Frame(gb, 1.0, 2.0)
        assert not fr.certainly_fails(fr.screen(v), 0)
    fr = Frame(g, 1.0, 2.0)
    assert fr.certainly_fails(F32(np.inf), 50) and not fr.certainly_fails(F32(np.nan), 50)
    tiny = Frame(g * 1e-37, 1e-37, 2e-37)  # the band alone exceeds 1e30: no limit
    assert not tiny.certainly_fails(F32(np.inf), 50)
