"""Inputs of the extreme-magnitude tests, shared by tests/test_gpu_extreme_values.py (which runs them on the GPU against
the oracle) and tests/test_extreme_values_host.py (which checks on the CPU that none of them sits next to a decision
threshold of the oracle, so that the GPU test may excuse no frame as "boundary").

Base series: helpers.synth_series(SEED, n, klass) for the smooth (0), busy (1) and run-length (3) classes, scaled by exact
powers of two (ldexp: mantissas survive, except in the subnormal range).  Why each scale is there:
   90   |x| reaches 1e30: the FFT error loop's compare-select side, the transform still finite in f32
  110   the f32 spectrum overflows; the reference reports the FFT error as NaN and the selector takes the polynomial
  126, 130   min and max both convert to f32 infinity: the 10-byte FFT payload with error 0.0
  500, 600   beyond 1e150 (the spline's compare-select side); the values are integers, so the integer bit depths saturate
  1000, 1012 x * 1e5 overflows in the 5-decimal rounding
  -20   the 5-decimal grid dominates
  -1000 tiny normal numbers
  -1030, -1040  subnormal numbers: 1 / |g| overflows
"""
import numpy as np

from tests import helpers as H

SEED = 7
KLASSES = (0, 1, 3)
SCALES = (90, 110, 126, 130, 500, 600, 1000, 1012, -20, -1000, -1030, -1040)
# one length per kernel family: one wavefront; the fixed 256 instantiation and the generic kernel; the wide fixed
# instantiations; the large tier (its fast path, and the general kernel when the fast path is switched off)
SMALL_LENGTHS = (64, 256, 300)
WIDE_LENGTHS = (1024, 4096)
LARGE_LENGTH = 8192

ME5 = float(np.float32(5) / np.float32(100))
ME1 = float(np.float32(1) / np.float32(100))
ME50 = float(np.float32(50) / np.float32(100))

# (name, compressor name, bounded, max error); an unbounded call has no error loop and no selector: its max error is not used
MODES = (
    ("auto-e5", "AUTO", True, ME5), ("auto-e1", "AUTO", True, ME1), ("auto-e50", "AUTO", True, ME50),
    ("fft-e5", "FFT", True, ME5), ("fft-e50", "FFT", True, ME50), ("fft-unbounded", "FFT", False, ME5),
    ("poly-e5", "POLYNOMIAL", True, ME5), ("poly-e50", "POLYNOMIAL", True, ME50), ("poly-unbounded", "POLYNOMIAL", False, ME5),
    ("idw-e5", "IDW", True, ME5), ("idw-e50", "IDW", True, ME50), ("idw-unbounded", "IDW", False, ME5),
)
EXACT_MODES = (("rle", "RLE", False, 0.0), ("noop", "NOOP", False, 0.0), ("constant", "CONSTANT", False, 0.0))


def scaled(n, klass, exp, seed=SEED):
    return np.ldexp(H.synth_series(seed, n, klass=klass), exp)


def straddling(n, exp, seed=SEED):
    """A frame with samples on both sides of zero at a large scale."""
    return np.ldexp(H.synth_series(seed, n, klass=0) - 1000.0, exp)


def with_tiny_sample(n, value, where, seed=SEED):
    """An ordinary frame with one zero or subnormal sample inside (some 1 / |g| is not finite)."""
    x = H.synth_series(seed, n, klass=0).copy()
    x[where] = value
    return x


def tiny_straddling(n, seed=SEED):
    """Samples on both sides of zero, all below half a step of the 5-decimal grid (every reconstruction rounds to 0, so
    every MAPE term is |0 - g| / |g| = 1), one of them subnormal: its term is 1 by the reference's division and inf by
    |0 - g| * (1 / |g|)."""
    x = np.ldexp(H.synth_series(seed, n, klass=0) - 1000.0, -30)
    x[n // 2] = float(np.ldexp(1.0, -1060))
    return x


def extras(n):
    return [straddling(n, 110), straddling(n, 600), tiny_straddling(n),
            with_tiny_sample(n, 0.0, n // 3), with_tiny_sample(n, float(np.ldexp(1.0, -1060)), n // 2),
            with_tiny_sample(n, -float(np.ldexp(1.0, -1074)), n - 1)]


def uniform_batch(n):
    """Frames of one length: every scale for every class at the small lengths, class 0 (and class 1 at the two
    scales where the two predicted divergences sit) above them -- the oracle's ladders are the slow part there."""
    if n in SMALL_LENGTHS:
        fr = [scaled(n, k, e) for k in KLASSES for e in SCALES]
        if n != 64:
            fr += extras(n)
        return fr
    return [scaled(n, 0, e) for e in SCALES] + [scaled(n, 1, 1000), scaled(n, 1, -1040)]


def large_batch():
    """A few 8192-sample frames: the large tier's compare-select sides, both predicted divergences, one frame with a
    zero inside, one with a subnormal sample among samples that all round to zero, and one at 2^90 -- the only one
    here whose FFT ladder runs at a large finite magnitude (the others take the 10-byte exit or are excused)."""
    n = LARGE_LENGTH
    return [scaled(n, 0, 110), scaled(n, 0, 600), scaled(n, 0, 1000), scaled(n, 0, -1040), scaled(n, 1, 130),
            with_tiny_sample(n, 0.0, n // 3), tiny_straddling(n), scaled(n, 0, 90)]


def mixed_batch():
    """Mixed lengths in one call (the table-driven kernels): every length up to 4096 at a few scales each."""
    fr = []
    for i, n in enumerate((64, 300, 256, 1024, 300, 4096, 64, 256)):
        for e in (SCALES[i % len(SCALES)], SCALES[(i + 5) % len(SCALES)], SCALES[(2 * i + 9) % len(SCALES)]):
            fr.append(scaled(n, KLASSES[i % 3], e))
    return fr


FLT_MAX = float(np.finfo(np.float32).max)


def f32_transform_may_overflow(x):
    """True for a frame whose forward transform can overflow in f32.  Every partial sum of any butterfly order is
    bounded by the sum of the |samples| (as f32): below FLT_MAX / 2 (the factor covers the edge padding, at most as
    long again) nothing overflows in any implementation; from there on which sums do, and whether +inf meets -inf,
    depends on the order of the additions (documented deviation).  Frames whose samples ALL
    convert to the same infinity are not meant: they take the max == min exit before any transform."""
    with np.errstate(over="ignore"):
        f = np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)
    if not np.all(np.isfinite(f)):
        return not (f.min() == f.max())
    return 2.0 * float(np.sum(np.abs(f))) >= FLT_MAX


def pack(frames):
    off = np.cumsum([0] + [len(f) for f in frames]).astype(np.uint64)
    return np.concatenate(frames), off


NONFINITE = (float("nan"), float("inf"), float("-inf"))


def nonfinite_batch(n):
    """NaN, +Inf and -Inf at the first, a middle and the last sample of an ordinary frame: nine frames."""
    fr = []
    for v in NONFINITE:
        for where in (0, n // 2, n - 1):
            x = H.synth_series(SEED, n, klass=0).copy()
            x[where] = v
            fr.append(x)
    return fr


# The IDW ladder is O(n K) a trip, on the CPU too (and the subnormal frame runs it in subnormal arithmetic: seconds per
# frame): above 300 samples IDW gets one frame of each compare-select side and the frames of the two divergences only.
def frames_for(n, mode):
    if mode[1] == "IDW" and n > 300:
        fr = [scaled(n, 0, 90), scaled(n, 0, 600), scaled(n, 0, 1000), scaled(n, 0, -1040)]
        return fr[:3] if mode[0] == "idw-e5" else fr
    return uniform_batch(n)


def mixed_frames(mode):
    fr = mixed_batch()
    return [f for f in fr if len(f) <= 1024] if mode[0] == "idw-e5" else fr


def large_frames(mode):
    fr = large_batch()
    return [fr[1], fr[2]] if mode[0] == "idw-e5" else fr


def all_batches():
    """(label, mode, frames) of every compress comparison of tests/test_gpu_extreme_values.py."""
    out = []
    for mode in MODES:
        for n in SMALL_LENGTHS + WIDE_LENGTHS:
            out.append(("uniform n=%d" % n, mode, frames_for(n, mode)))
        out.append(("mixed", mode, mixed_frames(mode)))
        out.append(("large", mode, large_frames(mode)))
        for n in (256, LARGE_LENGTH):
            out.append(("nonfinite n=%d" % n, mode, nonfinite_batch(n)))
    return out
