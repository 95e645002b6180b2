"""CPU side of the extreme-magnitude tests (tests/test_gpu_extreme_values.py).

(a) Known answers that pin the measuring stick -- the CPU oracle -- where the GPU tests lean on it: hand-derived from
    the reference's source (file and line cited), as tests/test_oracle_kat.py does.
(b) The condition that keeps the GPU test honest: for every input it compresses, the oracle's errors are not within
    BOUNDARY_EPS of a threshold at which the reference's decisions flip (parity._near_threshold), so a frame that differs
    can never be excused as "boundary"; and every batch stays below 500 frames, where assert_summary allows no boundary
    frame and at most one tie.
(c) parity.py's comparison of non-finite values: by class, never vacuously.
"""
import struct

import numpy as np
import pytest

from tests import extreme_cases as X
from tests import helpers as H
from tests import parity as P


# ---- (a) known answers -----------------------------------------------------------------

def test_round_and_limit_when_the_product_overflows(oracle):
    # utils/mod.rs:66-74: out = (x * y).round() / y; 1.8e303 * 1e5 is beyond f64::MAX (1.797e308): +inf, inf.round() = inf,
    # inf / 1e5 = inf, which is `> max` -> max.  The mirror image gives min.  NaN compares false twice and stays NaN.
    assert oracle.round_and_limit_f64(1.8e303, -1.0e308, 1.5e308, 5) == 1.5e308
    assert oracle.round_and_limit_f64(-1.8e303, -1.0e308, 1.5e308, 5) == -1.0e308
    assert oracle.round_and_limit_f64(1.0e304, -np.inf, np.inf, 5) == np.inf
    assert np.isnan(oracle.round_and_limit_f64(np.nan, -1.0, 1.0, 5))
    # just below the overflow nothing is clamped: 1e303 * 1e5 = 1e308 is finite
    assert abs(oracle.round_and_limit_f64(1.0e303, -1.7e308, 1.7e308, 5) / 1.0e303 - 1.0) < 1e-15


def test_mape_term_of_a_subnormal_original(oracle):
    # utils/error.rs:104-116: sum(|(generated - original) / original|) / len -- a division, so a subnormal original
    # (whose reciprocal would overflow) gives a finite term: (0 - g) / g = -1; (3g - g) / g = 2 (exact: powers of two)
    g = float(np.ldexp(1.0, -1040))
    assert oracle.error_mape([g], [0.0]) == 1.0
    assert oracle.error_mape([g], [3.0 * g]) == 2.0
    assert oracle.error_mape([g, 4.0], [0.0, 5.0]) == 0.625
    # a zero original: x / 0 = inf, 0 / 0 = NaN
    assert oracle.error_mape([0.0, 4.0], [1.0, 4.0]) == np.inf
    assert np.isnan(oracle.error_mape([0.0, 4.0], [0.0, 4.0]))


def test_f32_overflow_gives_the_ten_byte_fft_payload(oracle):
    # fft.rs:173-180: `x as f32` of a finite value beyond f32::MAX is +inf (Rust's float casts saturate to infinity; the
    # function only logs).  Every sample of the class-0 series * 2^126 (about 7e40 .. 1e41) is: max == min == inf, and
    # fft.rs:289-292 returns without a transform.  Payload (fft.rs:119-130): id 15, zero frequencies, max f32, min f32.
    x = X.scaled(256, 0, 126)
    assert x.min() > float(np.finfo(np.float32).max)
    pay, err = oracle.compress(oracle.FFT, x, True, X.ME5)
    assert pay == bytes([15, 0]) + struct.pack("<ff", np.inf, np.inf) and len(pay) == 10
    assert err == 0.0
    _, chosen, e = oracle.compress_best(x, X.ME5)  # 10 bytes with error 0.0: nothing is smaller
    assert chosen == oracle.FFT and e == 0.0


def test_bit_depth_casts_saturate_on_huge_integers(oracle):
    # optimizer/utils.rs:115-160 split_n: for an exponent that shifts the mantissa out of 128 bits the integer part is 0
    # and the fraction is "zero": 3 * 2^600 counts as the integer 0, so the frame's bit depth is U8 (utils.rs:91-113).
    # constant.rs:43-60 then encodes `self.constant as u8`: a saturating cast, 255.  Payload: id 30, bit depth 3, 255.
    big = float(np.ldexp(3.0, 600))
    s = oracle.stats([big] * 4)
    assert s.bitdepth == oracle.BD_U8 and not s.fractional
    assert oracle.constant([big] * 4) == bytes([30, 3, 255])
    # the negative image: min_int = 0 as well, still U8; `as u8` of a negative value is 0
    assert oracle.constant([-big] * 4) == bytes([30, 3, 0])
    # polynomial.rs:61-66 casts every point the same way
    x = np.floor(X.scaled(64, 0, 600))
    pay = oracle.polynomial(x)
    info = H.parse_poly_payload(pay)
    assert info["bitdepth"] == oracle.BD_U8 and set(pay[3:3 + info["npoints"]]) == {255}


def test_a_nan_error_never_passes_the_selector(oracle):
    # frame/mod.rs:128-141: a result is eligible when `result.error <= max_error`, false for NaN.  A frame with a NaN sample
    # has NaN errors for FFT and Polynomial (utils/error.rs:112 sums a NaN term); RLE reports 0.0 and is taken although
    # both lossy payloads are smaller.
    x = H.synth_series(7, 256, klass=0).copy()
    x[128] = np.nan
    pf, ef, _ = oracle.fft_allowed_error(x, X.ME50)
    pp, ep, _ = oracle.polynomial_allowed_error(x, X.ME50)
    pr = oracle.rle(x)
    assert np.isnan(ef) and np.isnan(ep)
    assert len(pf) < len(pr) and len(pp) < len(pr)
    pay, chosen, err = oracle.compress_best(x, X.ME50)
    assert chosen == oracle.RLE and err == 0.0 and pay == pr


def test_predicted_divergence_figures(oracle):
    # the figures the issue quotes for forced bounded Polynomial at e = 50 % on the class-0 series
    for n, exp, size, err in ((300, 1000, 24, 0.2216), (1024, 1000, 32, 0.2704), (8192, 1000, 103, 0.2786),
                              (300, -1040, 24, 0.1874)):
        pay, e = oracle.compress(oracle.POLYNOMIAL, X.scaled(n, 0, exp), True, X.ME50)
        assert len(pay) == size and abs(e - err) < 1e-4, (n, exp, len(pay), e)


# ---- (b) no input of the GPU test sits next to a threshold ------------------------------

@pytest.mark.parametrize("mode", X.MODES, ids=[m[0] for m in X.MODES])
def test_no_input_is_near_a_decision_threshold(oracle, mode):
    name, comp, bounded, me = mode
    seen = 0
    for label, m, frames in X.all_batches():
        if m is not mode:
            continue
        assert len(frames) < 500, label
        if not bounded:
            continue  # no error loop and no selector: nothing is decided by the error
        for i, f in enumerate(frames):
            if comp == "AUTO":
                errs = (oracle.fft_allowed_error(f, me)[1], oracle.polynomial_allowed_error(f, me)[1])
            else:
                errs = (oracle.compress(getattr(oracle, comp), f, True, me)[1],)
            assert not any(P._near_threshold(e, me) for e in errs), (label, name, i, errs)
            seen += 1
    assert seen or not bounded


# ---- (c) parity.py compares non-finite values by class ----------------------------------

def _fft_payload(bins, mx, mn):
    pay = bytes([15]) + P.H_varint(len(bins))
    for p, re, im in bins:
        pay += P.H_varint(p) + struct.pack("<ff", re, im)
    return pay + struct.pack("<ff", mx, mn)


def test_compare_frame_does_not_let_a_nan_match(oracle):
    x = np.arange(64, dtype=np.float64)
    nan, inf = float("nan"), float("inf")
    ref = _fft_payload([(0, 5.0, 0.0), (3, 1.0, -2.0)], 9.0, 1.0)

    def verdict(gpu, orc_pay=ref):
        return P.compare_frame(oracle, x, 0.05, oracle.FFT, gpu, oracle.FFT, orc_pay, {}, 0, {"e": 0.2})

    assert verdict(_fft_payload([(0, 5.0, 0.0), (3, 1.0, -2.000001)], 9.0, 1.0)) == "tol"
    assert verdict(_fft_payload([(0, 5.0, 0.0), (3, nan, -2.0)], 9.0, 1.0)).startswith("FAIL")
    assert verdict(_fft_payload([(0, 5.0, 0.0), (3, 1.0, inf)], 9.0, 1.0)).startswith("FAIL")
    assert verdict(_fft_payload([(0, 5.0, 0.0), (3, 1.0, -2.0)], nan, 1.0)).startswith("FAIL")
    # the same class on both sides matches; another infinity, or a NaN against an infinity, does not
    both = _fft_payload([(0, inf, 0.0), (3, nan, -2.0)], inf, -inf)
    assert verdict(_fft_payload([(0, inf, 0.0), (3, nan, -2.000001)], inf, -inf), both) == "tol"
    assert verdict(_fft_payload([(0, -inf, 0.0), (3, nan, -2.0)], inf, -inf), both).startswith("FAIL")
    assert verdict(_fft_payload([(0, nan, 0.0), (3, nan, -2.0)], inf, -inf), both).startswith("FAIL")
    assert verdict(_fft_payload([(0, inf, 0.0), (3, nan, -2.0)], inf, nan), both).startswith("FAIL")
    # an infinite bin does not widen the tolerance of the finite ones
    assert verdict(_fft_payload([(0, inf, 0.0), (3, nan, -2.1)], inf, -inf), both).startswith("FAIL")


def test_differs_by_class():
    nan, inf = float("nan"), float("inf")
    assert not P.differs(nan, nan, 0.0) and not P.differs(inf, inf, 0.0) and not P.differs(1.0, 1.0 + 1e-9, 1e-6)
    assert P.differs(nan, 1.0, inf) and P.differs(1.0, nan, inf) and P.differs(inf, -inf, inf)
    assert P.differs(inf, 1.0, inf) and P.differs(nan, inf, inf) and P.differs(1.0, 2.0, 0.5)
