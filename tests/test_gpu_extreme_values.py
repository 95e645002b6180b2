"""The lossy codecs at extreme sample magnitudes, on the GPU against the CPU oracle (tests/parity.py, bars unchanged).

The compress and decode kernels choose code by a frame's magnitude: fmin / fmax or compare-select clamps (|min|, |max|
against 1e150 in the spline, against 1e30f in the FFT error loop), the one-slice early exit (no zero in the frame),
v_rcp_f64 + Newton or a true divide for 1 / |g| (1e-290 < |g| < 1e290), the FMA form of x / 1e5, the saturating
casts of the integer bit depths.  tests/extreme_cases.py lists the inputs and why each scale is there;
tests/test_extreme_values_host.py shows on the CPU that none of them sits next to a decision threshold, so no frame
here may be excused as "boundary" (assert_summary allows none in a batch below 500 frames).

Two divergences from the reference were found with these tests and fixed (atsc_device.h: spline_term_slow, fft_term_slow,
div1e5_fix, mape_term; the decoders divide; DESIGN.md section 4 names the test that guards each fix):
  * x * 1e5 overflowing made div1e5 return NaN where round(x * 1e5) / 1e5 is +-inf, clamped to max / min
    (test_uniform_lengths[poly-e50-*] at 2^1000, test_hand_built_spline_records);
  * 1 / |g| overflowing for subnormal g made every error term inf where |(o - g) / g| is finite
    (test_uniform_lengths[poly-e50-*] at 2^-1040; the FFT evaluation, small and large tier: tiny_straddling frames
    under fft-e5 / fft-e50).  Both are spelled out in test_predicted_divergences_have_the_oracles_figures.
"""
import struct

import numpy as np
import pytest

from tests import extreme_cases as X
from tests import helpers as H
from tests import parity as P

pytestmark = pytest.mark.gpu


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


class _Cached:
    """The oracle with its per-frame answers kept: the compress tests, the two large-tier paths and the decode tests
    ask for the same frames under the same modes."""

    def __init__(self, oracle):
        self._o = oracle
        self._memo = {}

    def __getattr__(self, name):
        return getattr(self._o, name)

    def _call(self, name, x, *args):
        key = (name, np.asarray(x, dtype=np.float64).tobytes(), args)
        if key not in self._memo:
            self._memo[key] = getattr(self._o, name)(x, *args)
        return self._memo[key]

    def compress_best(self, x, me, level=0):
        return self._call("compress_best", x, float(me), level)

    def fft_allowed_error(self, x, me):
        return self._call("fft_allowed_error", x, float(me))

    def polynomial_allowed_error(self, x, me, idw=False):
        return self._call("polynomial_allowed_error", x, float(me), idw)

    def compress(self, comp, x, bounded=False, me=0.0):
        key = ("compress", comp, np.asarray(x, dtype=np.float64).tobytes(), bool(bounded), float(me))
        if key not in self._memo:
            self._memo[key] = self._o.compress(comp, x, bounded, me)
        return self._memo[key]


_cache = {}


@pytest.fixture(scope="module")
def orc(oracle):
    if "o" not in _cache:
        _cache["o"] = _Cached(oracle)
    return _cache["o"]


def _log(msg):
    print(msg)  # (shown for a failing case, or with -s: the figures before the assertion)


def _well_formed_fft(ctx, A, orc, frames, bounded, me, same_k, nan_err):
    """What is pinned where the FFT candidate cannot be held to the oracle's bins (documented
    deviations): the call succeeds, every record parses as an FFT record with positions inside the transform and the
    oracle's max / min (so bounded and unbounded runs agree on them), and decodes to n samples.  The bin count lies
    between 1 and the transform's bin count, and is the oracle's when unbounded (one pass, nothing measured) or with
    same_k.  The reported error is 0.0 when unbounded, NaN with nan_err, and otherwise NaN or a finite value >= 0."""
    x, off = X.pack(frames)
    rec, rec_off, chosen, err = ctx.compress_host(x, off, A.FFT, bounded, me, 0)
    recs = H.parse_bro_body(rec, with_count=False)
    assert len(recs) == len(frames) and int(rec_off[-1]) == len(rec)
    for i, (fs, sc, tag, payload) in enumerate(recs):
        n = len(frames[i])
        assert (fs, sc, tag) == (41, n, A.FFT)
        fg, mxg, mng = H.parse_fft_payload(payload)
        po, eo = orc.compress(A.FFT, frames[i], bounded, me)
        fo, mxo, mno = H.parse_fft_payload(po)
        assert all(p < int(orc.next_size(n)) or n < 128 and p < n for p, _, _ in fg)
        assert P.same_class(mxg, mxo) and P.same_class(mng, mno), (i, mxg, mxo, mng, mno)
        L = int(orc.next_size(n)) if n >= 128 else n
        assert 1 <= len(fg) <= L // 2 + 1, (i, len(fg), L)
        if same_k or not bounded:
            assert len(fg) == len(fo), (i, len(fg), len(fo))
        if not bounded:
            assert err[i] == 0.0 and eo == 0.0, (i, err[i], eo)
        elif nan_err:
            assert np.isnan(eo) and np.isnan(err[i]), (i, eo, err[i])
        else:
            assert np.isnan(err[i]) or (np.isfinite(err[i]) and err[i] >= 0.0), (i, err[i])
        out = ctx.decompress_host(_record(tag, n, payload))
        assert len(out) == n
        _log("well-formed fft n=%d K gpu=%d oracle=%d err gpu=%r oracle=%r" % (n, len(fg), len(fo), float(err[i]), eo))


def _compare(ctx, A, orc, frames, mode, what):
    name, comp, bounded, me = mode
    if comp == "FFT":
        over = [f for f in frames if X.f32_transform_may_overflow(f)]
        frames = [f for f in frames if not X.f32_transform_may_overflow(f)]
        if over:
            _well_formed_fft(ctx, A, orc, over, bounded, me, same_k=False, nan_err=False)
    x, off = X.pack(frames)
    s = P.compare_batch(orc, ctx, x, off, getattr(A, comp), bounded, me)
    _log("%s %s codecs %s err %s" % (what, name, s["codecs"], [float(e) for e in s["err"]]))
    _log(P.assert_summary(s, len(frames), "%s %s" % (what, name)))
    return s


MODE_IDS = [m[0] for m in X.MODES]


# ---------------------------------------------------------------------------------------
# compress: uniform batches (the fixed-length instantiations run), mixed lengths, the large tier's two paths
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", X.SMALL_LENGTHS + X.WIDE_LENGTHS)
@pytest.mark.parametrize("mode", X.MODES, ids=MODE_IDS)
def test_uniform_lengths(ctx, A, orc, mode, n):
    _compare(ctx, A, orc, X.frames_for(n, mode), mode, "uniform n=%d" % n)


@pytest.mark.parametrize("mode", X.MODES, ids=MODE_IDS)
def test_mixed_lengths(ctx, A, orc, mode):
    _compare(ctx, A, orc, X.mixed_frames(mode), mode, "mixed")


@pytest.mark.parametrize("path", ["fast", "general"])
@pytest.mark.parametrize("mode", X.MODES, ids=MODE_IDS)
def test_large_tier(ctx, A, orc, monkeypatch, mode, path):
    """8192-sample frames: the large tier's fast path, and (ATSC_LARGE_NO_FAST, as
    test_large_fast_path_matches_general_kernel selects it) the general per-frame kernel."""
    if path == "general":
        monkeypatch.setenv("ATSC_LARGE_NO_FAST", "1")
    else:
        monkeypatch.delenv("ATSC_LARGE_NO_FAST", raising=False)
    _compare(ctx, A, orc, X.large_frames(mode), mode, "large %s" % path)


@pytest.mark.parametrize("mode", X.EXACT_MODES, ids=[m[0] for m in X.EXACT_MODES])
def test_exact_codecs_control(ctx, A, orc, mode):
    """RLE, Noop and Constant on the same frames: bytes equal the oracle's (verdict exact for every frame)."""
    for fr in (X.uniform_batch(256), X.large_batch()[:3]):
        s = _compare(ctx, A, orc, fr, mode, "control n=%d" % len(fr[0]))
        assert s["exact"] == len(fr), s["codecs"]


def test_predicted_divergences_have_the_oracles_figures(ctx, A, orc):
    """The two cases the tests were written for, with the oracle's figures spelled out: forced bounded Polynomial at
    e = 50 % on the class-0 series * 2^1000 (x * 1e5 overflows: 24 B at n = 300, 32 B at 1024, 103 B at 8192) and
    * 2^-1040 (subnormal: 24 B at n = 300; a kernel whose error terms are inf runs to the K = n fallback, 322 B)."""
    for n, exp, size, err in ((300, 1000, 24, 0.2216), (1024, 1000, 32, 0.2704), (8192, 1000, 103, 0.2786),
                              (300, -1040, 24, 0.1874)):
        x = X.scaled(n, 0, exp)
        po, eo = orc.compress(A.POLYNOMIAL, x, True, X.ME50)
        assert len(po) == size and abs(eo - err) < 1e-4, (n, exp, len(po), eo)
        rec, _, _, e = ctx.compress_host(x, np.array([0, n], dtype=np.uint64), A.POLYNOMIAL, True, X.ME50, 0)
        (_, _, tag, payload), = H.parse_bro_body(rec, with_count=False)
        assert payload == po and not P.differs(e[0], eo, P.POLY_ERR_RTOL * eo), (n, exp, len(payload), e[0], eo)


# ---------------------------------------------------------------------------------------
# decode, both decoders: the oracle's own streams of the cases above
# ---------------------------------------------------------------------------------------
def _record(tag, n, payload):
    return P.H_varint(41) + P.H_varint(n) + P.H_varint(tag) + P.H_varint(len(payload)) + payload


def _same_values(out, ref):
    """Bit for bit where the reference is a number or an infinity; a NaN by class (its sign and payload are not the
    operation's: an x86 CPU and the GPU produce different default NaNs)."""
    out, ref = np.asarray(out), np.asarray(ref)
    nan = np.isnan(ref)
    return (len(out) == len(ref) and np.array_equal(np.isnan(out), nan)
            and np.array_equal(out[~nan].view(np.uint64), ref[~nan].view(np.uint64)))


def _decode_check(ctx, orc, frames, mode, A, what):
    name, comp, bounded, me = mode
    cid = getattr(A, comp)
    for i, fx in enumerate(frames):
        n = len(fx)
        if cid == A.AUTO:
            po, tag, _ = orc.compress_best(fx, me, 0)
        else:
            po, _ = orc.compress(cid, fx, bounded, me)
            tag = cid
        ref = np.array(orc.decompress(tag, po, n))
        out = ctx.decompress_host(_record(tag, n, po))
        assert len(out) == n
        if tag == A.FFT and X.f32_transform_may_overflow(fx):
            continue  # (documented deviation: the inverse of infinite bins; the decode above succeeded with n samples)
        if tag == A.FFT:
            # the bar of test_decompress_matches_oracle / test_decompress_large_frames (f32 inverse transform: 4 ulp of the
            # frame's magnitude up to 4096 samples, 4 + log2 n above; + one step of the 5-decimal grid); samples that
            # are not finite in the reference are compared by class
            fin = np.isfinite(ref)
            assert np.array_equal(np.isnan(out), np.isnan(ref)), (what, name, i)
            assert np.array_equal(out[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), (what, name, i)
            if fin.any():
                scale = max(float(np.max(np.abs(ref[fin]))), 1e-30)
                ulps = 4 if n <= 4096 else 4 + np.log2(n)
                d = float(np.max(np.abs(out[fin] - ref[fin])))
                assert d <= ulps * scale * 2.0 ** -23 + 1.00001e-5, (what, name, i, d, scale)
        else:
            assert _same_values(out, ref), (what, name, i, tag)


@pytest.mark.parametrize("mode", X.MODES, ids=MODE_IDS)
def test_decode_oracle_streams_small_tier(ctx, A, orc, mode):
    for n in (256, 300):
        _decode_check(ctx, orc, X.frames_for(n, mode), mode, A, "decode n=%d" % n)


@pytest.mark.parametrize("path", ["fast", "general"])
@pytest.mark.parametrize("mode", X.MODES, ids=MODE_IDS)
def test_decode_oracle_streams_large_tier(ctx, A, orc, monkeypatch, mode, path):
    if path == "general":
        monkeypatch.setenv("ATSC_LARGE_NO_FAST", "1")
    else:
        monkeypatch.delenv("ATSC_LARGE_NO_FAST", raising=False)
    _decode_check(ctx, orc, X.large_frames(mode), mode, A, "decode large %s" % path)


# ---------------------------------------------------------------------------------------
# decode: hand-built records
# ---------------------------------------------------------------------------------------
BIG = (1.7e308, -1.7e308, 1e304, -1e304)


def _spline_payload(orc, n, idw, points, mn, mx):
    """A Polynomial / IDW payload with f64 points (polynomial.rs:54-87: id, bit depth, points, min, max, point step) --
    the oracle's own record of an n-sample fractional frame (which fixes the point count and step as the reference
    lays them out), with the point values and min / max replaced."""
    base = orc.polynomial(H.synth_series(3, n, klass=0), idw=idw)
    pid, pos = H.varint_decode(base, 0)
    bd, pos = H.varint_decode(base, pos)
    k, pos = H.varint_decode(base, pos)
    assert bd == 0 and len(base) == pos + 8 * k + 17
    vals = [points[i % len(points)] for i in range(k)]
    return base[:pos] + struct.pack("<%dd" % k, *vals) + struct.pack("<dd", mn, mx) + base[-1:], k


@pytest.mark.parametrize("n", [300, 1024, 8192])
@pytest.mark.parametrize("idw", [False, True], ids=["poly", "idw"])
def test_hand_built_spline_records(ctx, A, orc, monkeypatch, idw, n):
    """Points at +-1.7e308 and +-1e304, alone and among ordinary values; min / max of the same sizes and at +-Inf.  The
    spline's value times 1e5 overflows: the reference rounds it to +-inf and clamps that to max / min
    (utils/mod.rs:66-74)."""
    tag = A.IDW if idw else A.POLYNOMIAL
    point_sets = (BIG, (1e304, 1e304, 1.7e308, 1.5e308), (1.0, 1e304, -3.5, -1.7e308, 2e303), (1.7e308,) * 3 + (-1.7e308,))
    # (the last two: a narrow range around huge points -- the overflowed value still clamps to max / min)
    ranges = ((-1.7e308, 1.7e308), (-1e304, 1e304), (-np.inf, np.inf), (-1e304, np.inf), (-np.inf, 1.7e308), (1e304, 1.7e308),
              (-1.0, 1.0), (2.5, 1e10))
    for path in (("fast", "general") if n > 4096 else ("small",)):
        if path == "general":
            monkeypatch.setenv("ATSC_LARGE_NO_FAST", "1")
        else:
            monkeypatch.delenv("ATSC_LARGE_NO_FAST", raising=False)
        for pts in point_sets:
            for mn, mx in ranges:
                pay, k = _spline_payload(orc, n, idw, pts, mn, mx)
                ref = np.array(orc.decompress(tag, pay, n))
                out = ctx.decompress_host(_record(tag, n, pay))
                assert _same_values(out, ref), (path, pts, mn, mx, k,
                                                [(i, out[i], ref[i]) for i in range(n) if not _same_values(out[i:i + 1], ref[i:i + 1])][:4])


@pytest.mark.parametrize("n", [256, 300, 8192])
def test_hand_built_fft_records(ctx, A, orc, monkeypatch, n):
    """FFT records with f32 coefficients near FLT_MAX and max_value / min_value = +-inf: the inverse transform overflows
    in f32.  Samples that are not finite in the reference are compared by class, the others to the decode bar.  (Bins whose
    sums overflow with opposite signs are left out: whether +inf meets -inf there is the transform's order of additions,
    DESIGN.md section 4.)"""
    flt_max = float(np.finfo(np.float32).max)
    L = int(orc.next_size(n))
    cases = []
    for mx, mn in ((np.inf, -np.inf), (flt_max, -flt_max), (np.inf, 0.0)):
        cases.append(([(0, flt_max / 2, 0.0)], mx, mn))                         # DC alone: L * (FLT_MAX / 2 / L), finite
        cases.append(([(0, flt_max, 0.0), (1, flt_max / 4, -flt_max / 4)], mx, mn))
        cases.append(([(0, 5.0e4, 0.0), (2, 1.0e3, -2.0e3)], mx, mn))           # ordinary bins, infinite range
    for path in (("fast", "general") if n > 4096 else ("small",)):
        if path == "general":
            monkeypatch.setenv("ATSC_LARGE_NO_FAST", "1")
        else:
            monkeypatch.delenv("ATSC_LARGE_NO_FAST", raising=False)
        for bins, mx, mn in cases:
            pay = bytes([15]) + P.H_varint(len(bins))
            for p, re, im in bins:
                pay += P.H_varint(p) + struct.pack("<ff", re, im)
            pay += struct.pack("<ff", mx, mn)
            ref = np.array(orc.decompress(A.FFT, pay, n))
            out = ctx.decompress_host(_record(A.FFT, n, pay))
            assert len(out) == n
            fin = np.isfinite(ref)
            assert np.array_equal(np.isnan(out), np.isnan(ref)), (path, bins, mx, mn, int(np.isnan(out).sum()), int(np.isnan(ref).sum()))
            inf = ~fin & ~np.isnan(ref)
            assert np.array_equal(out[inf], ref[inf]), (path, bins, mx, mn)
            if fin.any():
                scale = max(float(np.max(np.abs(ref[fin]))), 1e-30)
                d = float(np.max(np.abs(out[fin] - ref[fin])))
                ulps = 4 if n <= 4096 else 4 + np.log2(n)  # (the rule of _decode_check)
                assert d <= ulps * scale * 2.0 ** -23 + 1.00001e-5, (path, bins, mx, mn, d, scale)


# ---------------------------------------------------------------------------------------
# NaN, +Inf and -Inf inside a frame, through the frame-level ABI (compress_data's cleaner is not in front of it)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 8192])
@pytest.mark.parametrize("mode", [m for m in X.MODES if m[1] != "FFT"] + list(X.EXACT_MODES),
                         ids=lambda m: m[0])
def test_nonfinite_samples(ctx, A, orc, mode, n):
    """The oracle takes RLE under AUTO with both lossy errors NaN; the byte-exact codecs and the polynomial payloads
    (points are samples) equal the oracle's."""
    fr = X.nonfinite_batch(n)
    s = _compare(ctx, A, orc, fr, mode, "nonfinite n=%d" % n)
    if mode[1] == "AUTO":
        assert s["codecs"] == {A.RLE: len(fr)}, s["codecs"]
    if mode[1] != "FFT":
        assert s["exact"] == len(fr)


@pytest.mark.parametrize("n", [256, 8192])
@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
def test_nonfinite_samples_forced_fft(ctx, A, orc, bounded, n):
    """Forced FFT on a frame with a NaN or an infinity inside (documented deviation): every bin of the
    spectrum is NaN or infinite, the reference's choice among them is its heap's order over incomparable norms and
    its coefficients are whatever rustfft's butterflies leave.  Pinned here: the call succeeds, the record parses with
    as many bins as the oracle stores, positions inside the transform, max / min as the oracle's by class, and the
    reported error NaN when bounded (never chosen under AUTO: test_nonfinite_samples)."""
    _well_formed_fft(ctx, A, orc, X.nonfinite_batch(n), bounded, X.ME5, same_k=True, nan_err=True)
