"""CPU-only tests of the windowed aggregates' host half: atsc_vsri_step_windows against the VSRI oracle bucket by
bucket, bucket_windows, and the NumPy model of the documented sum order against math.fsum."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import agg_model as M


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def oracle_window(v, t0, t1):
    """this-or-next(t0) .. this-or-previous(t1) of the VSRI oracle, moved inwards past samples whose get_time falls
    outside [t0, t1] (the rule of atsc_vsri_sample_window)"""
    n = v.get_sample_count()
    if not v.vsri_segments or n <= 0 or t1 < t0:
        return 0, 0
    i = v.get_this_or_next(t0)
    if i is None:
        return 0, 0
    j = v.get_this_or_previous(t1)
    if j is None:
        return 0, 0
    i, j = max(i, 0), min(j, n - 1)
    while i <= j and (v.get_time(i) is None or v.get_time(i) < t0):
        i += 1
    while j >= i and (v.get_time(j) is None or v.get_time(j) > t1):
        j -= 1
    return (i, j - i + 1) if j >= i else (0, 0)


def oracle_steps(v, t0, t1, step):
    out = []
    a = t0
    while a <= t1:  # Python integers: no wrap near INT32_MAX
        out.append(oracle_window(v, a, min(a + step - 1, t1)))
        a += step
    return out


def _index(A, pts):
    from oracle import vsri_oracle as VO

    mine, ref = A.Vsri(), VO.Vsri()
    for p in pts:
        mine.update_for_point(p)
        ref.update_for_point(p)
    return mine, ref


def _check(A, mine, ref, t0, t1, step):
    from oracle import vsri_oracle as VO

    try:
        want = oracle_steps(ref, t0, t1, step)
    except VO.Panic:
        with pytest.raises(A.AtscError) as e:
            mine.step_windows(t0, t1, step)
        assert e.value.rc == A.capi.E_INVALID
        return
    b, c = mine.step_windows(t0, t1, step)
    got = list(zip(b.tolist(), c.tolist()))
    assert got == [tuple(w) for w in want], (t0, t1, step)


def test_step_windows_match_oracle(A):
    rng = np.random.default_rng(41)
    tried = 0
    for trial in range(80):
        t = int(rng.integers(0, 1000))
        pts = []
        for _ in range(int(rng.integers(1, 5))):
            step = int(rng.integers(1, 30))
            for _k in range(int(rng.integers(2, 40))):
                pts.append(t)
                t += step
            t += int(rng.integers(5, 500))  # gaps between runs
        mine, ref = _index(A, pts)
        if any(s[3] < 2 for s in ref.vsri_segments):
            continue
        tried += 1
        lo, hi = pts[0], pts[-1]
        for _ in range(12):
            t0 = int(rng.integers(lo - 100, hi + 100))
            t1 = t0 + int(rng.integers(-20, hi - lo + 200))  # t1 < t0 included
            step = int(rng.choice([1, 2, 7, 60, 333, 10 ** 6]))  # off-grid starts; steps beyond the range
            _check(A, mine, ref, t0, t1, step)
    assert tried > 20


def test_step_windows_edges(A):
    mine, ref = _index(A, list(range(100, 400, 3)))
    for t0, t1, step in ((100, 397, 3), (101, 397, 3), (0, 1000, 50), (250, 250, 1), (300, 200, 5), (0, 10, 1000),
                         (-(2 ** 31), 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 10, 2 ** 31 - 1, 4),
                         (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (-(2 ** 31), -(2 ** 31) + 5, 2)):
        _check(A, mine, ref, t0, t1, step)
    # a run of points near INT32_MAX: bucket starts past it must not wrap
    top = 2 ** 31 - 1
    mine2, ref2 = _index(A, list(range(top - 300, top - 2, 7)))
    for t0, t1, step in ((top - 400, top, 10), (top - 300, top, 1000), (top - 5, top, 2)):
        _check(A, mine2, ref2, t0, t1, step)
    # capacity: *n is the bucket count, nothing is written
    b = np.full(4, 7, dtype=np.uint64)
    c = np.full(4, 7, dtype=np.uint64)
    n = C.c_uint64()
    p = C.POINTER(C.c_uint64)
    rc = A.capi.lib().atsc_vsri_step_windows(mine._h, 100, 399, 10, b.ctypes.data_as(p), c.ctypes.data_as(p), 4,
                                             C.byref(n))
    assert rc == A.capi.E_CAPACITY and n.value == 30 and np.all(b == 7) and np.all(c == 7)
    for step in (0, -3):
        with pytest.raises(A.AtscError) as e:
            mine.step_windows(100, 200, step)
        assert e.value.rc == A.capi.E_INVALID
    eb, ec = mine.step_windows(300, 200, 5)
    assert len(eb) == 0 and len(ec) == 0


def test_bucket_windows(A):
    for begin, count, bucket in ((0, 10, 3), (5, 9, 3), (7, 0, 4), (0, 2048, 2048), (100, 1, 60), (3, 100, 1000)):
        b, c = A.bucket_windows(begin, count, bucket)
        assert b.dtype == np.uint64 and c.dtype == np.uint64
        assert int(c.sum()) == count
        assert all(int(x) == begin + i * bucket for i, x in enumerate(b))
        assert all(int(x) == bucket for x in c[:-1]) and (count == 0 or 0 < int(c[-1]) <= bucket)
    with pytest.raises(ValueError):
        A.bucket_windows(0, 10, 0)


def test_window_stats_dtype(A):
    assert A.WINDOW_STATS.itemsize == 48
    assert A.WINDOW_STATS.names == ("count", "min", "max", "sum", "first", "last")


def test_sum_model_within_bound_of_fsum():
    rng = np.random.default_rng(43)
    x = np.concatenate([rng.normal(0, 1e3, 300000), rng.normal(1e9, 1.0, 50000) * rng.choice([-1, 1], 50000),
                        rng.uniform(-1, 1, 100000) * 10.0 ** rng.integers(-30, 30, 100000)])
    x[rng.integers(0, len(x), 500)] = np.nan
    wins = [(0, len(x)), (1, 2047), (2047, 2), (4096, 2048), (5000, 1), (0, 0), (123, 0)]
    wins += [(int(b), int(rng.integers(0, min(len(x) - b, 300000) + 1))) for b in rng.integers(0, len(x), 60)]
    for b, c in wins:
        v = x[b:b + c]
        s = M.window_sum(x, b, c)
        ok = v[~np.isnan(v)]
        exact = math.fsum(ok)
        assert abs(s - exact) <= M.error_bound(v), (b, c, s, exact)
        n, mn, mx, _s, first, last = M.window_stats(x, b, c)
        assert n == len(ok)
        if len(ok):
            assert mn == np.nanmin(v) and mx == np.nanmax(v)
        else:
            assert s == 0.0 and math.copysign(1, s) == 1 and math.isnan(mn) and math.isnan(mx)
    # padding never changes a bit: a window's tile sums ignore what lies outside it
    y = x.copy()
    y[:1000] = 1e300
    y[3000:] = -7.0
    assert np.float64(M.window_sum(x, 1000, 2000)).view(np.uint64) == np.float64(M.window_sum(y, 1000, 2000)).view(np.uint64)
