"""NumPy restatement of the windowed moments' contract (include/atsc_hip.h, DESIGN.md "Windowed moments"): nodes
(n, mx, M2x, mt, M2t, C) merged level by level in the documented tree, from the full decode's samples; the fit read off
them (atsc_moments_fit); exact values in rational arithmetic and the documented error bounds."""
import math
from fractions import Fraction

import numpy as np

TILE = 2048
U = 2.0 ** -53

FIELDS = ("count", "mean", "m2", "t_mean", "t_m2", "c_tx")


def merge(a, b):
    """Merge(a, b) of arrays of nodes (n, mx, M2x, mt, M2t, C): a where nb == 0, b where na == 0, else the rule -- every
    line one rounded f64 operation (NumPy does not fuse)"""
    na, mxa, m2xa, mta, m2ta, ca = a
    nb, mxb, m2xb, mtb, m2tb, cb = b
    n = na + nb
    with np.errstate(all="ignore"):  # 0 / 0 where both are empty; Inf - Inf as on the GPU
        w = nb.astype(np.float64) / n.astype(np.float64)
        f = na.astype(np.float64) * w
        dx = mxb - mxa
        dt = mtb - mta
        mx = mxa + dx * w
        mt = mta + dt * w
        m2x = (m2xa + m2xb) + (dx * dx) * f
        m2t = (m2ta + m2tb) + (dt * dt) * f
        c = (ca + cb) + (dx * dt) * f
    ea, eb = na == 0, nb == 0

    def pick(ra, rb, r):
        return np.where(eb, ra, np.where(ea, rb, r))

    return (pick(na, nb, n), pick(mxa, mxb, mx), pick(m2xa, m2xb, m2x), pick(mta, mtb, mt), pick(m2ta, m2tb, m2t),
            pick(ca, cb, c))


def _take(node, idx):
    return tuple(f[idx] for f in node)


def tile_nodes(x, t, ok):
    """the nodes of tiles: x, t, ok of shape (tiles, 2048) -- values, stream positions and "inside the window and not
    NaN"; per virtual lane v the pairs (512 q + 2 v, 512 q + 2 v + 1) as Merge(Merge(p0, p1), Merge(p2, p3)), then a
    halving tree over the 256 lanes"""
    ok = np.asarray(ok, dtype=bool).reshape(-1, 4, 256, 2)
    z = np.zeros(ok.shape)
    leaf = (ok.astype(np.uint64), np.where(ok, np.asarray(x, dtype=np.float64).reshape(ok.shape), 0.0), z,
            np.where(ok, np.asarray(t, dtype=np.float64).reshape(ok.shape), 0.0), z, z)
    p = merge(_take(leaf, (Ellipsis, 0)), _take(leaf, (Ellipsis, 1)))
    q = [_take(p, (slice(None), k)) for k in range(4)]
    s = merge(merge(q[0], q[1]), merge(q[2], q[3]))
    h = 128
    while h >= 1:
        s = merge(_take(s, (slice(None), slice(0, h))), _take(s, (slice(None), slice(h, 2 * h))))
        h //= 2
    return _take(s, (slice(None), 0))


def pairwise(q):
    """q[i] = Merge(q[2 i], q[2 i + 1]) level by level, an odd last entry merged with the empty node -> one node"""
    while len(q[0]) > 1:
        if len(q[0]) % 2:
            q = tuple(np.append(f, f.dtype.type(0)) for f in q)
        q = merge(_take(q, slice(0, None, 2)), _take(q, slice(1, None, 2)))
    return tuple(f[0] for f in q)


def window_moments(x, begin, count):
    """-> (count, mean, m2, t_mean, t_m2, c_tx) of x[begin:begin + count] as the contract defines them"""
    nan = float("nan")
    if count == 0:
        return 0, nan, nan, nan, nan, nan
    kb, ke = begin // TILE, (begin + count - 1) // TILE
    n_slots = (ke - kb + 1) * TILE
    lo = begin - kb * TILE
    seg = np.zeros(n_slots)
    seg[lo:lo + count] = x[begin:begin + count]
    ok = np.zeros(n_slots, dtype=bool)
    ok[lo:lo + count] = ~np.isnan(seg[lo:lo + count])
    t = np.arange(kb * TILE, kb * TILE + n_slots, dtype=np.float64)
    shape = (-1, TILE)
    n, mx, m2x, mt, m2t, c = pairwise(tile_nodes(seg.reshape(shape), t.reshape(shape), ok.reshape(shape)))
    if int(n) == 0:
        return 0, nan, nan, nan, nan, nan
    with np.errstate(all="ignore"):
        return int(n), float(mx), float(m2x), float(mt - np.float64(begin)), float(m2t), float(c)


def windows_moments(x, wins):
    """-> structured array (the fields of atsc_window_moments) of the windows (begin, count) of x"""
    out = np.zeros(len(wins), dtype=[("count", "<u8")] + [(k, "<f8") for k in FIELDS[1:]])
    for i, (b, c) in enumerate(wins):
        out[i] = window_moments(x, int(b), int(c))
    return out


def fit(count, mean, m2, t_mean, t_m2, c_tx):
    """atsc_moments_fit of one record -> (mean, variance, stddev, sample_variance, sample_stddev, slope, intercept)"""
    nan = np.float64("nan")
    if count == 0:
        return (nan,) * 7
    mean, m2, t_mean, t_m2, c_tx = (np.float64(v) for v in (mean, m2, t_mean, t_m2, c_tx))
    with np.errstate(all="ignore"):
        var = m2 / np.float64(count)
        svar = m2 / np.float64(count - 1) if count >= 2 else nan
        slope = c_tx / t_m2 if t_m2 > 0 else nan
        st = slope * t_mean
        return mean, var, np.sqrt(var), svar, np.sqrt(svar), slope, mean - st


def _scaled_int(v):
    """v * 2^1074 as an integer (exact for every finite double)"""
    num, den = float(v).as_integer_ratio()
    return num * ((1 << 1074) // den)


def exact_moments(v):
    """-> (count, mean, m2, t_mean, t_m2, c_tx, mean|x|) as Fractions, of the finite samples v (NaN excluded) at the
    positions 0 .. len(v) - 1"""
    v = np.asarray(v, dtype=np.float64)
    idx = [i for i in range(len(v)) if not math.isnan(v[i])]
    n = len(idx)
    if n == 0:
        return 0, None, None, None, None, None, None
    xs = [_scaled_int(v[i]) for i in idx]
    sx, sxx, st, stt = sum(xs), sum(a * a for a in xs), sum(idx), sum(i * i for i in idx)
    stx = sum(i * a for i, a in zip(idx, xs))
    one, two = Fraction(1, 1 << 1074), Fraction(1, 1 << 2148)
    mean = Fraction(sx, n) * one
    m2 = (Fraction(sxx) - Fraction(sx * sx, n)) * two
    t_mean = Fraction(st, n)
    t_m2 = Fraction(stt) - Fraction(st * st, n)
    c_tx = (Fraction(stx) - Fraction(st * sx, n)) * one
    return n, mean, m2, t_mean, t_m2, c_tx, Fraction(sum(abs(a) for a in xs), n) * one


def bounds(n, mean, m2, t_m2):
    """the documented bounds (b_mean / mean|x|, b_m2, b_t_m2, b_c_tx) from the exact values: with L = max(1,
    ceil(log2 n)) and kappa = sqrt(1 + n mean^2 / m2), (L + 2) u times (1, kappa m2, t_m2, kappa sqrt(t_m2 m2)).
    kappa m2 = sqrt(m2 (m2 + n mean^2)) keeps the product finite where m2 == 0."""
    L = max(1, math.ceil(math.log2(n))) if n > 1 else 1
    k = (L + 2) * U
    m2f, tf = float(m2), float(t_m2)
    km2 = math.sqrt(m2f * (m2f + n * float(mean) ** 2))  # kappa m2
    return k, k * km2, k * tf, k * math.sqrt(tf * (m2f + n * float(mean) ** 2))  # kappa sqrt(t_m2 m2)
