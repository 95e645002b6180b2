"""CPU-only tests of the window read's host half: atsc_bro_find_window against an independent walk of the records in
Python (reference fixtures encoded by the oracle, and the known-answer stream), its errors, and
atsc_vsri_sample_window against the VSRI oracle's look-ups."""
import os
import struct

import numpy as np
import pytest

from tests import helpers as H
from tests.golden import kat as K


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def walk(bro):
    """[(record start, record end, decoded samples)] of a .bro image; a Noop record decodes to its stored count"""
    n, pos = H.varint_decode(bro, 9)
    recs = []
    for _ in range(n):
        start = pos
        _fs, pos = H.varint_decode(bro, pos)
        sc, pos = H.varint_decode(bro, pos)
        tag, pos = H.varint_decode(bro, pos)
        ln, pos = H.varint_decode(bro, pos)
        if tag == 0:
            sc, _ = H.varint_decode(bro, pos + 1)
        pos += ln
        recs.append((start, pos, sc))
    return recs


def expect(recs, begin, count):
    starts = np.cumsum([0] + [r[2] for r in recs])
    total = int(starts[-1])
    assert begin + count <= total
    if count == 0:
        f = next((i for i in range(len(recs)) if starts[i + 1] > begin), len(recs))
        at = recs[f][0] if f < len(recs) else recs[-1][1]
        return dict(byte_begin=at, byte_end=at, frame_begin=f, frame_end=f, sample_begin=int(starts[f]))
    fb = next(i for i in range(len(recs)) if starts[i + 1] > begin)
    fe = next(i for i in range(len(recs)) if starts[i + 1] >= begin + count) + 1
    return dict(byte_begin=recs[fb][0], byte_end=recs[fe - 1][1], frame_begin=fb, frame_end=fe,
                sample_begin=int(starts[fb]))


def windows_of(recs, rng, n_random=40):
    starts = np.cumsum([0] + [r[2] for r in recs])
    total = int(starts[-1])
    w = {(0, total), (0, 0), (total, 0), (total - 1, 1), (0, 1)}
    for s in starts[1:-1]:
        s = int(s)
        for b in (s - 1, s, s + 1):
            if 0 <= b < total:
                w.add((b, 1))
                w.add((b, total - b))  # ends on the last sample
                w.add((b, 0))
            if 0 < b <= total:
                w.add((0, b))
    for _ in range(n_random):
        b = int(rng.integers(0, total))
        w.add((b, int(rng.integers(0, total - b + 1))))
    return sorted(w)


def fixture_streams(oracle, golden_dir):
    out = []
    for name in ("go_gc_heap_goal_bytes", "memory_used", "uptime"):
        x = H.read_wbro(os.path.join(golden_dir, "wbros", name + ".wbro"))
        for comp, err in ((oracle.AUTO, 3), (oracle.FFT, 1), (oracle.RLE, 0), (oracle.NOOP, 0), (oracle.POLYNOMIAL, 5)):
            out.append(("%s/%d" % (name, comp), oracle.compress_data(x, comp, err)))
    out.append(("kat_constant_1024", bytes(K.STREAM_CONSTANT_1024)))
    out.append(("kat_csv_constant", bytes.fromhex(K.CSV_CONSTANT_BRO_HEX)))
    return out


def test_find_window_matches_python_walk(A, oracle, golden_dir):
    rng = np.random.default_rng(11)
    for label, bro in fixture_streams(oracle, golden_dir):
        recs = walk(bro)
        assert A.bro_find_window(bro, 0, 0)["frame_begin"] == 0
        for b, c in windows_of(recs, rng):
            got = A.bro_find_window(bro, b, c)
            assert got == expect(recs, b, c), (label, b, c, got)


def test_find_window_errors(A, oracle, golden_dir):
    x = H.read_wbro(os.path.join(golden_dir, "wbros", "uptime.wbro"))
    bro = oracle.compress_data(x, oracle.POLYNOMIAL, 3)
    recs = walk(bro)
    total = sum(r[2] for r in recs)
    for b, c in ((0, total + 1), (total, 1), (total + 1, 0), (2 ** 63, 2 ** 63)):
        with pytest.raises(A.AtscError) as e:
            A.bro_find_window(bro, b, c)
        assert e.value.rc == A.capi.E_INVALID, (b, c)
    # truncated: the last record loses its last byte
    with pytest.raises(A.AtscError) as e:
        A.bro_find_window(bro[:-1], total - 1, 1)
    assert e.value.rc == A.capi.E_FORMAT
    # inflated: the first record's length field grows past the bytes present
    first = bytearray(bro)
    p = 9
    _n, p = H.varint_decode(first, p)
    for _ in range(3):
        _v, p = H.varint_decode(first, p)
    ln, q = H.varint_decode(first, p)
    if q - p == 1:
        first[p] = 250
    else:
        struct.pack_into({3: "<H", 5: "<I", 9: "<Q"}[q - p], first, p + 1, (1 << (8 * (q - p - 1))) - 1)
    with pytest.raises(A.AtscError) as e:
        A.bro_find_window(bytes(first), 0, 1)
    assert e.value.rc == A.capi.E_FORMAT
    # a window in front of a broken record is found: only the walk up to the window's end is checked
    broken = bytearray(bro)
    broken[recs[-1][0] + 2] = 5  # compressor id AUTO in the last record
    with pytest.raises(A.AtscError):
        A.bro_find_window(bytes(broken), 0, total)
    assert A.bro_find_window(bytes(broken), 0, recs[0][2])["frame_end"] == 1


def oracle_window(v, t0, t1):
    """this-or-next(t0) .. this-or-previous(t1) of the VSRI oracle, moved inwards past samples whose get_time falls
    outside [t0, t1]"""
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

    def time(x):
        return v.get_time(x)

    while i <= j and (time(i) is None or time(i) < t0):
        i += 1
    while j >= i and (time(j) is None or time(j) > t1):
        j -= 1
    return (i, j - i + 1) if j >= i else (0, 0)


def test_vsri_sample_window_matches_oracle(A):
    from oracle import vsri_oracle as VO

    rng = np.random.default_rng(5)
    for trial in range(60):
        # runs of equally spaced points with gaps between them (no one-point run: the reference's look-ups
        # divide by zero on those)
        t = int(rng.integers(0, 1000))
        pts = []
        for _ in range(int(rng.integers(1, 5))):
            step = int(rng.integers(1, 30))
            for _k in range(int(rng.integers(2, 40))):
                pts.append(t)
                t += step
            t += int(rng.integers(5, 500))
        mine, ref = A.Vsri(), VO.Vsri()
        for p in pts:
            mine.update_for_point(p)
            ref.update_for_point(p)
        if any(s[3] < 2 for s in ref.vsri_segments):
            continue
        lo, hi = pts[0], pts[-1]
        probes = [lo - 100, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, hi + 100] + [int(v) for v in rng.integers(lo - 50, hi + 50, 30)]
        for _ in range(40):
            a, b = sorted(rng.choice(probes, 2))
            a, b = int(a), int(b)
            got = mine.sample_window(a, b)
            want = oracle_window(ref, a, b)
            assert got == want, (trial, a, b, got, want, ref.vsri_segments)
            if got[1]:  # the window's ends lie inside [a, b]
                assert a <= ref.get_time(got[0]) <= b and a <= ref.get_time(got[0] + got[1] - 1) <= b
    # the reference README's index: windows of sample-aligned times in its first run are exactly those samples
    # (get_time of the second run adds m times the absolute sample number, lib.rs:320-341)
    v = A.Vsri()
    for p in K.VSRI_README_POINTS:
        v.update_for_point(p)
    ts = K.VSRI_README_POINTS
    for i, j in ((0, 0), (0, 165), (10, 100), (165, 165)):
        assert v.sample_window(ts[i], ts[j]) == (i, j - i + 1)
        assert v.sample_window(ts[i] - 7, ts[j] + 7) == (i, j - i + 1)
    assert v.sample_window(0, ts[0] - 1) == (0, 0)
    assert v.sample_window(ts[5], ts[4]) == (0, 0)
