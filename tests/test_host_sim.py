"""The host path of libatsc_hip.so on the CPU (no GPU): atsc_host.cpp / atsc_windows.cpp / atsc_stream.cpp built with
g++, AddressSanitizer and UBSan (tests/asan) and linked, without the HIP runtime, against a checking stand-in for it
(tests/asan/fake_hip.cpp: exact-size heap blocks for device memory, a table of page-locked ranges, a happens-before
record of every copy and launch) and against stand-ins for all 45 kernel launchers (tests/asan/sim_kernels.cpp: they
check every address the host's task tables name).  tests/asan/host_sim.cpp drives the pool, the plan cache, compress
and decode in parts, the pipelined entry point and every window query through their device, host and stream calls; the
decode and window scenarios walk valid streams of every codec and tier that the oracle writes here.

Each scenario is a process of its own (the library reads several switches once per process); it must end with exit
status 0: no sanitizer report, no leak, no violation counted by the stand-in, nothing left behind."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN = os.path.join(ROOT, "tests", "asan")
ME5 = float(np.float32(5) / np.float32(100))


@pytest.fixture(scope="module")
def host_sim():
    if shutil.which("g++") is None or shutil.which("make") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("no g++ / make / ROCm headers")
    subprocess.check_call(["make", "-s", "-j4", "-C", ASAN, "_build/host_sim"], stdout=subprocess.DEVNULL)
    return os.path.join(ASAN, "_build", "host_sim")


@pytest.fixture(scope="module")
def corpus(oracle, tmp_path_factory):
    """Valid .bro files from the oracle: every codec at several frame lengths, a large-tier stream, two streams of
    131072-sample frames whose records are longer than a part of the decode in parts (3 Noop, 5 RLE: more than 2^20
    record bytes each), and a stream long enough for a window to be cut into five pieces."""
    d = tmp_path_factory.mktemp("host_sim_corpus")
    for n in (12, 64, 256, 1000):
        x = np.concatenate([H.synth_series(11, n, klass=k) for k in (0, 1, 2, 3)])
        off = H.frame_offsets(len(x), n)
        for name, comp, bounded in (("auto", oracle.AUTO, True), ("fft", oracle.FFT, True), ("poly", oracle.POLYNOMIAL, True),
                                    ("idw", oracle.IDW, True), ("rle", oracle.RLE, False), ("noop", oracle.NOOP, False),
                                    ("constant", oracle.CONSTANT, False)):
            bro, _, _ = oracle.stream_compress(x, off, comp, bounded, ME5, 0)
            (d / ("%s_%d.bro" % (name, n))).write_bytes(bytes(bro))
    x = H.synth_series(2, 16384 + 3 * 2048)
    bro, _, _ = oracle.stream_compress(x, np.array([0, 16384, 18432, 20480, 22528], dtype=np.uint64), oracle.AUTO, True, ME5, 0)
    (d / "large_16384.bro").write_bytes(bytes(bro))
    F = 131072
    # (RLE of a series without repeats: a record per frame of more than a megabyte)
    for name, comp, klass, nfr in (("noop3", oracle.NOOP, 0, 3), ("rle5", oracle.RLE, 0, 5)):
        x = np.concatenate([H.synth_series(60 + k, F, klass=klass) for k in range(nfr)])
        bro, _, _ = oracle.stream_compress(x, H.frame_offsets(len(x), F), comp, False, 0.0, 0)
        assert len(bro) >= (1 << 20), name
        (d / (name + ".bro")).write_bytes(bytes(bro))
    # 5 x 32 tiles of 2048 samples and a little more, in frames of 256: lossless codecs (cheap in the oracle) around a
    # stretch of Auto frames
    n = 5 * 32 * 2048 + 3 * 256
    x = H.synth_series(9, n, block=4096)
    parts = []
    for a, b, comp, bounded in ((0, 300, oracle.RLE, False), (300, 700, oracle.AUTO, True), (700, n // 256, oracle.NOOP, False)):
        seg = x[a * 256:b * 256]
        bro, _, _ = oracle.stream_compress(seg, H.frame_offsets(len(seg), 256), comp, bounded, ME5, 0)
        bro = bytes(bro)
        parts.append(bro[9 + len(_varint(b - a)):])
    head = b"BRRO" + (1).to_bytes(4, "little") + bytes([(n // 256) & 0xFF]) + _varint(n // 256)
    (d / "win_small.bro").write_bytes(head + b"".join(parts))
    return str(d)


def _varint(v):
    if v < 251:
        return bytes([v])
    if v < 1 << 16:
        return bytes([251]) + v.to_bytes(2, "little")
    if v < 1 << 32:
        return bytes([252]) + v.to_bytes(4, "little")
    return bytes([253]) + v.to_bytes(8, "little")


def _run(host_sim, corpus, scenario, extra_env=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.update(extra_env or {})
    p = subprocess.run([host_sim, scenario, corpus], env=env, capture_output=True, text=True, timeout=600)
    counts = [l for l in p.stdout.splitlines() if l.startswith("fake_hip: scenario=")]
    # (the counts of every run, beside the binary: tests/asan/_build is git-ignored)
    with open(os.path.join(ASAN, "_build", "host_sim.log"), "a") as f:
        f.write("%s%s exit=%d\n" % ("".join(c + " " for c in counts) or scenario + ": no count line ",
                                   " ".join("%s=%s" % kv for kv in (extra_env or {}).items()), p.returncode))
    return p, counts


SCENARIOS = ["compress", "decode", "faulted", "pipelined", "windows", "windows_large", "windows_across64"]


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_host_path_against_the_checking_runtime(host_sim, corpus, scenario):
    p, counts = _run(host_sim, corpus, scenario)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert len(counts) == 1 and counts[0].endswith(" violations=0"), p.stdout[-2000:]
    assert "VIOLATION" not in p.stderr and "ERROR: " not in p.stderr, p.stderr[-6000:]
    m = re.search(r"launches=(\d+) copies=(\d+)", counts[0])
    assert m and int(m.group(1)) > 50 and int(m.group(2)) > 50, counts[0]  # the scenario got past atsc_ctx_create


@pytest.mark.parametrize("fail_set", [1, 2, 3, 5])
def test_pipelined_with_a_scratch_set_that_cannot_be_built(host_sim, corpus, fail_set):
    """ATSC_DEBUG_FAIL_SET lets the allocation of scratch set q and every later one fail half-way: the sets built so far
    stay, the rotation goes over fewer chains, and the half-built set's blocks go back to the pool."""
    p, counts = _run(host_sim, corpus, "pipelined", {"ATSC_DEBUG_FAIL_SET": str(fail_set)})
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert len(counts) == 1 and counts[0].endswith(" violations=0"), p.stdout[-2000:]


def test_the_stand_in_counts_misuse(host_sim, corpus):
    """No product code in this one: a double free, a copy one byte past a block, an unordered write after a read on
    two streams, an unregister with a copy in flight and a pageable result handed on before its copy was joined are
    each counted once -- and the same accesses with an event or a join between them are not."""
    p, counts = _run(host_sim, corpus, "selfcheck")
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert "selfcheck: 5 of 5 misuses counted, 5 violations in all" in p.stdout
    assert p.stderr.count("fake_hip: VIOLATION") == 5
