"""Windowed value counts probe (atsc_values_windows_dev) on one GPU.

The bench's batch (10,485,760 samples, 40960 frames x 256) in two kinds: the bench's noisy series (auto, e = 5 %; next
to every decoded value is distinct, so every tile runs k rounds) and a five-level state series with long dwell times
(auto, e = 0: Constant and RLE frames), each queried as one whole-stream window and as 1-minute buckets (60 samples).
Per series and shape four things are timed alternately in one process, after warm-up rounds, each between HIP events of
its own around the device call (host task planning is inside: call time, not kernel time), and reported as median, min
and max over --reps rounds, with the median time the host spent inside the call beside them:
  values4   atsc_values_windows_dev with k = 4
  values32  atsc_values_windows_dev with k = 32
  extremes  atsc_extremes_windows_dev with k = 16
  decode    atsc_decompress_windows_dev of the same windows (the samples handed out, no reduction)
A few windows of every result are checked against the NumPy model.  Kernel-only times come from a
rocprofv3 --kernel-trace --stats run of this probe (a run of its own; --reps 3 keeps it short).

--parent NAME then runs the extremes and decode timings alone in child processes, twice on this build's library and
twice on the side-by-side library libatsc_hip_NAME.so (a build of the parent commit copied next to the package's library;
atsc_amd/capi.py, ATSC_LIB_VARIANT), in turn: the parent has no value-count call, so those are the existing calls whose
cost must not move.  Prints one JSON object per series, shape and library; --out FILE also writes them there.

    python tools/values_probe.py [--reps 20] [--buckets 0,60] [--parent parent] [--out profiles/values_probe.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, FRAME = 10485760, 256


def _time_ms(torch, fns, reps):
    """-> [(median, min, max, host) per fn]: `reps` rounds of every fn in turn, each between HIP events of its own, after
    three warm-up rounds; host: the median time the host spent in fn (planning, upload and launches enqueued), in ms"""
    st = torch.cuda.current_stream()
    for _ in range(3):
        for fn in fns:
            fn(st.cuda_stream)
    torch.cuda.synchronize()
    ts, hs = [[] for _ in fns], [[] for _ in fns]
    for _ in range(reps):
        for fn, t, h in zip(fns, ts, hs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            t0 = time.perf_counter()
            fn(st.cuda_stream)
            h.append((time.perf_counter() - t0) * 1e3)
            e1.record(st)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t)), float(np.median(h))) for t, h in zip(ts, hs)]


def _state_series(n):
    """five levels, dwell times of 200 .. 3000 samples"""
    rng = np.random.default_rng(83)
    d = rng.integers(200, 3000, n // 200 + 1)
    lv = np.array([0.0, 1.0, 2.0, 3.0, 503.0])[rng.integers(0, 5, len(d))]
    return np.repeat(lv, d)[:n].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--buckets", default="0,60", help="comma-separated bucket lengths in samples (0: one whole-stream window)")
    ap.add_argument("--series", default="noisy,state")
    ap.add_argument("--parent", default="", help="variant name of a parent-commit library to time the existing calls on")
    ap.add_argument("--existing-only", action="store_true", help="(the child of --parent) no value-count call: the library has none")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    from atsc_amd import capi

    if args.existing_only:
        for k in [k for k in capi.SIGNATURES if "_values_" in k]:  # the parent's library does not export them
            del capi.SIGNATURES[k]
    else:
        import __graft_entry__ as G

        G.build()
    import atsc_amd as A
    from tests import extremes_model as EM
    from tests import helpers as H
    from tests import values_model as VM

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    me5 = float(np.float32(5) / np.float32(100))
    off = H.frame_offsets(N, FRAME)
    res = []
    for series in args.series.split(","):
        if series == "noisy":
            recs, _, chosen, _ = ctx.compress_host(H.synth_series(0, N), off, A.AUTO, True, me5, 0)
        else:
            recs, _, chosen, _ = ctx.compress_host(_state_series(N), off, A.AUTO, True, 0.0, 0)
        tags = {A.capi.COMPRESSOR_NAMES[int(t)]: int(c) for t, c in zip(*np.unique(chosen, return_counts=True))}
        dp = A.DPlan(ctx, recs)
        body = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        d_full = torch.empty(N, dtype=torch.float64, device=dev)
        dp.decompress(body, d_full, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        full = d_full.cpu().numpy()
        del d_full
        for bk in [int(v) or N for v in args.buckets.split(",")]:
            bb, bc = A.bucket_windows(0, N, bk)
            oo = np.concatenate([[0], np.cumsum(bc)[:-1]]).astype(np.uint64)
            d_v4 = torch.empty(len(bb) * (4 + 2 * 4), dtype=torch.int64, device=dev)
            d_v32 = torch.empty(len(bb) * (4 + 2 * 32), dtype=torch.int64, device=dev)
            d_e = torch.empty(len(bb) * (2 + 4 * 16), dtype=torch.int64, device=dev)
            d_s = torch.empty(N, dtype=torch.float64, device=dev)
            fns = [lambda s: dp.extremes_windows(body, bb, bc, 16, d_e, s), lambda s: dp.decompress_windows(body, bb, bc, d_s, oo, s)]
            names = ["extremes", "decode"]
            if not args.existing_only:
                fns = [lambda s: dp.values_windows(body, bb, bc, 4, d_v4, stream=s),
                       lambda s: dp.values_windows(body, bb, bc, 32, d_v32, stream=s)] + fns
                names = ["values4", "values32"] + names
            row = {"series": series, "frames": tags, "bucket": bk, "windows": len(bb), "reps": args.reps,
                   "library": capi.LIB_PATH.split(os.sep)[-1]}
            for name, (med, lo, hi, host) in zip(names, _time_ms(torch, fns, args.reps)):
                row.update({name + "_ms_median": med, name + "_ms_min": lo, name + "_ms_max": hi, name + "_host_ms_median": host})
            some = sorted({0, len(bb) // 2, len(bb) - 1})  # spot checks against the models
            wins = [(int(bb[k]), int(bc[k])) for k in some]
            got = d_e.cpu().numpy().view(A.window_extremes_dtype(16))[some]
            assert np.array_equal(EM.words(got), EM.words(EM.windows_extremes(full, wins, 16))), (series, bk)
            if not args.existing_only:
                for k, d in ((4, d_v4), (32, d_v32)):
                    got = d.cpu().numpy().view(A.window_values_dtype(k))
                    assert np.array_equal(VM.words(got[some]), VM.words(VM.windows_values(full, wins, k))), (series, bk, k)
                    row["values%d_more_windows" % k] = int((got["more"] != 0).sum())
                for name in ("values4", "values32"):
                    row[name + "_over_extremes"] = row[name + "_ms_median"] / row["extremes_ms_median"]
                    row[name + "_over_decode"] = row[name + "_ms_median"] / row["decode_ms_median"]
            print(json.dumps(row), flush=True)
            res.append(row)
            del d_v4, d_v32, d_e, d_s
        dp.close()
        del body
    ctx.close()
    if args.parent:  # fresh processes, one library each: this build's existing calls like for like with the parent's
        for variant in ("", args.parent, "", args.parent):
            env = dict(os.environ, ATSC_LIB_VARIANT=variant)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-only", "--reps", str(args.reps), "--buckets",
                                args.buckets, "--series", args.series],
                               env=env, capture_output=True, text=True, timeout=900)
            sys.stderr.write(r.stderr)
            assert r.returncode == 0, r.returncode
            for line in r.stdout.splitlines():
                print(line, flush=True)
                res.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
