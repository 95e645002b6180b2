"""Windowed histograms probe (atsc_histogram_windows_dev) on one GPU.

Per shape, the histogram call's time beside atsc_aggregate_windows_dev on the same plan and windows -- the same
decode, a different reduce.  ms_*: HIP events around the device call, so host task planning is inside (call time, not
kernel time); host_ms_median: the host part alone, until the call returns:
  long       one window over 2^26 samples of 256-sample frames
  short      2^20 windows of 64 samples over the same stream
  chunker    80 x 131072-sample frames (the reference chunker's framing) in 1024 windows
each with 16 and with 1024 edges (uniform over the data's range), once on spread data (synthetic series, auto
e = 5 %) and once on a stream of Constant frames, where every sample lands in one bin.  A few rows of every result are
checked against the NumPy model.  Prints one JSON object per case; --out FILE also writes them there.

    python tools/histogram_probe.py [--reps 10] [--out profiles/histogram_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_ms(torch, fn, reps):
    """-> (median, min, max, host median) of `reps` timed calls after two warm-up calls.  The first three are the call
    as a caller sees it: HIP events around it, so the host's task planning and upload staging, during which the GPU
    idles, are inside.  The last is the host part alone: the wall time until the call returns with its work enqueued.
    Kernel-only times come from a rocprofv3 --kernel-trace --stats run of this probe."""
    st = torch.cuda.current_stream()
    for _ in range(2):
        fn(st.cuda_stream)
    torch.cuda.synchronize()
    ts, hs = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        t0 = time.perf_counter()
        fn(st.cuda_stream)
        hs.append((time.perf_counter() - t0) * 1e3)
        e1.record(st)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), float(np.median(hs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip", default="", help="comma-separated shapes to leave out (long, short, chunker)")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import helpers as H
    from tests import hist_model as M

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    res = []

    def emit(d):
        print(json.dumps(d), flush=True)
        res.append(d)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    me5 = float(np.float32(5) / np.float32(100))

    def stream(kind, seed, n, fl):
        if kind == "constant":
            return ctx.compress_host(np.full(n, 3.25), H.frame_offsets(n, fl), A.CONSTANT, False, 0.0, 0)[0]
        return ctx.compress_host(H.synth_series(seed, n), H.frame_offsets(n, fl), A.AUTO, True, me5, 0)[0]

    def case(shape, kind, recs, n, bb, bc):
        dp = A.DPlan(ctx, recs)
        d_body = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        d_full = torch.empty(n, dtype=torch.float64, device=dev)
        full_ms, _, _, _ = _time_ms(torch, lambda s: dp.decompress(d_body, d_full, s), args.reps)
        ref = d_full.cpu().numpy()
        del d_full
        d_st = torch.empty(len(bb) * 6, dtype=torch.int64, device=dev)
        ams, amn, amx, ahost = _time_ms(torch, lambda s: dp.aggregate_windows(d_body, bb, bc, d_st, s), args.reps)
        del d_st
        lo, hi = float(ref.min()), float(ref.max())
        if not hi > lo:
            lo, hi = lo - 1.0, hi + 1.0
        rows = []
        for n_edges in (16, 1024):
            edges = A.histogram_edges_uniform(lo, hi, n_edges - 1)
            nr = n_edges + 2
            d_h = torch.empty(len(bb) * nr, dtype=torch.int64, device=dev)
            ms, mn, mx, host = _time_ms(torch, lambda s: dp.histogram_windows(d_body, bb, bc, edges, d_h, A.HIST_LEFT_CLOSED, s),
                                  args.reps)
            for k in sorted({0, len(bb) // 2, len(bb) - 1}):  # spot check against the model
                got = d_h[k * nr:(k + 1) * nr].cpu().numpy().view(np.uint64)
                want = M.row(ref[int(bb[k]):int(bb[k] + bc[k])], edges, M.LEFT_CLOSED)
                assert np.array_equal(got, want), (shape, kind, n_edges, k)
            del d_h
            rows.append({"edges": n_edges, "ms_median": ms, "ms_min": mn, "ms_max": mx, "host_ms_median": host,
                         "x_aggregate": ms / ams,
                         "x_full_decode": ms / full_ms})
        emit({"shape": shape, "data": kind, "samples": n, "windows": len(bb), "reps": args.reps,
              "full_decode_ms_median": full_ms, "aggregate_ms_median": ams, "aggregate_ms_min": amn,
              "aggregate_ms_max": amx, "aggregate_host_ms_median": ahost, "rows": rows})
        dp.close()

    n_small, n_big = 1 << 26, 80 * 131072
    one = (np.array([0], dtype=np.uint64), np.array([n_small], dtype=np.uint64))
    for kind in ("spread", "constant"):
        if not {"long", "short"} <= skip:
            recs = stream(kind, 0, n_small, 256)
            if "long" not in skip:
                case("long", kind, recs, n_small, *one)
            if "short" not in skip:
                case("short", kind, recs, n_small, *A.bucket_windows(0, n_small, 64))
            del recs
        if "chunker" not in skip:
            case("chunker", kind, stream(kind, 1, n_big, 131072), n_big, *A.bucket_windows(0, n_big, n_big // 1024))
    ctx.close()


if __name__ == "__main__":
    main()
