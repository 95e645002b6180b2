"""Windowed runs probe (atsc_runs_windows_dev) on one GPU.

Per shape, the runs call's time beside atsc_delta_windows_dev and atsc_aggregate_windows_dev on the same plan and
windows -- the same decode and host planning, one pass over the same scratch, a different reduce.  The three calls are
timed in turn in one process (HIP events around each device call, so host task planning is inside: call time, not kernel
time):
  bench     the bench's batch (10,485,760 samples, 40960 frames x 256, auto e = 5 %)
  chunker   the reference chunker's framing (80 x 131072, auto e = 5 %)
each with one whole-stream window and whole-stream buckets of 65536, 1024 and 60 samples, under the condition
x > median of the decode.  A few windows of every result are checked against the NumPy model.  Prints one JSON object per
shape; --out FILE also writes them there.  Kernel-only times come from a rocprofv3 --kernel-trace --stats run of this
probe.

    python tools/runs_probe.py [--reps 20] [--out profiles/runs_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_round_ms(torch, fns, reps):
    """-> (median, min, max) of every fn: `reps` rounds of the fns in turn, each call between HIP events of its own,
    after two warm-up rounds"""
    st = torch.cuda.current_stream()
    for _ in range(2):
        for fn in fns:
            fn(st.cuda_stream)
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn(st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
    return [(float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip", default="", help="comma-separated shapes to leave out (bench, chunker)")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import helpers as H
    from tests import runs_model as M

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

    def case(name, seed, n, fl):
        recs = ctx.compress_host(H.synth_series(seed, n), H.frame_offsets(n, fl), A.AUTO, True, me5, 0)[0]
        dp = A.DPlan(ctx, recs)
        d_body = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        d_full = torch.empty(n, dtype=torch.float64, device=dev)
        dp.decompress(d_body, d_full, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ref = d_full.cpu().numpy()
        del d_full
        limit = float(np.median(ref))
        rows = []
        for bk in (n, 65536, 1024, 60):
            bb, bc = A.bucket_windows(0, n, bk)
            d_st = torch.empty(len(bb) * 6, dtype=torch.int64, device=dev)
            d_dl = torch.empty(len(bb) * 8, dtype=torch.int64, device=dev)
            d_rn = torch.empty(len(bb) * 10, dtype=torch.int64, device=dev)
            (rms, rmn, rmx), (dms, dmn, dmx), (ams, amn, amx) = _time_round_ms(
                torch, [lambda s: dp.runs_windows(d_body, bb, bc, A.RUNS_GT, limit, d_rn, s),
                        lambda s: dp.delta_windows(d_body, bb, bc, d_dl, s),
                        lambda s: dp.aggregate_windows(d_body, bb, bc, d_st, s)], args.reps)
            got = d_rn.cpu().numpy().view(A.WINDOW_RUNS)
            st = d_st.cpu().numpy().view(A.WINDOW_STATS)
            assert np.array_equal(got["samples"], st["count"])  # (the probe's data holds no NaN)
            for k in sorted({0, len(bb) // 2, len(bb) - 1}):  # spot check against the model
                want = M.windows_runs(ref, [(int(bb[k]), int(bc[k]))], M.GT, limit)
                assert got[k:k + 1].tobytes() == want.tobytes(), (name, bk, k, got[k], want[0])
            rows.append({"bucket": bk, "windows": len(bb), "runs_ms_median": rms, "runs_ms_min": rmn, "runs_ms_max": rmx,
                         "delta_ms_median": dms, "delta_ms_min": dmn, "delta_ms_max": dmx,
                         "aggregate_ms_median": ams, "aggregate_ms_min": amn, "aggregate_ms_max": amx,
                         "x_aggregate": rms / ams, "x_delta": rms / dms,
                         "runs_total": int(got["runs"].sum()), "longest_max": int(got["longest"].max())})
            del d_st, d_dl, d_rn
        emit({"shape": name, "samples": n, "frame": fl, "reps": args.reps, "limit": limit, "rows": rows})
        dp.close()

    if "bench" not in skip:
        case("bench", 0, 10485760, 256)
    if "chunker" not in skip:
        case("chunker", 1, 80 * 131072, 131072)
    ctx.close()


if __name__ == "__main__":
    main()
