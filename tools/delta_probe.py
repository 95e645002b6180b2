"""Windowed deltas probe (atsc_delta_windows_dev) on one GPU.

Per shape, the delta call's time beside atsc_aggregate_windows_dev on the same plan and windows -- the same decode and
host planning, one pass over the same scratch, a different reduce.  The two calls are timed alternately in one process (HIP events around each device
call, so host task planning is inside: call time, not kernel time):
  bench     the bench's batch (10,485,760 samples, 40960 frames x 256, auto e = 5 %)
  chunker   the reference chunker's framing (80 x 131072, auto e = 5 %)
each with one whole-stream window and whole-stream buckets of 65536, 1024 and 60 samples.  A few windows of every
result are checked against the NumPy model.  Prints one JSON object per shape; --out FILE also writes them there.
Kernel-only times come from a rocprofv3 --kernel-trace --stats run of this probe.

    python tools/delta_probe.py [--reps 20] [--out profiles/delta_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_pair_ms(torch, fa, fb, reps):
    """-> ((median, min, max) of fa, the same of fb): `reps` rounds of fa then fb, each between HIP events of its own,
    after two warm-up rounds"""
    st = torch.cuda.current_stream()
    for _ in range(2):
        fa(st.cuda_stream)
        fb(st.cuda_stream)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            fn(st.cuda_stream)
            e1.record(st)
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    return tuple((float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in (ta, tb))


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
    from tests import delta_model as M

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
        rows = []
        for bk in (n, 65536, 1024, 60):
            bb, bc = A.bucket_windows(0, n, bk)
            d_st = torch.empty(len(bb) * 6, dtype=torch.int64, device=dev)
            d_dl = torch.empty(len(bb) * 8, dtype=torch.int64, device=dev)
            (ams, amn, amx), (dms, dmn, dmx) = _time_pair_ms(
                torch, lambda s: dp.aggregate_windows(d_body, bb, bc, d_st, s),
                lambda s: dp.delta_windows(d_body, bb, bc, d_dl, s), args.reps)
            got = d_dl.cpu().numpy().view(A.WINDOW_DELTA)
            st = d_st.cpu().numpy().view(A.WINDOW_STATS)
            assert np.array_equal(got["pairs"], np.maximum(st["count"], 1) - 1)  # (the probe's data holds no NaN)
            for k in sorted({0, len(bb) // 2, len(bb) - 1}):  # spot check against the model
                want = M.windows_delta(ref, [(int(bb[k]), int(bc[k]))])
                assert got[k:k + 1].tobytes() == want.tobytes(), (name, bk, k, got[k], want[0])
            rows.append({"bucket": bk, "windows": len(bb), "delta_ms_median": dms, "delta_ms_min": dmn,
                         "delta_ms_max": dmx, "aggregate_ms_median": ams, "aggregate_ms_min": amn,
                         "aggregate_ms_max": amx, "x_aggregate": dms / ams})
            del d_st, d_dl
        emit({"shape": name, "samples": n, "frame": fl, "reps": args.reps, "rows": rows})
        dp.close()

    if "bench" not in skip:
        case("bench", 0, 10485760, 256)
    if "chunker" not in skip:
        case("chunker", 1, 80 * 131072, 131072)
    ctx.close()


if __name__ == "__main__":
    main()
