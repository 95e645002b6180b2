"""Windowed extremes probe (atsc_extremes_windows_dev) on one GPU.

Per shape, the extremes call's time at k = 1, 4 and 16 beside atsc_runs_windows_dev and atsc_aggregate_windows_dev on the
same plan and windows -- the same decode and host planning, one pass over the same scratch, a different reduce.  The
aggregate call is the yardstick.  The five calls are timed in turn in one process (HIP events around each device call,
so host task planning is inside: call time, not kernel time):
  bench      the bench's batch (10,485,760 samples, 40960 frames x 256, auto e = 5 %)
  chunker    the reference chunker's framing (80 x 131072, auto e = 5 %)
  ascending  an ascending integer counter, Noop frames of 256: every sample beats all before it
  one_lane   in every tile of 2048 samples one lane's 32 slots hold the tile's top, Noop frames of 256
each with one whole-stream window and whole-stream buckets of 65536, 1024 and 60 samples.  The last two streams are the
inputs the tile kernel's bound on insertions is about.  A few windows of every result are checked against the NumPy model.
Prints one JSON object per shape; --out FILE also writes them there.  Kernel-only times come from a
rocprofv3 --kernel-trace --stats run of this probe.

    python tools/extremes_probe.py [--reps 20] [--out profiles/extremes_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.runs_probe import _time_round_ms  # noqa: E402

KS = (1, 4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip", default="", help="comma-separated shapes to leave out (bench, chunker, ascending, one_lane)")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import extremes_model as M
    from tests import helpers as H

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

    def case(name, x, fl, comp):
        n = len(x)
        recs = ctx.compress_host(x, H.frame_offsets(n, fl), comp, comp == A.AUTO, me5 if comp == A.AUTO else 0.0, 0)[0]
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
            d_rn = torch.empty(len(bb) * 10, dtype=torch.int64, device=dev)
            d_ex = {k: torch.empty(len(bb) * (2 + 4 * k), dtype=torch.int64, device=dev) for k in KS}
            fns = [lambda s, k=k: dp.extremes_windows(d_body, bb, bc, k, d_ex[k], s) for k in KS]
            fns += [lambda s: dp.runs_windows(d_body, bb, bc, A.RUNS_GT, limit, d_rn, s),
                    lambda s: dp.aggregate_windows(d_body, bb, bc, d_st, s)]
            t = _time_round_ms(torch, fns, args.reps)
            st = d_st.cpu().numpy().view(A.WINDOW_STATS)
            row = {"bucket": bk, "windows": len(bb)}
            for k, (ms, mn, mx) in zip(KS, t):
                got = d_ex[k].cpu().numpy().view(A.window_extremes_dtype(k))
                assert np.array_equal(got["count"] - got["nans"], st["count"])
                for i in sorted({0, len(bb) // 2, len(bb) - 1}):  # spot check against the model
                    want = M.windows_extremes(ref, [(int(bb[i]), int(bc[i]))], k)
                    assert np.array_equal(M.words(got[i:i + 1]), M.words(want)), (name, bk, k, i, got[i], want[0])
                row.update({"k%d_ms_median" % k: ms, "k%d_ms_min" % k: mn, "k%d_ms_max" % k: mx,
                            "k%d_x_aggregate" % k: ms / t[-1][0]})
            for nm, (ms, mn, mx) in zip(("runs", "aggregate"), t[len(KS):]):
                row.update({nm + "_ms_median": ms, nm + "_ms_min": mn, nm + "_ms_max": mx})
            rows.append(row)
            del d_st, d_rn, d_ex
        emit({"shape": name, "samples": n, "frame": fl, "reps": args.reps, "rows": rows})
        dp.close()

    n = 10485760
    if "bench" not in skip:
        case("bench", H.synth_series(0, n), 256, A.AUTO)
    if "chunker" not in skip:
        case("chunker", H.synth_series(1, 80 * 131072), 131072, A.AUTO)
    if "ascending" not in skip:
        case("ascending", np.arange(n, dtype=np.float64), 256, A.NOOP)
    if "one_lane" not in skip:
        rng = np.random.default_rng(7)
        x = rng.integers(0, 1000, n).astype(np.float64).reshape(-1, 2048)
        lane = [512 * q + 2 * (5 + 64 * kk) + e for q in range(4) for kk in range(4) for e in range(2)]
        x[:, lane] = 10000.0 + rng.permuted(np.tile(np.arange(32.0), (len(x), 1)), axis=1)
        case("one_lane", x.reshape(-1), 256, A.NOOP)
    ctx.close()


if __name__ == "__main__":
    main()
