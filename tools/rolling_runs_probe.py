"""Windowed rolling runs probe (atsc_rolling_runs_windows_dev) on one GPU.

The bench's batch (10,485,760 samples, 40960 frames x 256, auto e = 5 %) read as one stream, under the condition
x > the stream's median.  Per shape (width, stride) one range of the stream is queried four ways, timed alternately in one
process after warm-up rounds, each between HIP events of its own around the device call (host task planning is inside:
call time, not kernel time), and reported as median, min and max over --reps rounds, with the median time the host spent
inside the call beside them:
  runs      one atsc_rolling_runs_windows_dev call: the range named once, with the width, the stride and the condition
  explicit  one atsc_runs_windows_dev call over the explicitly listed windows of the same positions (code that this
            query does not touch: it stands for what a caller has to do without it)
  rolling   one atsc_rolling_windows_dev call of the same range, width and stride: a partial of the same size, for scale
  decode    one atsc_decompress_windows_dev call of the range (the samples handed out, no reduction)
The range is the whole stream where the stride keeps the explicit list below --max-positions windows, else the stream's
first --max-positions * stride + width - 1 samples, as tools/rolling_probe.py has it.  The nine integers of every record
are checked against the explicit call's, exactly; excess against its within the sum of the two stated bounds; and a few
records against the NumPy model, bit for bit.  Prints one JSON object per shape; --out FILE also writes them.

    python tools/rolling_runs_probe.py [--reps 9] [--shapes 20:1,300:15,3600:1] [--max-positions 1048576] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rolling_probe import FRAME, N, _time_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="20:1,300:15,3600:1", help="comma-separated WIDTH:STRIDE")
    ap.add_argument("--max-positions", type=int, default=1 << 20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import helpers as H
    from tests import rolling_runs_model as M
    from tests import runs_model as RM

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    me5 = float(np.float32(5) / np.float32(100))
    recs = ctx.compress_host(H.synth_series(0, N), H.frame_offsets(N, FRAME), A.AUTO, True, me5, 0)[0]
    dp = A.DPlan(ctx, recs)
    body = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
    d_full = torch.empty(N, dtype=torch.float64, device=dev)
    dp.decompress(body, d_full, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x = d_full.cpu().numpy().copy()
    assert np.isfinite(x).all()
    op, limit = A.RUNS_GT, float(np.median(x))
    res = []
    for shape in args.shapes.split(","):
        w, s = (int(v) for v in shape.split(":"))
        count = min(N, args.max_positions * s + w - 1)
        m = A.rolling_outputs(count, w, s)
        lo = (s * np.arange(m)).astype(np.uint64)
        cn = np.full(m, w, dtype=np.uint64)
        d_new, d_list = (torch.empty(10 * m, dtype=torch.int64, device=dev) for _ in range(2))
        d_roll = torch.empty(4 * m, dtype=torch.int64, device=dev)
        fns = [lambda st: dp.rolling_runs_windows(body, [0], [count], w, s, op, limit, d_new, st),
               lambda st: dp.runs_windows(body, lo, cn, op, limit, d_list, st),
               lambda st: dp.rolling_windows(body, [0], [count], w, s, d_roll, st),
               lambda st: dp.decompress_windows(body, [0], [count], d_full, [0], st)]
        row = {"width": w, "stride": s, "range": count, "positions": m, "reps": args.reps, "op": "gt", "limit": limit}
        for name, (med, tlo, thi, host) in zip(("runs", "explicit", "rolling", "decode"), _time_ms(torch, fns, args.reps)):
            row.update({name + "_ms_median": med, name + "_ms_min": tlo, name + "_ms_max": thi, name + "_host_ms_median": host})
        got = d_new.cpu().numpy().view(A.WINDOW_RUNS)
        ref = d_list.cpu().numpy().view(A.WINDOW_RUNS)
        for k in RM.FIELDS[:9]:
            assert got[k].tobytes() == ref[k].tobytes(), (shape, k)
        k = (M.bound_factor(w) + RM.bound_factor(w)) * 1.01  # (inside <= w: the explicit call's bound at its largest)
        bad = np.flatnonzero(~(np.abs(got["excess"] - ref["excess"]) <= k * ref["excess"]))
        assert len(bad) == 0, (shape, len(bad), got[bad[0]], ref[bad[0]])
        at = sorted({0, 1, m // 3, m // 2, m - 1})
        want = M.Pyramid(x[:count], op, limit).records(lo[at].astype(np.int64), w)
        assert got[at].tobytes() == want.tobytes(), (shape, got[at], want)
        row.update({"inside_mean": float(got["inside"].mean()), "runs_mean": float(got["runs"].mean()),
                    "all_inside": int((got["inside"] == w).sum())})
        if count < N:  # the new call and the decode alone over the whole stream, which the explicit list does not reach
            mw = A.rolling_outputs(N, w, s)
            d_whole = torch.empty(10 * mw, dtype=torch.int64, device=dev)
            fns = [lambda st: dp.rolling_runs_windows(body, [0], [N], w, s, op, limit, d_whole, st),
                   lambda st: dp.decompress_windows(body, [0], [N], d_full, [0], st)]
            (r_med, r_lo, r_hi, r_host), (d_med, _, _, _) = _time_ms(torch, fns, args.reps)
            assert d_whole.cpu().numpy().view(A.WINDOW_RUNS)[:m].tobytes() == got.tobytes(), shape
            row.update({"whole_positions": mw, "whole_runs_ms_median": r_med, "whole_runs_ms_min": r_lo,
                        "whole_runs_ms_max": r_hi, "whole_runs_host_ms_median": r_host, "whole_decode_ms_median": d_med})
            del d_whole
        row["runs_over_explicit"] = row["runs_ms_median"] / row["explicit_ms_median"]
        row["runs_over_rolling"] = row["runs_ms_median"] / row["rolling_ms_median"]
        row["runs_over_decode"] = row["runs_ms_median"] / row["decode_ms_median"]
        print(json.dumps(row), flush=True)
        res.append(row)
        del d_new, d_list, d_roll
    dp.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
