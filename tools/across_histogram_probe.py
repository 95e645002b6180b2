"""Windowed across histograms probe (atsc_across_histogram_windows_dev) on one GPU.

Eight streams of 2^20 samples (4096 frames x 256, auto e = 5 %), listed in turn to make N of them.  Per shape
(N, n_edges, positions, stride) one range is queried three ways, timed alternately in one process after warm-up rounds,
each between HIP events of its own around the device calls (host planning is inside: call time, not kernel time), and
reported as median, min and max over --reps rounds, with the median time the host spent inside beside them:
  histogram one atsc_across_histogram_windows_dev call over the N plans
  route     what a caller does without it: N atsc_histogram_windows_dev calls, one per stream, over the explicitly listed
            one-sample windows of the same positions, each added to an accumulator on the device (torch add_)
  moments   one atsc_across_moments_windows_dev call of the same range and stride: another fold of the same N samples
The new call's rows are checked against the route's sum, byte for byte, and a few rows against the NumPy model.  Beside
the times: the bytes of the rows, 8 (n_edges + 2) positions, over the new call's median time, to hold against the
about 6.3 TB/s a streaming store reaches on this GPU (the call also decodes N streams: this is not a kernel's share of peak).
Prints one JSON object per shape; --out FILE also writes them.

    python tools/across_histogram_probe.py [--reps 7] [--shapes 8:10:1000000:1,64:10:1000000:1,64:1024:100000:1,64:10:66667:15]
                                           [--no-route] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rolling_probe import FRAME, _time_ms  # noqa: E402

SAMPLES = 1 << 20
SERIES = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="8:10:1000000:1,64:10:1000000:1,64:1024:100000:1,64:10:66667:15",
                    help="comma-separated N:N_EDGES:POSITIONS:STRIDE")
    ap.add_argument("--no-route", action="store_true", help="skip the route (for a kernel trace of the new call: a run of its own)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import across_histogram_model as M
    from tests import helpers as H

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    me5 = float(np.float32(5) / np.float32(100))
    recs = [ctx.compress_host(H.synth_series(k, SAMPLES), H.frame_offsets(SAMPLES, FRAME), A.AUTO, True, me5, 0)[0]
            for k in range(SERIES)]
    dps = [A.DPlan(ctx, r) for r in recs]
    bodies = [torch.frombuffer(bytearray(r), dtype=torch.uint8).to(dev) for r in recs]
    fulls = []
    d_full = torch.empty(SAMPLES, dtype=torch.float64, device=dev)
    for dp, body in zip(dps, bodies):
        dp.decompress(body, d_full, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        fulls.append(d_full.cpu().numpy().copy())
    distinct = np.unique(np.concatenate([f[:: 64] for f in fulls]))
    closed = A.HIST_RIGHT_CLOSED
    res = []
    for shape in args.shapes.split(","):
        n, n_edges, m, s = (int(v) for v in shape.split(":"))
        count = (m - 1) * s + 1
        assert 1 <= n <= A.ACROSS_MAX_STREAMS and count <= SAMPLES and A.across_offsets([count], s)[-1] == m
        if n_edges <= 64:  # `le`-style edges: the streams' own quantiles (distinct values), +Inf last
            q = np.linspace(0.05, 0.95, n_edges - 1) if n_edges > 1 else np.zeros(0)
            edges = np.concatenate([distinct[np.round(q * (len(distinct) - 1)).astype(np.int64)], [np.inf]])
        else:
            edges = np.linspace(float(distinct[len(distinct) // 100]), float(distinct[-len(distinct) // 100]), n_edges)
        assert len(edges) == n_edges and np.all(np.diff(edges) > 0)
        rows = n_edges + 2
        order = [k % SERIES for k in range(n)]
        lo = (s * np.arange(m)).astype(np.uint64)
        one = np.ones(m, dtype=np.uint64)
        d_new = torch.empty(rows * m, dtype=torch.int64, device=dev)
        d_sum = torch.empty(rows * m, dtype=torch.int64, device=dev)
        d_one = torch.empty(rows * m, dtype=torch.int64, device=dev)
        d_mom = torch.empty(3 * m, dtype=torch.int64, device=dev)

        def route(st):
            d_sum.zero_()
            for k in order:
                dps[k].histogram_windows(bodies[k], lo, one, edges, d_one, closed, st)
                d_sum.add_(d_one)

        fns = [lambda st: dps[order[0]].across_histogram_windows(bodies[order[0]], [dps[k] for k in order[1:]],
                                                                 [bodies[k] for k in order[1:]], [0], [count], edges, d_new, s,
                                                                 closed, st),
               route,
               lambda st: dps[order[0]].across_moments_windows(bodies[order[0]], [dps[k] for k in order[1:]],
                                                               [bodies[k] for k in order[1:]], [0], [count], d_mom, s, st)]
        row = {"n_streams": n, "n_edges": n_edges, "positions": m, "stride": s, "range": count, "reps": args.reps,
               "rows_a_pass": M.rows_a_pass(n_edges), "row_bytes": 8 * rows * m}
        names = ("histogram", "route", "moments")
        if args.no_route:
            fns, names = [fns[0], fns[2]], ("histogram", "moments")
        for name, (med, tlo, thi, host) in zip(names, _time_ms(torch, fns, args.reps)):
            row.update({name + "_ms_median": med, name + "_ms_min": tlo, name + "_ms_max": thi, name + "_host_ms_median": host})
        got = d_new.cpu().numpy().view(np.uint64).reshape(m, rows)
        assert args.no_route or got.tobytes() == d_sum.cpu().numpy().tobytes(), shape
        at = np.array(sorted({0, 1, m // 3, m // 2, m - 1}), dtype=np.int64)
        want = M.rows(np.array([fulls[k][s * at] for k in order]), edges, closed)
        assert np.array_equal(got[at], want), (shape, got[at], want)
        assert np.all(got.sum(axis=1) == n)
        if not args.no_route:
            row["histogram_over_route"] = row["histogram_ms_median"] / row["route_ms_median"]
        row["histogram_over_moments"] = row["histogram_ms_median"] / row["moments_ms_median"]
        row["row_bytes_per_s_TB"] = row["row_bytes"] / (row["histogram_ms_median"] * 1e-3) / 1e12
        print(json.dumps(row), flush=True)
        res.append(row)
        del d_new, d_sum, d_one, d_mom
    for dp in dps:
        dp.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
