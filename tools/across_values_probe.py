"""Windowed across value counts probe (atsc_across_values_windows_dev) on one GPU.

Eight state-like streams of 2^20 samples (the rounded values of slow waves with noise, about seven levels each; 4096
frames x 256, Noop: kept exactly, so that columns repeat), listed in turn to make N of them.  Per shape
(N, k, positions, stride) one range is queried three ways, timed alternately in one process after warm-up rounds, each
between HIP events of its own around the device calls (host planning is inside: call time, not kernel time), and
reported as median, min and max over --reps rounds, with the median time the host spent inside beside them:
  values    one atsc_across_values_windows_dev call over the N plans
  route     what a caller does without it: N atsc_values_windows_dev calls, one per stream, over the explicitly listed
            one-sample windows of the same positions (at most --route-positions of them: the time is scaled to the
            shape's positions and the row says so), then, outside the events and timed once by the wall clock, the
            records' way back to the host and one atsc_values_merge per position over the N records
  extremes  one atsc_across_extremes_windows_dev call of the same range and stride at the k (at most 16) whose record is
            nearest in size: another fold of the same N samples
The new call's records are checked against the route's merged records, byte for byte, and a few against the NumPy model.
Beside the times: the bytes of the records, (32 + 16 k) positions, over the new call's median time, to hold against the
about 6.3 TB/s a streaming store reaches on this GPU (the call also decodes N streams: this is not a kernel's share of
peak).  Prints one JSON object per shape; --out FILE also writes them.

    python tools/across_values_probe.py [--reps 7] [--shapes 8:4:1000000:1,64:4:1000000:1,64:32:100000:1,64:4:66667:15]
                                        [--route-positions 20000] [--no-route] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rolling_probe import FRAME, _time_ms  # noqa: E402

SAMPLES = 1 << 20
SERIES = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="8:4:1000000:1,64:4:1000000:1,64:32:100000:1,64:4:66667:15",
                    help="comma-separated N:K:POSITIONS:STRIDE")
    ap.add_argument("--route-positions", type=int, default=20000, help="the most positions the route is run over")
    ap.add_argument("--no-route", action="store_true", help="skip the route (for a kernel trace of the new call: a run of its own)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import across_values_model as M
    from tests import helpers as H

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    t = np.arange(SAMPLES)
    recs, fulls = [], []
    for j in range(SERIES):
        x = np.rint(2.5 * np.sin(t / (5000.0 + 1300 * j) + j) + 0.3 * rng.normal(0, 1, SAMPLES)) + 0.0
        recs.append(ctx.compress_host(x, H.frame_offsets(SAMPLES, FRAME), A.NOOP, False, 0.0, 0)[0])
    dps = [A.DPlan(ctx, r) for r in recs]
    bodies = [torch.frombuffer(bytearray(r), dtype=torch.uint8).to(dev) for r in recs]
    d_full = torch.empty(SAMPLES, dtype=torch.float64, device=dev)
    for dp, body in zip(dps, bodies):
        dp.decompress(body, d_full, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        fulls.append(d_full.cpu().numpy().copy())
    res = []
    for shape in args.shapes.split(","):
        n, k, m, s = (int(v) for v in shape.split(":"))
        count = (m - 1) * s + 1
        assert 1 <= n <= A.ACROSS_MAX_STREAMS and count <= SAMPLES and A.across_offsets([count], s)[-1] == m
        size = A.window_values_dtype(k).itemsize
        order = [j % SERIES for j in range(n)]
        mr = min(m, args.route_positions)  # the route's positions: the first mr of the shape's
        lo = (s * np.arange(mr)).astype(np.uint64)
        one = np.ones(mr, dtype=np.uint64)
        ke = min(16, max(1, size // 32))  # 16 + 32 ke bytes nearest to 32 + 16 k
        d_new = torch.empty(size * m, dtype=torch.uint8, device=dev)
        d_one = torch.empty(n * size * mr, dtype=torch.uint8, device=dev)
        d_ext = torch.empty(A.window_extremes_dtype(ke).itemsize * m, dtype=torch.uint8, device=dev)

        def route(st):
            for i, j in enumerate(order):
                dps[j].values_windows(bodies[j], lo, one, k, d_one[i * size * mr: (i + 1) * size * mr], stream=st)

        first, others, other_bodies = dps[order[0]], [dps[j] for j in order[1:]], [bodies[j] for j in order[1:]]
        fns = [lambda st: first.across_values_windows(bodies[order[0]], others, other_bodies, [0], [count], k, d_new, s, stream=st),
               route,
               lambda st: first.across_extremes_windows(bodies[order[0]], others, other_bodies, [0], [count], ke, d_ext, s, st)]
        row = {"n_streams": n, "k": k, "positions": m, "stride": s, "range": count, "reps": args.reps, "record_bytes": size * m,
               "extremes_k": ke, "extremes_record_bytes": A.window_extremes_dtype(ke).itemsize * m}
        names = ("values", "route", "extremes")
        if args.no_route:
            fns, names = [fns[0], fns[2]], ("values", "extremes")
        for name, (med, tlo, thi, host) in zip(names, _time_ms(torch, fns, args.reps)):
            row.update({name + "_ms_median": med, name + "_ms_min": tlo, name + "_ms_max": thi, name + "_host_ms_median": host})
        got = d_new.cpu().numpy().view(A.window_values_dtype(k))
        if not args.no_route:
            t0 = time.perf_counter()
            parts = d_one.cpu().numpy().view(A.window_values_dtype(k)).reshape(n, mr)
            merged = np.array([A.values_merge(np.ascontiguousarray(parts[:, p]), k) for p in range(mr)])
            fold = (time.perf_counter() - t0) * 1e3
            assert got[:mr].tobytes() == merged.tobytes(), shape
            scale = m / mr
            row.update({"route_positions": mr, "route_scaled_by": scale, "route_fold_ms": fold,
                        "route_ms_scaled": (row["route_ms_median"] + fold) * scale})
            row["values_over_route"] = row["values_ms_median"] / row["route_ms_scaled"]
        at = np.array(sorted({0, 1, m // 3, m // 2, m - 1}), dtype=np.int64)
        want = M.records(np.array([fulls[j][s * at] for j in order]), k)
        assert got[at].tobytes() == want.tobytes(), (shape, got[at], want)
        assert np.all(got["count"] == n)
        row["values_over_extremes"] = row["values_ms_median"] / row["extremes_ms_median"]
        row["record_bytes_per_s_TB"] = row["record_bytes"] / (row["values_ms_median"] * 1e-3) / 1e12
        print(json.dumps(row), flush=True)
        res.append(row)
        del d_new, d_one, d_ext
    for dp in dps:
        dp.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
