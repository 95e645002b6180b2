"""Windowed pair matrix probe (atsc_pair_matrix_windows_dev) on one GPU.

Eight series of 2^20 samples (4096 frames x 256, auto e = 5 %), listed in turn to make N streams, each with a decode plan
of its own.  Per shape (N, windows, window length) the windows are queried two ways, timed alternately in one process
after two warm-up rounds, each between HIP events of its own around the device calls (host planning is inside: call time,
not kernel time), and reported as median, min and max over --reps rounds, with the median time the host spent inside:
  matrix  one atsc_pair_matrix_windows_dev call over the N plans
  route   what a caller does without it: P = N (N + 1) / 2 atsc_pair_windows_dev calls over the same plans, one per pair,
          the diagonal included
The new call's records are checked against the route's, byte for byte (any NaN equal to any NaN), and a few against the
NumPy model.  Beside the times: the f64 operations of the tile merges, 19 per Merge (the equal-count form: 8 multiplies,
11 adds) and 2047 Merges per pair and tile, over the new call's median time -- a call's rate, not a kernel's share of
peak (the call also decodes N streams; tools/README.md says how the kernel's own time is taken).
Prints one JSON object per shape; --out FILE also writes them.

    python tools/pair_matrix_probe.py [--reps 7] [--route-reps 7] [--shapes 8:1:1048576,64:1:1048576,8:1440:728,64:1440:728]
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
TILE = 2048
MERGE_OPS = 19


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--route-reps", type=int, default=7, help="rounds of the route where they differ from --reps (1: no warm-up either)")
    ap.add_argument("--shapes", default="8:1:1048576,64:1:1048576,8:1440:728,64:1440:728", help="comma-separated N:WINDOWS:LENGTH")
    ap.add_argument("--no-route", action="store_true", help="skip the route (for a kernel trace of the new call: a run of its own)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import helpers as H
    from tests import pair_matrix_model as PM

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    me5 = float(np.float32(5) / np.float32(100))
    recs = [ctx.compress_host(H.synth_series(k, SAMPLES), H.frame_offsets(SAMPLES, FRAME), A.AUTO, True, me5, 0)[0]
            for k in range(SERIES)]
    bodies8 = [torch.frombuffer(bytearray(r), dtype=torch.uint8).to(dev) for r in recs]
    fulls = [ctx.decompress_host(r) for r in recs]
    res = []
    for shape in args.shapes.split(","):
        n, w, length = (int(v) for v in shape.split(":"))
        assert 1 <= n <= A.ACROSS_MAX_STREAMS and w * length <= SAMPLES
        p = A.pair_matrix_records(n)
        dps = [A.DPlan(ctx, recs[k % SERIES]) for k in range(n)]
        bodies = [bodies8[k % SERIES] for k in range(n)]
        b = (np.arange(w, dtype=np.uint64) * np.uint64(length)).astype(np.uint64)
        c = np.full(w, length, dtype=np.uint64)
        d_new = torch.empty(w * p * 6, dtype=torch.int64, device=dev)
        d_route = torch.empty((p, w * 6), dtype=torch.int64, device=dev)

        def matrix(st):
            dps[0].pair_matrix_windows(bodies[0], dps[1:], bodies[1:], b, c, d_new, st)

        def route(st):
            for i, j in PM.pairs(n):
                dps[i].pair_windows(bodies[i], dps[j], bodies[j], b, c, d_route[PM.index(n, i, j)], st)

        tiles = int(sum((int(x) + int(y) - 1) // TILE - int(x) // TILE + 1 for x, y in zip(b, c)))  # tile tasks, none shared here
        row = {"n_streams": n, "pairs": p, "windows": w, "length": length, "reps": args.reps, "tile_tasks": tiles}
        rr = args.route_reps
        both = not args.no_route and rr == args.reps  # the two in turn, round by round
        timed = _time_ms(torch, [matrix, route] if both else [matrix], args.reps)
        med, tlo, thi, host = timed[0]
        row.update({"matrix_ms_median": med, "matrix_ms_min": tlo, "matrix_ms_max": thi, "matrix_host_ms_median": host})
        if not args.no_route:
            if both:
                med, tlo, thi, host = timed[1]
            elif rr > 1:
                med, tlo, thi, host = _time_ms(torch, [route], rr)[0]
            else:  # one round, no warm-up: the route's first call pays what first calls pay
                st = torch.cuda.current_stream()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                import time

                e0.record(st)
                t0 = time.perf_counter()
                route(st.cuda_stream)
                host = (time.perf_counter() - t0) * 1e3
                e1.record(st)
                torch.cuda.synchronize()
                med = tlo = thi = e0.elapsed_time(e1)
            row.update({"route_reps": rr, "route_ms_median": med, "route_ms_min": tlo, "route_ms_max": thi,
                        "route_host_ms_median": host, "matrix_over_route": row["matrix_ms_median"] / med})
            matrix(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            got = d_new.cpu().numpy().view(np.uint64).reshape(w, p, 6)
            want = np.ascontiguousarray(d_route.cpu().numpy().view(np.uint64).reshape(p, w, 6).transpose(1, 0, 2))
            same = (got == want) | (np.isnan(got.view(np.float64)) & np.isnan(want.view(np.float64)))
            same[..., 0] = got[..., 0] == want[..., 0]
            assert bool(same.all()), shape
        got = d_new.cpu().numpy().view(A.WINDOW_PAIR).reshape(w, p)
        only = sorted({(0, 0), (0, n - 1), (n - 1, n - 1), (n // 2, n - 1)})
        at = sorted({0, w // 2, w - 1})
        wins = [(int(b[k]), int(c[k])) for k in at]
        want = PM.windows_pair_matrix([fulls[k % SERIES] for k in range(n)], wins, only)
        for i, j in only:
            q = PM.index(n, i, j)
            assert got[at, q].tobytes() == want[:, q].astype(A.WINDOW_PAIR).tobytes(), (shape, i, j)
        ops = MERGE_OPS * (TILE - 1) * p * tiles
        row["merge_f64_ops"] = ops
        row["merge_f64_Tops_per_s"] = ops / (row["matrix_ms_median"] * 1e-3) / 1e12
        print(json.dumps(row), flush=True)
        res.append(row)
        for dp in dps:
            dp.close()
        del d_new, d_route
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
