"""Windowed across moments probe (atsc_across_moments_windows_dev) on one GPU.

The streams of tools/across_probe.py: N plans over eight series of the bench's framing (10,485,760 samples, 40960 frames
x 256, auto e = 5 %; stream k being series k % 8 with a plan of its own), queried as one whole-stream range at stride 1.
Per N two calls are timed alternately in one process, after warm-up rounds, each between HIP events of its own around
the device call (host task planning is inside: call time, not kernel time), and reported as median, min and max over
--reps rounds, with the median time the host spent inside the call beside them:
  moments   one atsc_across_moments_windows_dev call over the N plans
  across    one atsc_across_windows_dev call over the same plans and range: it plans and decodes the same pieces, so the
            difference between the two is the merge chain (a divide per stream) against the fold of min, max and sum
            (and 24 against 32 bytes per record)
and beside them the floor: (8 N + 24) bytes per position -- the kernel's reads and its records, without the decode --
at --rate TB/s (6.3: what a streaming copy reaches on an MI355X, profiles/across_timing.txt).
A few stretches of the result are checked against the NumPy model, bit for bit.

Each N runs in a child process of its own under a time limit (--limit seconds): this process never opens the GPU, and a
child that fails or runs out of time ends the probe.  Prints one JSON object per N; --out FILE also writes them there.

    python tools/across_moments_probe.py [--reps 20] [--streams 8,64] [--budget BYTES] [--limit 600] [--out FILE]
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

N, FRAME, SERIES = 10485760, 256, 8


def _time_ms(torch, fns, reps):
    """-> [(median, min, max, host) per fn]: `reps` rounds of every fn in turn, each between HIP events of its own, after
    two warm-up rounds; host: the median time the host spent in fn (planning, upload and launches enqueued), in ms"""
    st = torch.cuda.current_stream()
    for _ in range(2):
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


def child(ns, reps, budget, rate):
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import across_moments_model as M
    from tests import helpers as H

    ctx = A.Context(0)
    ctx.set_aggregate_scratch(budget)  # (0: the default)
    dev = torch.device("cuda:0")
    me5 = float(np.float32(5) / np.float32(100))
    off = H.frame_offsets(N, FRAME)
    recs = [ctx.compress_host(H.synth_series(k, N), off, A.AUTO, True, me5, 0)[0] for k in range(min(ns, SERIES))]
    bodies = [torch.frombuffer(bytearray(r), dtype=torch.uint8).to(dev) for r in recs]
    dps = [A.DPlan(ctx, recs[k % SERIES]) for k in range(ns)]
    bds = [bodies[k % SERIES] for k in range(ns)]
    d_rec = torch.empty(4 * N, dtype=torch.int64, device=dev)
    d_mom = torch.empty(3 * N, dtype=torch.int64, device=dev)
    d_s = torch.empty(N, dtype=torch.float64, device=dev)
    b, c = [0], [N]
    fulls = []
    for k in range(min(ns, SERIES)):
        dps[k].decompress(bds[k], d_s, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        fulls.append(d_s.cpu().numpy().copy())
    del d_s

    def across(s):
        dps[0].across_windows(bds[0], dps[1:], bds[1:], b, c, d_rec, 1, s)

    def moments(s):
        dps[0].across_moments_windows(bds[0], dps[1:], bds[1:], b, c, d_mom, 1, s)

    (mm, mlo, mhi, mh), (am, alo, ahi, ah) = _time_ms(torch, [moments, across], reps)
    # spot check against the model: a few stretches of the records
    moments(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for at in (0, 2047, N // 2 + 1, N - 300):
        got = d_mom[3 * at: 3 * (at + 300)].cpu().numpy().view(M.dtype).reshape(-1)
        want = M.records(np.stack([fulls[j % SERIES][at:at + 300] for j in range(ns)]))
        assert M.same(got, want), (ns, at)
    row = {"streams": ns, "positions": N, "reps": reps, "budget_bytes": budget, "moments_ms_median": mm, "moments_ms_min": mlo,
           "moments_ms_max": mhi, "moments_host_ms_median": mh, "across_ms_median": am, "across_ms_min": alo,
           "across_ms_max": ahi, "across_host_ms_median": ah, "moments_minus_across_ms": mm - am, "moments_over_across": mm / am,
           "floor_ms": (8 * ns + 24) * N / (rate * 1e12) * 1e3}
    print(json.dumps(row), flush=True)
    for dp in dps:
        dp.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--streams", default="8,64", help="comma-separated numbers of streams, one child process each")
    ap.add_argument("--limit", type=int, default=600, help="seconds a child may take")
    ap.add_argument("--budget", type=int, default=0, help="atsc_ctx_set_aggregate_scratch of the children, bytes (0: the default)")
    ap.add_argument("--rate", type=float, default=6.3, help="the streaming rate of the floor, TB/s")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", type=int, default=0, help="(internal) run this number of streams in this process")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps, args.budget, args.rate)
    res = []
    for ns in [int(v) for v in args.streams.split(",")]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(ns), "--reps", str(args.reps),
                            "--budget", str(args.budget), "--rate", str(args.rate)], capture_output=True, text=True,
                           timeout=args.limit)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            sys.exit("the child for %d streams ended with %d: nothing more is started" % (ns, r.returncode))
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                res.append(json.loads(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
