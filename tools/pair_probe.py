"""Windowed pair moments probe (atsc_pair_windows_dev) on one GPU.

The bench's batch (10,485,760 samples, 40960 frames x 256, auto e = 5 %) as stream X and a second series in the same
framing as stream Y, queried as one whole-stream window and as 1-minute buckets (60 samples).  Per shape three things
are timed alternately in one process, after warm-up rounds, each between HIP events of its own around the device calls
(host task planning is inside: call time, not kernel time), and reported as median, min and max over --reps rounds,
with the median time the host spent inside the calls beside them:
  pair      one atsc_pair_windows_dev call over both plans
  moments   the sum of two atsc_moments_windows_dev calls, one per plan, on the same windows
  decodes   the sum of two atsc_decompress_windows_dev calls of the same windows (the samples handed out, no reduction)
A few windows of every result are checked against the NumPy model.  Kernel-only times come from a
rocprofv3 --kernel-trace --stats run of this probe (--buckets 0 keeps it to the one-window shape).

--parent NAME then runs the moments and decode timings alone in child processes, twice on this build's library and twice
on the side-by-side library libatsc_hip_NAME.so (a build of the parent commit copied next to the package's library;
atsc_amd/capi.py, ATSC_LIB_VARIANT), in turn: the parent has no pair call, so that is its cost of the same answer's two
halves, and this build's figures beside it show what the process and the day add.  Prints one JSON object per shape and
library; --out FILE also writes them there.

    python tools/pair_probe.py [--reps 30] [--buckets 0,60] [--parent parent] [--out profiles/pair_probe.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--buckets", default="0,60", help="comma-separated bucket lengths in samples (0: one whole-stream window)")
    ap.add_argument("--parent", default="", help="variant name of a parent-commit library to time the two halves on")
    ap.add_argument("--halves-only", action="store_true", help="(the child of --parent) no pair call: the library has none")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    from atsc_amd import capi

    if args.halves_only:
        for k in [k for k in capi.SIGNATURES if "_pair_" in k]:  # the parent's library does not export them
            del capi.SIGNATURES[k]
    else:
        import __graft_entry__ as G

        G.build()
    import atsc_amd as A
    from tests import helpers as H
    from tests import pair_model as P

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    me5 = float(np.float32(5) / np.float32(100))
    off = H.frame_offsets(N, FRAME)
    rx = ctx.compress_host(H.synth_series(0, N), off, A.AUTO, True, me5, 0)[0]
    ry = ctx.compress_host(H.synth_series(3, N), off, A.AUTO, True, me5, 0)[0]
    dpx, dpy = A.DPlan(ctx, rx), A.DPlan(ctx, ry)
    bx = torch.frombuffer(bytearray(rx), dtype=torch.uint8).to(dev)
    by = torch.frombuffer(bytearray(ry), dtype=torch.uint8).to(dev)
    full = []
    for dp, b in ((dpx, bx), (dpy, by)):
        d_full = torch.empty(N, dtype=torch.float64, device=dev)
        dp.decompress(b, d_full, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        full.append(d_full.cpu().numpy())
        del d_full
    res = []
    for bk in [int(v) or N for v in args.buckets.split(",")]:
        bb, bc = A.bucket_windows(0, N, bk)
        oo = np.concatenate([[0], np.cumsum(bc)[:-1]]).astype(np.uint64)
        d_p = torch.empty(len(bb) * 6, dtype=torch.int64, device=dev)
        d_mx, d_my = torch.empty_like(d_p), torch.empty_like(d_p)
        d_sx = torch.empty(N, dtype=torch.float64, device=dev)
        d_sy = torch.empty(N, dtype=torch.float64, device=dev)

        def moments(s):
            dpx.moments_windows(bx, bb, bc, d_mx, s)
            dpy.moments_windows(by, bb, bc, d_my, s)

        def decodes(s):
            dpx.decompress_windows(bx, bb, bc, d_sx, oo, s)
            dpy.decompress_windows(by, bb, bc, d_sy, oo, s)

        fns, names = [moments, decodes], ["moments", "decodes"]
        if not args.halves_only:
            fns.insert(0, lambda s: dpx.pair_windows(bx, dpy, by, bb, bc, d_p, s))
            names.insert(0, "pair")
        row = {"bucket": bk, "windows": len(bb), "reps": args.reps, "library": capi.LIB_PATH.split(os.sep)[-1]}
        for name, (med, lo, hi, host) in zip(names, _time_ms(torch, fns, args.reps)):
            row.update({name + "_ms_median": med, name + "_ms_min": lo, name + "_ms_max": hi, name + "_host_ms_median": host})
        if not args.halves_only:
            got = d_p.cpu().numpy().view(A.WINDOW_PAIR)
            mx = d_mx.cpu().numpy().view(A.WINDOW_MOMENTS)
            assert np.array_equal(got["count"], mx["count"])  # no NaN in either stream
            for k in sorted({0, len(bb) // 2, len(bb) - 1}):  # spot check against the model
                want = P.windows_pair(full[0], full[1], [(int(bb[k]), int(bc[k]))])
                assert got[k:k + 1].tobytes() == want.tobytes(), (bk, k, got[k], want[0])
            row["pair_over_moments"] = row["pair_ms_median"] / row["moments_ms_median"]
            row["pair_over_decodes"] = row["pair_ms_median"] / row["decodes_ms_median"]
        print(json.dumps(row), flush=True)
        res.append(row)
        del d_p, d_mx, d_my, d_sx, d_sy
    dpx.close()
    dpy.close()
    ctx.close()
    if args.parent:  # fresh processes, one library each: this build's two halves like for like with the parent's
        for variant in ("", args.parent, "", args.parent):
            env = dict(os.environ, ATSC_LIB_VARIANT=variant)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--halves-only", "--reps", str(args.reps), "--buckets",
                                args.buckets],
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
