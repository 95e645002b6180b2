"""Windowed aggregates probe (atsc_aggregate_windows_dev / atsc_aggregate_windows) on one GPU.

Cases (HIP events around the device calls, host task building included; the host call timed on the wall clock):
  bench     whole-stream buckets of 60 / 1024 / 65536 samples and one whole-stream window over the bench's batch
            (10,485,760 samples, 40960 frames x 256, auto e = 5 %), against (a) the full decode of the same plan and
            (b) the full decode into a tensor plus a torch reshape with amin / amax / sum
  chunker   the same over the reference chunker's framing (80 x 131072, auto e = 5 %)
  scale     one whole-stream window and 65536-sample buckets over 2^28 samples (the chunker batch's records repeated)
            under a 256 MiB budget, with the device memory the call holds (free memory before / after, torch's own
            allocations kept apart)
  sweep     the whole-stream 1024-sample buckets of both batches under pieces of 2^20 .. 2^25 samples
  host      aggregate_data_windows against decompress_data_window plus NumPy on a large window of a ~1 GB .bro image
Prints one JSON object per case; --out FILE also writes them there.

    python tools/aggregate_probe.py [--reps 30] [--out profiles/aggregate_probe.json]
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
    st = torch.cuda.current_stream()
    for _ in range(3):
        fn(st.cuda_stream)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn(st.cuda_stream)
        e1.record(st)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--host-gb", type=float, default=1.0)
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
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

    def batch(seed, n, fl):
        x = H.synth_series(seed, n)
        recs, _, _, _ = ctx.compress_host(x, H.frame_offsets(n, fl), A.AUTO, True, me5, 0)
        return recs

    def case(name, recs, n, buckets):
        dp = A.DPlan(ctx, recs)
        d_body = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        d_full = torch.empty(n, dtype=torch.float64, device=dev)
        full_ms, full_min = _time_ms(torch, lambda s: dp.decompress(d_body, d_full, s), args.reps)
        ref = d_full.cpu().numpy()
        rows = []
        for bk in buckets:
            bb, bc = A.bucket_windows(0, n, bk)
            d_st = torch.empty(len(bb) * 6, dtype=torch.int64, device=dev)
            ms, mn = _time_ms(torch, lambda s: dp.aggregate_windows(d_body, bb, bc, d_st, s), args.reps)
            st = d_st.cpu().numpy().view(A.WINDOW_STATS)
            k = len(bb) // 2
            v = ref[int(bb[k]):int(bb[k] + bc[k])]
            assert st["count"][k] == len(v) and st["min"][k] == v.min() and st["max"][k] == v.max()
            row = {"bucket": bk, "windows": len(bb), "ms_median": ms, "ms_min": mn, "x_full_decode": ms / full_ms}
            if n % bk == 0:  # (b) full decode into a tensor, then torch reductions over a reshape
                def torch_way(s, bk=bk):
                    dp.decompress(d_body, d_full, s)
                    y = d_full.view(-1, bk)
                    return y.amin(1), y.amax(1), y.sum(1)

                tms, _ = _time_ms(torch, torch_way, args.reps)
                row["torch_reshape_ms_median"] = tms
            rows.append(row)
        d_st = torch.empty(6, dtype=torch.int64, device=dev)
        wms, wmin = _time_ms(torch, lambda s: dp.aggregate_windows(d_body, [0], [n], d_st, s), args.reps)
        emit({"case": name, "samples": n, "full_decode_ms_median": full_ms, "full_decode_ms_min": full_min,
              "whole_window_ms_median": wms, "whole_window_ms_min": wmin, "buckets": rows})
        return dp, d_body

    nb, nc = 10485760, 80 * 131072
    recs = batch(0, nb, 256)
    recc = batch(1, nc, 131072)
    keep = {}
    if "bench" not in skip:
        keep["bench"] = case("bench", recs, nb, (60, 1024, 65536))
    if "chunker" not in skip:
        keep["chunker"] = case("chunker", recc, nc, (1024, 65536))
    if "sweep" not in skip:
        rows = []
        for name, r, n, large in (("bench", recs, nb, False), ("chunker", recc, nc, True)):
            dp = A.DPlan(ctx, r)
            d_body = torch.frombuffer(bytearray(r), dtype=torch.uint8).to(dev)
            bb, bc = A.bucket_windows(0, n, 1024)
            d_st = torch.empty(len(bb) * 6, dtype=torch.int64, device=dev)
            for lg in range(20, 26):
                ctx.set_aggregate_scratch(8 * ((1 << lg) + (2 * 131072 if large else 0)))
                ms, mn = _time_ms(torch, lambda s: dp.aggregate_windows(d_body, bb, bc, d_st, s), args.reps)
                rows.append({"framing": name, "piece_samples": 1 << lg, "pieces": -(-n // (1 << lg)), "ms_median": ms,
                             "ms_min": mn})
            ctx.set_aggregate_scratch(0)
            dp.close()
        emit({"case": "sweep", "buckets": 1024, "rows": rows})
    for dp, _ in keep.values():
        dp.close()
    keep.clear()
    if "scale" not in skip:
        reps = 26  # 26 x 80 x 131072 = 272,629,760 >= 2^28 samples
        big = recc * reps
        n = nc * reps
        dp = A.DPlan(ctx, big)
        d_body = torch.frombuffer(bytearray(big), dtype=torch.uint8).to(dev)
        ctx.set_aggregate_scratch(256 << 20)
        d_st = torch.empty(6, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        dp.aggregate_windows(d_body, [0], [n], d_st, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        free1 = torch.cuda.mem_get_info()[0]
        st = d_st.cpu().numpy().view(A.WINDOW_STATS)
        bb, bc = A.bucket_windows(0, n, 65536)
        d_sb = torch.empty(len(bb) * 6, dtype=torch.int64, device=dev)
        ms, _ = _time_ms(torch, lambda s: dp.aggregate_windows(d_body, bb, bc, d_sb, s), 5)
        free2 = torch.cuda.mem_get_info()[0]
        wms, _ = _time_ms(torch, lambda s: dp.aggregate_windows(d_body, [0], [n], d_st, s), 5)
        ctx.set_aggregate_scratch(0)
        emit({"case": "scale", "samples": n, "budget_bytes": 256 << 20, "first_call_ms": (t1 - t0) * 1e3,
              "whole_window_ms_median": wms, "buckets_65536_ms_median": ms, "count": int(st["count"][0]),
              "held_bytes_whole_window": free0 - free1, "held_bytes_after_buckets": free0 - free2,
              "bucket_tables_bytes": len(bb) * (48 + 32 * 2 + 32 + 48)})
        dp.close()
        del d_body
    if "host" not in skip:
        reps = max(1, int(args.host_gb * (1 << 30) / len(recs)))
        bigb = A.bro_prefix(40960 * reps) + recs * reps
        ref = ctx.decompress_host(recs)
        bw, cw = nb * (reps // 2) + 777, 8 * nb
        rows = []
        for cwi in (4096, nb, cw):
            t0 = time.perf_counter()
            st = A.aggregate_data_windows(ctx, bigb, [bw], [cwi])
            t1 = time.perf_counter()
            x = A.decompress_data_window(ctx, bigb, bw, cwi)
            mm = (x.min(), x.max(), x.sum())
            t2 = time.perf_counter()
            assert st["count"][0] == cwi and st["min"][0] == mm[0] and st["max"][0] == mm[1]
            assert st["first"][0] == ref[777]
            rows.append({"window": [bw, cwi], "aggregate_ms": (t1 - t0) * 1e3, "window_decode_plus_numpy_ms": (t2 - t1) * 1e3})
        emit({"case": "host", "image_bytes": len(bigb), "rows": rows})
    ctx.close()


if __name__ == "__main__":
    main()
