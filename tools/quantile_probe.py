"""Windowed quantiles probe (atsc_quantile_windows_dev) on one GPU.

Cases (HIP events around the device calls, host task building included), each against three baselines: the aggregate
call on the same windows, the full decode of the same plan, and the full decode into a tensor plus torch.sort of the
(n_buckets, B) view and a gather (torch.quantile for the whole window, which takes up to 2^24 elements):
  bench      the bench's batch (10,485,760 samples, 40960 frames x 256, auto e = 5 %): one whole-stream window and
             buckets of 60 / 1024 / 16384 / 65536 samples, levels (0.5, 0.9, 0.99) linear
  chunker    the same over the reference chunker's framing (80 x 131072, auto e = 5 %)
  nq         the bench batch's 1024-sample buckets and whole window at n_q = 1 / 3 / 16 / 64
  dup        a duplicate-heavy stream (RLE of 8 values, bench framing): deep radix passes on long windows
Prints one JSON object per case; --out FILE also writes them there.

    python tools/quantile_probe.py [--reps 20] [--out profiles/quantile_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_ms(torch, fn, reps):
    st = torch.cuda.current_stream()
    for _ in range(2):
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out")
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import helpers as H
    from tests import quantile_model as M

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
    levels = [0.5, 0.9, 0.99]

    def batch(seed, n, fl, comp=A.AUTO, quantise=False):
        x = H.synth_series(seed, n)
        if quantise:
            x = np.round(x / np.ptp(x) * 7.0)
        recs, _, _, _ = ctx.compress_host(x, H.frame_offsets(n, fl), comp, comp == A.AUTO, me5 if comp == A.AUTO else 0.0,
                                          0)
        return recs

    def windows_row(dp, d_body, d_full, ref, n, bk, lv, full_ms):
        bb, bc = A.bucket_windows(0, n, bk) if bk else (np.array([0], dtype=np.uint64), np.array([n], dtype=np.uint64))
        d_q = torch.empty(len(bb) * len(lv), dtype=torch.float64, device=dev)
        ms, mn = _time_ms(torch, lambda s: dp.quantile_windows(d_body, bb, bc, lv, d_q, A.QUANTILE_LINEAR, s), args.reps)
        got = d_q.cpu().numpy().reshape(len(bb), len(lv))
        for k in sorted({0, len(bb) // 2, len(bb) - 1}):  # spot check against the model
            want = M.quantiles(ref[int(bb[k]):int(bb[k] + bc[k])], lv)
            assert np.array_equal(got[k].view(np.uint64), want.view(np.uint64)), (bk, k, got[k], want)
        d_st = torch.empty(len(bb) * 6, dtype=torch.int64, device=dev)
        ams, _ = _time_ms(torch, lambda s: dp.aggregate_windows(d_body, bb, bc, d_st, s), args.reps)
        row = {"bucket": bk or n, "windows": len(bb), "levels": len(lv), "ms_median": ms, "ms_min": mn,
               "aggregate_ms_median": ams, "x_aggregate": ms / ams, "x_full_decode": ms / full_ms}
        qt = torch.tensor(lv, dtype=torch.float64, device=dev)
        if bk and n % bk == 0:
            def torch_way(s, bk=bk):
                dp.decompress(d_body, d_full, s)
                y = torch.sort(d_full.view(-1, bk), dim=1)[0]
                pos = qt * (bk - 1)
                lo = pos.floor().long()
                hi = torch.clamp(lo + 1, max=bk - 1)
                t = pos - lo
                a, b = y[:, lo], y[:, hi]
                return a + (b - a) * t

            row["torch_sort_ms_median"], _ = _time_ms(torch, torch_way, args.reps)
        elif not bk and n <= (1 << 24):
            def torch_q(s):
                dp.decompress(d_body, d_full, s)
                return torch.quantile(d_full, qt)

            row["torch_quantile_ms_median"], _ = _time_ms(torch, torch_q, args.reps)
        return row

    def case(name, recs, n, buckets, lv=levels):
        dp = A.DPlan(ctx, recs)
        d_body = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        d_full = torch.empty(n, dtype=torch.float64, device=dev)
        full_ms, full_min = _time_ms(torch, lambda s: dp.decompress(d_body, d_full, s), args.reps)
        ref = d_full.cpu().numpy()
        rows = [windows_row(dp, d_body, d_full, ref, n, bk, lv, full_ms) for bk in buckets]
        emit({"case": name, "samples": n, "full_decode_ms_median": full_ms, "full_decode_ms_min": full_min,
              "rows": rows})
        dp.close()

    nb, nc = 10485760, 80 * 131072
    if "bench" not in skip:
        case("bench", batch(0, nb, 256), nb, (0, 60, 1024, 16384, 65536))
    if "chunker" not in skip:
        case("chunker", batch(1, nc, 131072), nc, (0, 1024, 65536))
    if "nq" not in skip:
        recs = batch(0, nb, 256)
        rng = np.random.default_rng(7)
        for nq in (1, 3, 16, 64):
            lv = [0.5] if nq == 1 else levels if nq == 3 else sorted(rng.random(nq).tolist())
            case("nq_%d" % nq, recs, nb, (0, 1024), lv)
    if "dup" not in skip:
        case("dup", batch(2, nb, 256, A.RLE, True), nb, (0, 1024, 65536))
    ctx.close()


if __name__ == "__main__":
    main()
