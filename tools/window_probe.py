"""Window decode probe (atsc_decompress_windows_dev / atsc_decompress_window) on one GPU.

Cases (HIP events around the device calls; the host call timed on the wall clock):
  single   one 4096-sample window on a prepared plan of the bench's batch (10,485,760 samples, 40960 frames x 256,
           auto e = 5 %), against the full decode of the same plan
  many     4096 windows of 256 samples at random offsets of the same batch in one call
  chunker  1000-sample windows over the reference chunker's framing (80 x 131072, auto e = 5 %), against the full
           decode (per frame)
  host     atsc_decompress_window on a ~1 GB .bro image (the batch's records repeated), with the bytes it uploads
           (the touched records' byte range, atsc_bro_find_window)
Prints one JSON object per case; --out FILE also writes them there.

    python tools/window_probe.py [--reps 50] [--out profiles/window_probe.json]
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--host-gb", type=float, default=1.0)
    args = ap.parse_args()
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

    me5 = float(np.float32(5) / np.float32(100))
    # ---- the bench batch
    n, fl = 10485760, 256
    x = H.synth_series(0, n)
    off = H.frame_offsets(n, fl)
    recs, _, _, _ = ctx.compress_host(x, off, A.AUTO, True, me5, 0)
    dp = A.DPlan(ctx, recs)
    d_body = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
    d_full = torch.empty(n, dtype=torch.float64, device=dev)
    full_ms, full_min = _time_ms(torch, lambda s: dp.decompress(d_body, d_full, s), args.reps)
    ref = d_full.cpu().numpy()
    d_win = torch.empty(4096, dtype=torch.float64, device=dev)
    b0 = 5000123
    one_ms, one_min = _time_ms(torch, lambda s: dp.decompress_windows(d_body, [b0], [4096], d_win, [0], s), args.reps)
    assert np.array_equal(d_win.cpu().numpy().view(np.uint64), ref[b0:b0 + 4096].view(np.uint64))
    emit({"case": "single", "samples": 4096, "frames_touched": 17, "window_ms_median": one_ms, "window_ms_min": one_min,
          "full_decode_ms_median": full_ms, "full_decode_ms_min": full_min, "stream_samples": n})
    rng = np.random.default_rng(1)
    nw, wl = 4096, 256
    begins = rng.integers(0, n - wl, nw).astype(np.uint64)
    counts = np.full(nw, wl, dtype=np.uint64)
    outo = (np.arange(nw) * wl).astype(np.uint64)
    d_many = torch.empty(nw * wl, dtype=torch.float64, device=dev)
    many_ms, many_min = _time_ms(torch, lambda s: dp.decompress_windows(d_body, begins, counts, d_many, outo, s), args.reps)
    got = d_many.cpu().numpy()
    for i in range(0, nw, 97):
        b = int(begins[i])
        assert np.array_equal(got[i * wl:(i + 1) * wl].view(np.uint64), ref[b:b + wl].view(np.uint64))
    emit({"case": "many", "windows": nw, "samples_per_window": wl, "ms_median": many_ms, "ms_min": many_min,
          "gsamples_per_s": nw * wl / (many_ms * 1e-3) / 1e9})
    dp.close()
    # ---- the chunker's framing
    nc, fc = 80 * 131072, 131072
    xc = H.synth_series(1, nc)
    offc = H.frame_offsets(nc, fc)
    recc, _, _, _ = ctx.compress_host(xc, offc, A.AUTO, True, me5, 0)
    dpc = A.DPlan(ctx, recc)
    d_bc = torch.frombuffer(bytearray(recc), dtype=torch.uint8).to(dev)
    d_fc = torch.empty(nc, dtype=torch.float64, device=dev)
    fullc_ms, _ = _time_ms(torch, lambda s: dpc.decompress(d_bc, d_fc, s), args.reps)
    refc = d_fc.cpu().numpy()
    d_w = torch.empty(1000, dtype=torch.float64, device=dev)
    rows = []
    for b in (17, 131072 - 500, 40 * 131072 + 99999, nc - 1000):
        ms, mn = _time_ms(torch, lambda s, b=b: dpc.decompress_windows(d_bc, [b], [1000], d_w, [0], s), args.reps)
        assert np.array_equal(d_w.cpu().numpy().view(np.uint64), refc[b:b + 1000].view(np.uint64))
        rows.append({"begin": b, "frames_touched": (b + 999) // fc - b // fc + 1, "ms_median": ms, "ms_min": mn})
    emit({"case": "chunker", "frames": 80, "frame_len": fc, "full_decode_ms_median": fullc_ms,
          "full_decode_ms_per_frame": fullc_ms / 80, "windows": rows})
    dpc.close()
    # ---- the host call on a ~1 GB image
    reps = max(1, int(args.host_gb * (1 << 30) / len(recs)))
    big = A.bro_prefix(40960 * reps) + recs * reps
    bw, cw = len(ref) * (reps // 2) + 777, 4096
    fw = A.bro_find_window(big, bw, cw)
    t0 = time.perf_counter()
    got = A.decompress_data_window(ctx, big, bw, cw)
    t1 = time.perf_counter()
    got2 = A.decompress_data_window(ctx, big, bw, cw)
    t2 = time.perf_counter()
    assert np.array_equal(got.view(np.uint64), ref[777:777 + cw].view(np.uint64)) and np.array_equal(got, got2)
    emit({"case": "host", "image_bytes": len(big), "window": [bw, cw], "uploaded_bytes": fw["byte_end"] - fw["byte_begin"],
          "touched_frames": fw["frame_end"] - fw["frame_begin"], "first_call_ms": (t1 - t0) * 1e3,
          "second_call_ms": (t2 - t1) * 1e3})
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
