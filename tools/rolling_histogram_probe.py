"""Windowed rolling histograms probe (atsc_rolling_histogram_windows_dev) on one GPU.

The bench's batch (10,485,760 samples, 40960 frames x 256, auto e = 5 %) read as one stream.  Per shape (width, stride)
one range of the stream is queried four ways over 12 `le`-style edges (eleven of the stream's own quantiles and +Inf,
right closed), timed alternately in one process after warm-up rounds, each between HIP events of its own around the
device call (host task planning is inside: call time, not kernel time), and reported as median, min and max over --reps
rounds, with the median time the host spent inside the call beside them:
  histogram one atsc_rolling_histogram_windows_dev call: the range named once, with the width and the stride
  explicit  one atsc_histogram_windows_dev call over the explicitly listed windows of the same positions (code that this
            query does not touch: it stands for what a caller has to do without it)
  rolling   one atsc_rolling_windows_dev call of the same range, width and stride: what a sum costs at every position
  decode    one atsc_decompress_windows_dev call of the range (the samples handed out, no reduction): the floor
The range is the whole stream where the stride keeps the explicit list below --max-positions windows, else the stream's
first --max-positions * stride + width - 1 samples, as tools/rolling_probe.py has it; there the new call and the decode
are also timed over the whole stream.  Every row is checked against the explicit call's, byte for byte, and a few rows
against the NumPy model.  Behind the shapes, not compared with anything: one shape with 1024 edges at 2^16 positions.
Prints one JSON object per shape; --out FILE also writes them.

    python tools/rolling_histogram_probe.py [--reps 9] [--shapes 20:1,300:15,3600:1] [--max-positions 1048576] [--out FILE]
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
    ap.add_argument("--wide", default="300:1", help="WIDTH:STRIDE of the shape with 1024 edges at 2^16 positions ('' for none)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import helpers as H
    from tests import rolling_histogram_model as M

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    me5 = float(np.float32(5) / np.float32(100))
    recs = ctx.compress_host(H.synth_series(0, N), H.frame_offsets(N, FRAME), A.AUTO, True, me5, 0)[0]
    dp = A.DPlan(ctx, recs)
    body = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
    d_full = torch.empty(N, dtype=torch.float64, device=dev)
    dp.decompress(body, d_full, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    full = d_full.cpu().numpy()
    distinct = np.unique(full[:: 64])  # (eleven DISTINCT values: the stream holds runs of equal samples)
    edges = np.concatenate([distinct[np.round(np.linspace(0.05, 0.95, 11) * (len(distinct) - 1)).astype(np.int64)], [np.inf]])
    assert len(edges) == 12 and np.all(np.diff(edges) > 0)
    closed = A.HIST_RIGHT_CLOSED
    rows = len(edges) + 2
    res = []
    for shape in args.shapes.split(","):
        w, s = (int(v) for v in shape.split(":"))
        count = min(N, args.max_positions * s + w - 1)
        m = A.rolling_outputs(count, w, s)
        lo = (s * np.arange(m)).astype(np.uint64)
        cn = np.full(m, w, dtype=np.uint64)
        d_new = torch.empty(rows * m, dtype=torch.int64, device=dev)
        d_list = torch.empty(rows * m, dtype=torch.int64, device=dev)
        d_roll = torch.empty(4 * m, dtype=torch.int64, device=dev)
        fns = [lambda st: dp.rolling_histogram_windows(body, [0], [count], w, s, edges, d_new, closed, st),
               lambda st: dp.histogram_windows(body, lo, cn, edges, d_list, closed, st),
               lambda st: dp.rolling_windows(body, [0], [count], w, s, d_roll, st),
               lambda st: dp.decompress_windows(body, [0], [count], d_full, [0], st)]
        row = {"width": w, "stride": s, "n_edges": len(edges), "range": count, "positions": m, "reps": args.reps,
               "task_positions": M.task_positions(w, s)}
        for name, (med, tlo, thi, host) in zip(("histogram", "explicit", "rolling", "decode"), _time_ms(torch, fns, args.reps)):
            row.update({name + "_ms_median": med, name + "_ms_min": tlo, name + "_ms_max": thi, name + "_host_ms_median": host})
        got = d_new.cpu().numpy().view(np.uint64).reshape(m, rows)
        ref = d_list.cpu().numpy().view(np.uint64).reshape(m, rows)
        assert got.tobytes() == ref.tobytes(), shape
        at = sorted({0, 1, m // 3, m // 2, m - 1})
        want = M.rows(full[:count], lo[at].astype(np.int64), w, edges, closed)
        assert np.array_equal(got[at], want), (shape, got[at], want)
        if count < N:  # the new call and the decode alone over the whole stream, which the explicit list does not reach
            mw = A.rolling_outputs(N, w, s)
            d_whole = torch.empty(rows * mw, dtype=torch.int64, device=dev)
            fns = [lambda st: dp.rolling_histogram_windows(body, [0], [N], w, s, edges, d_whole, closed, st),
                   lambda st: dp.decompress_windows(body, [0], [N], d_full, [0], st)]
            (r_med, r_lo, r_hi, r_host), (d_med, _, _, _) = _time_ms(torch, fns, args.reps)
            assert d_whole[: rows * m].cpu().numpy().tobytes() == got.tobytes(), shape
            row.update({"whole_positions": mw, "whole_histogram_ms_median": r_med, "whole_histogram_ms_min": r_lo,
                        "whole_histogram_ms_max": r_hi, "whole_histogram_host_ms_median": r_host, "whole_decode_ms_median": d_med})
            del d_whole
        row["histogram_over_explicit"] = row["histogram_ms_median"] / row["explicit_ms_median"]
        row["histogram_over_rolling"] = row["histogram_ms_median"] / row["rolling_ms_median"]
        row["histogram_over_decode"] = row["histogram_ms_median"] / row["decode_ms_median"]
        print(json.dumps(row), flush=True)
        res.append(row)
        del d_new, d_list, d_roll
    if args.wide:  # 1024 edges at 2^16 positions: a row of 8 KB per position, the store of the rows against the slide
        w, s = (int(v) for v in args.wide.split(":"))
        m = 1 << 16
        count = (m - 1) * s + w
        wide = np.linspace(float(np.quantile(full[:: 64], 0.01)), float(np.quantile(full[:: 64], 0.99)), 1024)
        d_new = torch.empty(1026 * m, dtype=torch.int64, device=dev)
        fns = [lambda st: dp.rolling_histogram_windows(body, [0], [count], w, s, wide, d_new, closed, st),
               lambda st: dp.decompress_windows(body, [0], [count], d_full, [0], st)]
        (h_med, h_lo, h_hi, h_host), (d_med, _, _, _) = _time_ms(torch, fns, args.reps)
        got = d_new.cpu().numpy().view(np.uint64).reshape(m, 1026)
        at = sorted({0, 1, m // 3, m // 2, m - 1})
        assert np.array_equal(got[at], M.rows(full[:count], s * np.array(at, dtype=np.int64), w, wide, closed)), "wide"
        row = {"width": w, "stride": s, "n_edges": 1024, "range": count, "positions": m, "reps": args.reps,
               "task_positions": M.task_positions(w, s), "histogram_ms_median": h_med, "histogram_ms_min": h_lo,
               "histogram_ms_max": h_hi, "histogram_host_ms_median": h_host, "decode_ms_median": d_med}
        print(json.dumps(row), flush=True)
        res.append(row)
        del d_new
    dp.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
