"""Windowed rolling pair moments probe (atsc_rolling_pair_windows_dev) on one GPU.

The bench's batch (10,485,760 samples, 40960 frames x 256, auto e = 5 %) read as one stream X, and a second series in
the same framing as Y.  Per shape (width, stride) one range of the streams is queried four ways, timed alternately in one
process after warm-up rounds, each between HIP events of its own around the device call (host task planning is inside:
call time, not kernel time), and reported as median, min and max over --reps rounds, with the median time the host spent
inside the call beside them:
  pair      one atsc_rolling_pair_windows_dev call: the range named once, with the width and the stride
  explicit  one atsc_pair_windows_dev call over the explicitly listed windows of the same positions (code that this
            query does not touch: it stands for what a caller has to do without it)
  moments   one atsc_rolling_moments_windows_dev call of the same range, width and stride on X alone: the same partial
            and merge over one region, for scale
  decode    one atsc_decompress_windows_dev call of the range of X (the samples handed out, no reduction)
The range is the whole stream where the stride keeps the explicit list below --max-positions windows, else the streams'
first --max-positions * stride + width - 1 samples, as tools/rolling_probe.py has it.  The count of every record is
checked against the explicit call's, the doubles against its within the sum of the two stated bounds (the scales read off
the explicit call's values in f64, which is good to the bounds' own relative size: 1 % is added), and a few records
against the NumPy model, bit for bit.  Prints one JSON object per shape; --out FILE also writes them.

    python tools/rolling_pair_probe.py [--reps 9] [--shapes 20:1,300:15,3600:1] [--max-positions 1048576] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.rolling_probe import FRAME, N, _time_ms  # noqa: E402


def _mean_abs(v, lo, w):
    cs = np.concatenate([[0.0], np.cumsum(np.abs(v))])
    return (cs[lo + w] - cs[lo]) / float(w)


def _close(got, ref, x, y, lo, w, M, PM):
    """every double of got within the two calls' bounds of ref's (no NaN and no Inf in these streams: count == w)"""
    n = float(w)
    k = (3 * M.depth(w) + 2 + M.depth(w) + 2) * PM.U * 1.01
    ax = ref["m2_x"] + n * ref["mean_x"] ** 2  # kappa_x^2 m2_x
    ay = ref["m2_y"] + n * ref["mean_y"] ** 2
    lims = {"mean_x": k * _mean_abs(x, lo, w), "m2_x": k * np.sqrt(ref["m2_x"] * ax), "mean_y": k * _mean_abs(y, lo, w),
            "m2_y": k * np.sqrt(ref["m2_y"] * ay), "c_xy": k * np.sqrt(ax * ay)}
    for name, lim in lims.items():
        bad = np.flatnonzero(~(np.abs(got[name] - ref[name]) <= lim))
        assert len(bad) == 0, (w, name, len(bad), got[bad[0]], ref[bad[0]], lim[bad[0]])


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
    from tests import pair_model as PM
    from tests import rolling_pair_model as M

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    me5 = float(np.float32(5) / np.float32(100))
    plans, bodies, fulls = [], [], []
    d_full = torch.empty(N, dtype=torch.float64, device=dev)
    for seed in (0, 1):
        recs = ctx.compress_host(H.synth_series(seed, N), H.frame_offsets(N, FRAME), A.AUTO, True, me5, 0)[0]
        plans.append(A.DPlan(ctx, recs))
        bodies.append(torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev))
        plans[-1].decompress(bodies[-1], d_full, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        fulls.append(d_full.cpu().numpy().copy())
        assert np.isfinite(fulls[-1]).all()
    (dpx, dpy), (bx, by), (x, y) = plans, bodies, fulls
    res = []
    for shape in args.shapes.split(","):
        w, s = (int(v) for v in shape.split(":"))
        count = min(N, args.max_positions * s + w - 1)
        m = A.rolling_outputs(count, w, s)
        lo = (s * np.arange(m)).astype(np.uint64)
        cn = np.full(m, w, dtype=np.uint64)
        d_new, d_list, d_mom = (torch.empty(6 * m, dtype=torch.int64, device=dev) for _ in range(3))
        fns = [lambda st: dpx.rolling_pair_windows(bx, dpy, by, [0], [count], w, s, d_new, st),
               lambda st: dpx.pair_windows(bx, dpy, by, lo, cn, d_list, st),
               lambda st: dpx.rolling_moments_windows(bx, [0], [count], w, s, d_mom, st),
               lambda st: dpx.decompress_windows(bx, [0], [count], d_full, [0], st)]
        row = {"width": w, "stride": s, "range": count, "positions": m, "reps": args.reps}
        for name, (med, tlo, thi, host) in zip(("pair", "explicit", "moments", "decode"), _time_ms(torch, fns, args.reps)):
            row.update({name + "_ms_median": med, name + "_ms_min": tlo, name + "_ms_max": thi, name + "_host_ms_median": host})
        got = d_new.cpu().numpy().view(A.WINDOW_PAIR)
        ref = d_list.cpu().numpy().view(A.WINDOW_PAIR)
        assert got["count"].tobytes() == ref["count"].tobytes() and np.all(got["count"] == w), shape
        _close(got, ref, x, y, lo.astype(np.int64), w, M, PM)
        at = sorted({0, 1, m // 3, m // 2, m - 1})
        want = M.Pyramid(x[:count], y[:count]).records(lo[at].astype(np.int64), w)
        assert got[at].tobytes() == want.tobytes(), (shape, got[at], want)
        if count < N:  # the new call and the decode alone over the whole streams, which the explicit list does not reach
            mw = A.rolling_outputs(N, w, s)
            d_whole = torch.empty(6 * mw, dtype=torch.int64, device=dev)
            fns = [lambda st: dpx.rolling_pair_windows(bx, dpy, by, [0], [N], w, s, d_whole, st),
                   lambda st: dpx.decompress_windows(bx, [0], [N], d_full, [0], st)]
            (r_med, r_lo, r_hi, r_host), (d_med, _, _, _) = _time_ms(torch, fns, args.reps)
            assert d_whole.cpu().numpy().view(A.WINDOW_PAIR)[:m].tobytes() == got.tobytes(), shape
            row.update({"whole_positions": mw, "whole_pair_ms_median": r_med, "whole_pair_ms_min": r_lo,
                        "whole_pair_ms_max": r_hi, "whole_pair_host_ms_median": r_host, "whole_decode_ms_median": d_med})
            del d_whole
        row["pair_over_explicit"] = row["pair_ms_median"] / row["explicit_ms_median"]
        row["pair_over_moments"] = row["pair_ms_median"] / row["moments_ms_median"]
        row["pair_over_decode"] = row["pair_ms_median"] / row["decode_ms_median"]
        print(json.dumps(row), flush=True)
        res.append(row)
        del d_new, d_list, d_mom
    for dp in plans:
        dp.close()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
