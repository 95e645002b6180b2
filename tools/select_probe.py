"""Windowed select probe (atsc_select_windows_dev) on one GPU.

On the 313215-sample stream of mixed small-tier records that tests/test_gpu_delta.py builds (`mixed`) and on the bench's
batch (10,485,760 samples, 40960 frames x 256, auto e = 5 %), each with the whole stream as one window and with windows
of 4096 samples, under GT at the stream's 99th percentile:
  select     atsc_select_windows_dev with cap = the number of selected samples, and the copy of its block (offsets and
             entries) to pinned host memory;
  sizing     the same call with cap = 0 (count and scan only);
  decode     atsc_decompress_windows_dev over the same windows, and the copy of the decoded samples to pinned host
             memory: what a caller does today before it filters on the host.
The calls are timed in turn in one process, each between HIP events of its own (tools/runs_probe.py's rounds), so the
host's task planning is inside: call time, not kernel time.  The select's block is checked against the NumPy model.
Prints one JSON object per window set; --out FILE also writes them there.

    python tools/select_probe.py [--reps 30] [--out profiles/select_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.runs_probe import _time_round_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available()
    import __graft_entry__ as G

    G.build()
    import atsc_amd as A
    from tests import helpers as H
    from tests import select_model as M
    from tests.test_gpu_delta import SMALL, _counter

    ctx = A.Context(0)
    dev = torch.device("cuda:0")
    # tests/test_gpu_delta.py's `mixed`
    lens = SMALL * 7
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    recs = b""
    rng = np.random.default_rng(3)
    for m, (comp, bounded, me) in enumerate([(A.FFT, True, 0.05), (A.CONSTANT, False, 0.0), (A.IDW, True, 0.05),
                                             (A.RLE, False, 0.0), (A.NOOP, False, 0.0)]):
        x = H.synth_series(2100 + m, int(off[-1]), block=3000)
        if comp == A.RLE:
            x = np.round(x / 8.0) * 8.0
        if comp == A.NOOP:
            x = _counter(rng, int(off[-1]))
        recs += ctx.compress_host(x, off, comp, bounded, float(np.float32(me)), 0)[0]
    res = []
    n_bench = 40960 * 256
    me5 = float(np.float32(5) / np.float32(100))
    bench = ctx.compress_host(H.synth_series(0, n_bench), H.frame_offsets(n_bench, 256), A.AUTO, True, me5, 0)[0]
    for stream, recs in (("mixed", recs), ("bench", bench)):
        full = ctx.decompress_host(recs)
        total = len(full)
        limit = float(np.quantile(full, 0.99))
        dp = A.DPlan(ctx, recs)
        d_body = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(dev)
        for name, bucket in (("one window", total), ("windows of 4096", 4096)):
            res.append(shape(torch, A, M, dp, d_body, full, limit, stream, name, bucket, args.reps))
            print(json.dumps(res[-1]), flush=True)
        dp.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


def shape(torch, A, M, dp, d_body, full, limit, stream, name, bucket, reps):
    """one window set of one stream -> its record"""
    dev, total = d_body.device, len(full)
    b, c = A.bucket_windows(0, total, bucket)
    wins = list(zip(b.tolist(), c.tolist()))
    want = M.windows_select(full, wins, M.GT, limit, 2 ** 62)
    n_sel = int(want[0][-1])
    words = A.select_bytes(len(wins), n_sel) // 8
    d_blk = torch.zeros(words, dtype=torch.int64, device=dev)
    h_blk = torch.zeros(words, dtype=torch.int64).pin_memory()
    d_dec = torch.zeros(total, dtype=torch.float64, device=dev)
    h_dec = torch.zeros(total, dtype=torch.float64).pin_memory()
    out_off = np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.uint64)

    def select(s):
        dp.select_windows(d_body, b, c, M.GT, limit, n_sel, d_blk, s)

    def select_copy(s):
        dp.select_windows(d_body, b, c, M.GT, limit, n_sel, d_blk, s)
        h_blk.copy_(d_blk, non_blocking=True)

    def sizing(s):
        dp.select_windows(d_body, b, c, M.GT, limit, 0, d_blk, s)

    def decode(s):
        dp.decompress_windows(d_body, b, c, d_dec, out_off, s)

    def decode_copy(s):
        dp.decompress_windows(d_body, b, c, d_dec, out_off, s)
        h_dec.copy_(d_dec, non_blocking=True)

    t = _time_round_ms(torch, [select, select_copy, sizing, decode, decode_copy], reps)
    select_copy(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = h_blk.numpy()
    n = len(wins)
    assert np.array_equal(h[: n + 1].view(np.uint64), want[0])
    e = h[n + 1: n + 1 + 2 * n_sel].view(A.SELECTED)
    assert np.array_equal(e["value"].view(np.uint64), want[1]["value"].view(np.uint64)) and np.array_equal(e["at"], want[1]["at"])
    assert np.array_equal(h_dec.numpy().view(np.uint64), full.view(np.uint64))
    d = {"stream": stream, "windows": name, "n_windows": n, "samples": total, "selected": n_sel, "block_bytes": 8 * words,
         "decoded_bytes": 8 * total, "reps": reps}
    for key, v in zip(("select", "select_and_copy", "sizing", "decode", "decode_and_copy"), t):
        d[key + "_us"] = [round(1000 * q, 1) for q in v]  # median, min, max
    return d


if __name__ == "__main__":
    main()
