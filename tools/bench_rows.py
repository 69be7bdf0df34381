#!/usr/bin/env python
"""Time TorchGate.forward(x, lengths=...) on a padded batch against the two things a caller can do without it:
(a) a Python loop of per-row TorchGate calls on the full-length path -- the only correct alternative -- and
(b) one full-length call on the padded tensor (wrong results for the padded rows: the floor).

256 x 16000 float32 rows at sr 16000, lengths uniform in [2048, 16000]; forward and forward + backward; stationary and
non-stationary.  Warm-up, then every repeat timed with a pair of events on the stream; the median and the spread of
the repeats are reported.

    python tools/bench_rows.py --out profiles/rows_v1.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "p90_ms": ms[int(0.9 * (len(ms) - 1))], "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--min-length", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--loop-repeats", type=int, default=5, help="repeats of the per-row loop (256 calls each)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from noisereduce_amd.torchgate import TorchGate
    B, L = args.rows, args.samples
    rng = np.random.default_rng(0)
    lens = [int(n) for n in rng.integers(args.min_length, L + 1, B)]
    x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(0))).cuda()
    for i, n in enumerate(lens):
        x[i, n:] = 0
    frames = sum(1 + n // 256 for n in lens)
    result = {"device": torch.cuda.get_device_name(0), "rows": B, "samples": L, "dtype": "float32", "sr": 16000,
              "lengths": "uniform [%d, %d], seed 0" % (args.min_length, L), "frames": frames, "cases": {}}
    for nonstationary in (False, True):
        tg = TorchGate(sr=16000, nonstationary=nonstationary).cuda()
        rows_x = [x[i:i + 1, :n].contiguous() for i, n in enumerate(lens)]
        for backward in (False, True):
            xg = x.clone().requires_grad_(backward)
            rows_g = [r.clone().requires_grad_(backward) for r in rows_x]

            def new_path():
                y = tg(xg, lengths=lens)
                if backward:
                    y.backward(torch.ones_like(y))

            def full_call():
                y = tg(xg)
                if backward:
                    y.backward(torch.ones_like(y))

            def row_loop():
                for r in rows_g:
                    y = tg(r)
                    if backward:
                        y.backward(torch.ones_like(y))

            key = ("nonstationary" if nonstationary else "stationary") + ("_fwd_bwd" if backward else "_fwd")
            case = {"lengths": timed(new_path, args.warmup, args.repeats),
                    "full_length_call_wrong_results": timed(full_call, args.warmup, args.repeats),
                    "per_row_loop": timed(row_loop, 1, args.loop_repeats)}
            case["speedup_over_loop"] = case["per_row_loop"]["median_ms"] / case["lengths"]["median_ms"]
            case["ns_per_frame"] = 1e6 * case["lengths"]["median_ms"] / frames
            result["cases"][key] = case
            print(key, json.dumps(case), flush=True)
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
