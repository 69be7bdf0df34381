#!/usr/bin/env python
"""Time TorchGate.gated_stft(x, lengths=...) on a padded batch (sg_gate_spectrum_rows, csrc/rows.hip) against
(a) the per-row loop of gated_stft calls -- the only correct alternative without the keyword -- and
(b) forward(x, lengths=...) from the same tree: the same statistics, decisions and smoothing, plus the inverse transform
    and the overlap-add, minus the complex store of the whole (B, T, F) field.

DESIGN section 12's workload: 256 x 16000 float32 rows at sr 16000, lengths uniform in [2048, 16000], default TorchGate,
stationary and non-stationary.  Device events after warm-up; the candidates of a gate are ALTERNATED within each round,
so drift of the clock or of a neighbour's load falls on all of them alike; medians and (p90 - p10) / median are reported.
The per-row loop (256 launch-bound calls) is timed in rounds of its own, fewer of them.

    python tools/bench_gated_stft_rows.py --out profiles/gated_stft_rows_v1.json
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


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    ms = sorted(ms)
    med = statistics.median(ms)
    p10, p90 = ms[int(0.1 * (len(ms) - 1))], ms[int(0.9 * (len(ms) - 1))]
    return {"median_ms": med, "min_ms": ms[0], "p10_ms": p10, "p90_ms": p90, "spread": (p90 - p10) / med, "repeats": len(ms)}


def alternated(fns, warmup, rounds):
    """name -> summary; every round runs every candidate once, in turn."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(once(fn))
    return {k: summary(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--min-length", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--loop-rounds", type=int, default=5, help="rounds of the per-row loop (one gated_stft call per row)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gated_stft_rows.py needs the GPU: nothing is measured without one")

    from noisereduce_amd.torchgate import TorchGate
    B, L = args.rows, args.samples
    rng = np.random.default_rng(0)
    lens = [int(n) for n in rng.integers(args.min_length, L + 1, B)]
    x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(0))).cuda()
    for i, n in enumerate(lens):
        x[i, n:] = 0
    frames = sum(1 + n // 256 for n in lens)
    T, F = 1 + L // 256, 513
    result = {"device": torch.cuda.get_device_name(0), "rows": B, "samples": L, "dtype": "float32", "sr": 16000,
              "lengths": "uniform [%d, %d], seed 0" % (args.min_length, L), "frames": frames,
              "spectrum_bytes": B * T * F * 8, "method": "device events, candidates alternated within each round",
              "cases": {}}
    for nonstationary in (False, True):
        tg = TorchGate(sr=16000, nonstationary=nonstationary).cuda()
        rows_x = [x[i:i + 1, :n].contiguous() for i, n in enumerate(lens)]
        xg = x.clone().requires_grad_(True)
        gY = torch.ones((B, T, F, 2), device="cuda")

        def spectrum():
            with torch.no_grad():
                tg.gated_stft(x, lengths=lens)

        def spectrum_bwd():
            Y = tg.gated_stft(xg, lengths=lens)
            torch.view_as_real(Y.transpose(1, 2)).backward(gY)
            xg.grad = None

        def waveform():
            with torch.no_grad():
                tg(x, lengths=lens)

        def row_loop():
            with torch.no_grad():
                for r in rows_x:
                    tg.gated_stft(r)

        case = alternated({"gated_stft_lengths": spectrum, "gated_stft_lengths_fwd_bwd": spectrum_bwd,
                           "forward_lengths": waveform}, args.warmup, args.rounds)
        case.update(alternated({"per_row_gated_stft_loop": row_loop}, 1, args.loop_rounds))
        s, w = case["gated_stft_lengths"], case["forward_lengths"]
        case["speedup_over_loop"] = case["per_row_gated_stft_loop"]["median_ms"] / s["median_ms"]
        case["ratio_to_forward_lengths"] = s["median_ms"] / w["median_ms"]
        case["not_slower_than_forward_within_spread"] = bool(s["median_ms"] <= w["median_ms"] * (1.0 + max(s["spread"], w["spread"])))
        case["ns_per_frame"] = 1e6 * s["median_ms"] / frames
        key = "nonstationary" if nonstationary else "stationary"
        result["cases"][key] = case
        print(key, json.dumps(case), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
