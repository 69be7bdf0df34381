#!/usr/bin/env python
"""Time TorchGate.gated_filterbank(x, fb, lengths=...) on a padded batch (sg_gate_features_rows, csrc/rows_feat.hip) against
(a) the composed route of the same tree (TorchGate._filterbank_composed: gated_stft(lengths=) -- which stores the whole
    (B, T, F) spectrogram -- then |.|^2, a GEMM, add and log in torch, torch autograd for the backward), the route ragged
    lengths took before the native one, and
(b) the per-row loop of gated_filterbank calls.

DESIGN section 14a's workload: 256 x 16000 float32 rows at sr 16000, lengths uniform in [2048, 16000] (seed 0), default
TorchGate (and the non-stationary gate), 80 mel bands, power 2, log.  Device events after warm-up; the one-call
candidates are ALTERNATED within each round, so drift of the clock or of a neighbour's load falls on all of them alike;
medians and (p90 - p10) / median are reported, forward and forward + backward of a scalar loss.  The per-row loop (256
launch-bound calls) is timed in rounds of its own, fewer of them.  torch.cuda.max_memory_allocated of one forward +
backward per candidate is recorded too (a number to report, no bar).  One process, one card.

    python tools/bench_gated_filterbank_rows.py --out profiles/gated_filterbank_rows_v1.json
    python tools/bench_gated_filterbank_rows.py --profile     # 20 forward + backward calls of each route, stationary: for
                                                              # rocprofv3 --kernel-trace --stats, a run of its own
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
    """name -> summary; every round runs every candidate once, in turn (tools/bench_gated_stft_rows.py's)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(once(fn))
    return {k: summary(v) for k, v in ms.items()}


def peak_bytes(fn):
    """Peak of torch's allocator over one call, above what was allocated before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--min-length", type=int, default=2048)
    ap.add_argument("--mels", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--loop-rounds", type=int, default=3, help="rounds of the per-row loop (one gated_filterbank call per row)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="a few calls of each route and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gated_filterbank_rows.py needs the GPU: nothing is measured without one")

    from noisereduce_amd.torchgate import TorchGate, mel_filterbank
    B, L, M = args.rows, args.samples, args.mels
    rng = np.random.default_rng(0)
    lens = [int(n) for n in rng.integers(args.min_length, L + 1, B)]
    x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(0))).cuda()
    for i, n in enumerate(lens):
        x[i, n:] = 0
    fb = mel_filterbank(16000, 1024, M)
    frames = sum(1 + n // 256 for n in lens)
    T, F = 1 + L // 256, 513
    kw = dict(power=2.0, log=True, eps=1e-6)
    result = {"device": torch.cuda.get_device_name(0), "rows": B, "samples": L, "dtype": "float32", "sr": 16000,
              "lengths": "uniform [%d, %d], seed 0" % (args.min_length, L), "frames": frames, "mels": M, "power": 2, "log": True,
              "spectrum_bytes": B * T * F * 8, "features_bytes": B * T * M * 4,
              "method": "device events, one-call candidates alternated within each round", "cases": {}}
    for nonstationary in (False, True):
        tg = TorchGate(sr=16000, nonstationary=nonstationary).cuda()
        bank = tg._bank(fb)
        rows_x = [x[i:i + 1, :n].contiguous() for i, n in enumerate(lens)]
        xg = x.clone().requires_grad_(True)

        def native():
            with torch.no_grad():
                tg.gated_filterbank(x, fb, lengths=lens, **kw)

        def composed():
            with torch.no_grad():
                tg._filterbank_composed(x, None, bank, 2, True, 1e-6, lens, None)

        def native_bwd():
            tg.gated_filterbank(xg, fb, lengths=lens, **kw).sum().backward()
            xg.grad = None

        def composed_bwd():
            tg._filterbank_composed(xg, None, bank, 2, True, 1e-6, lens, None)[0].sum().backward()
            xg.grad = None

        def row_loop():
            with torch.no_grad():
                for r in rows_x:
                    tg.gated_filterbank(r, fb, **kw)

        if args.profile:
            for fn in (native_bwd, composed_bwd):
                for _ in range(23):
                    fn()
            torch.cuda.synchronize()
            return
        case = alternated({"native": native, "composed": composed, "native_fwd_bwd": native_bwd,
                           "composed_fwd_bwd": composed_bwd}, args.warmup, args.rounds)
        case.update(alternated({"per_row_loop": row_loop}, 1, args.loop_rounds))
        for a, b, name in (("native", "composed", "forward"), ("native_fwd_bwd", "composed_fwd_bwd", "fwd_bwd")):
            n, c = case[a], case[b]
            case["speedup_over_composed_" + name] = c["median_ms"] / n["median_ms"]
            case["not_slower_than_composed_within_spread_" + name] = bool(
                n["median_ms"] <= c["median_ms"] * (1.0 + max(n["spread"], c["spread"])))
        case["speedup_over_loop"] = case["per_row_loop"]["median_ms"] / case["native"]["median_ms"]
        case["ns_per_frame"] = 1e6 * case["native"]["median_ms"] / frames
        case["peak_bytes_fwd_bwd"] = {"native": peak_bytes(native_bwd), "composed": peak_bytes(composed_bwd)}
        case["peak_bytes_forward"] = {"native": peak_bytes(native), "composed": peak_bytes(composed)}
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
