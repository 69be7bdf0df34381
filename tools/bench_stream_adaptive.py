#!/usr/bin/env python
"""Steady-state cost of a StreamBank step with the noise profile learnt from the stream (noise_from_stream=True) against
the fixed-profile bank, both in the same process.

For S mono streams fed 20 ms blocks as device tensors: median of event-timed ``push`` steps after warm-up, and the decide /
fsmooth / apply / finish split of one step from the engine's own event timing, for the two banks in turn.  Writes
profiles/stream_adaptive_v1.json (``--out``) and prints it.

    python tools/bench_stream_adaptive.py [--streams 1,16,256,1024] [--steps 30] [--warmup 10] [--noise-memory-s 2.0]
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

import noisereduce_amd as nr  # noqa: E402
from oracle import spectralgate_oracle as O  # noqa: E402
from tools.bench_stream import CONFIGS  # noqa: E402


def step_ms(bank, blocks, steps, warmup):
    for _ in range(warmup):
        bank.push(blocks)
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        bank.push(blocks)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    g = bank.gate
    g.profile_enable(True)
    g.profile_read(reset=True)
    bank.push(blocks)
    stages = {k: v[0] for k, v in g.profile_read(reset=True).items()}
    g.profile_enable(False)
    return {"step_ms": statistics.median(times), "stage_ms": stages}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,256,1024")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--noise-memory-s", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_adaptive_v1.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
              "noise_memory_s": a.noise_memory_s, "configs": {}}
    for name, cfg in CONFIGS.items():
        sr = cfg["sr"]
        kw = {k: v for k, v in cfg.items() if k != "sr"}
        block = sr // 50
        noise = 0.1 * np.random.default_rng(7).standard_normal(3 * sr // 4)
        rows = {}
        for S in [int(s) for s in a.streams.split(",")]:
            x = torch.from_numpy(np.stack([O.synth_signal(block, sr=sr, seed=s, dtype=np.float32)
                                           for s in range(min(S, 32))])).cuda()
            blocks = {s: x[s % x.shape[0]] for s in range(S)}
            fixed = nr.StreamBank(sr, S, y_noise=noise, max_block=block, **kw)
            adaptive = nr.StreamBank(sr, S, noise_from_stream=True, noise_memory_s=a.noise_memory_s, max_block=block, **kw)
            row = {"fixed": step_ms(fixed, blocks, a.steps, a.warmup), "adaptive": step_ms(adaptive, blocks, a.steps, a.warmup)}
            row["adaptive_over_fixed"] = row["adaptive"]["step_ms"] / row["fixed"]["step_ms"]
            fixed.close()
            adaptive.close()
            rows[str(S)] = row
            print(f"[bench_stream_adaptive] {name} S={S}: fixed {row['fixed']['step_ms']:.3f} ms, adaptive "
                  f"{row['adaptive']['step_ms']:.3f} ms ({row['adaptive_over_fixed']:.3f} x)", flush=True)
        result["configs"][name] = rows
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"stream_adaptive_bench": result["configs"]}))


if __name__ == "__main__":
    main()
