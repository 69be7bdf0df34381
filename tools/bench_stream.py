#!/usr/bin/env python
"""Steady-state cost of a StreamBank step against what a caller could do before it existed.

For S mono streams fed 20 ms blocks as device tensors: median of event-timed ``push`` steps after warm-up, against a loop
of one ``reduce_noise(context + block, y_noise=, stationary=True, chunk_size=None, padding=0)`` per stream and block on a
device tensor of ``latency_samples + block`` samples.  Writes profiles/stream_v1.json (``--out``) and prints it.

    python tools/bench_stream.py [--streams 1,16,256,1024] [--steps 30] [--loop-repeats 5] [--out profiles/stream_v1.json]

``--stage-split`` adds the per-stage times of one step from the engine's own event timing (the names are those of the
batched path's stages, which the stream kernels are booked under)."""
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

CONFIGS = {"16k_512_400_160": dict(sr=16000, n_fft=512, win_length=400, hop_length=160),
           "48k_defaults": dict(sr=48000, n_fft=1024, win_length=None, hop_length=None)}


def step_ms(cfg, S, steps, warmup, split):
    sr = cfg["sr"]
    kw = {k: v for k, v in cfg.items() if k != "sr"}
    block = sr // 50
    noise = 0.1 * np.random.default_rng(7).standard_normal(3 * sr // 4)
    bank = nr.StreamBank(sr, S, y_noise=noise, max_block=block, **kw)
    x = torch.from_numpy(np.stack([O.synth_signal(block, sr=sr, seed=s, dtype=np.float32) for s in range(min(S, 32))])).cuda()
    blocks = {s: x[s % x.shape[0]] for s in range(S)}
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
    res = {"step_ms": statistics.median(times), "block_ms": 1000.0 * block / sr, "latency_samples": bank.latency_samples}
    if split:
        g = bank.gate
        g.profile_enable(True)
        g.profile_read(reset=True)
        bank.push(blocks)
        res["stage_ms"] = {k: v[0] for k, v in g.profile_read(reset=True).items()}
        g.profile_enable(False)
    # the loop a caller had to write before: re-gate a sliding window of context per stream and block
    ctx = torch.from_numpy(O.synth_signal(bank.latency_samples + block, sr=sr, seed=1, dtype=np.float32)).cuda()
    bank.close()
    return res, ctx, noise, kw


def loop_ms(cfg, S, ctx, noise, kw, repeats):
    sr = cfg["sr"]
    call = lambda: nr.reduce_noise(ctx, sr, y_noise=noise, stationary=True, chunk_size=None, padding=0, device="cuda", **kw)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(S):
            call()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,256,1024")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--loop-repeats", type=int, default=5)
    ap.add_argument("--stage-split", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_v1.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "loop_repeats": a.loop_repeats, "configs": {}}
    for name, cfg in CONFIGS.items():
        rows = {}
        for S in [int(s) for s in a.streams.split(",")]:
            res, ctx, noise, kw = step_ms(cfg, S, a.steps, a.warmup, a.stage_split)
            res["loop_ms"] = loop_ms(cfg, S, ctx, noise, kw, a.loop_repeats)
            res["loop_over_step"] = res["loop_ms"] / res["step_ms"]
            rows[str(S)] = res
            print(f"[bench_stream] {name} S={S}: step {res['step_ms']:.3f} ms, loop {res['loop_ms']:.3f} ms "
                  f"({res['loop_over_step']:.1f} x), block {res['block_ms']:.0f} ms", flush=True)
        result["configs"][name] = rows
    if os.path.exists(a.out):   # keep what other tools put there (the local-parity ratio of the GPU tests)
        try:
            old = json.load(open(a.out))
            for k in old:
                result.setdefault(k, old[k])
        except ValueError:
            pass
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"stream_bench": result["configs"]}))


if __name__ == "__main__":
    main()
