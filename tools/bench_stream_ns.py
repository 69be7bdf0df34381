#!/usr/bin/env python
"""Steady-state cost of a non-stationary StreamBank step (tools/bench_stream.py's sibling).

For S mono streams fed 20 ms blocks as device tensors, at ``lookahead_ms`` 0 and 100: median of event-timed ``push`` steps
after warm-up with the per-stage times of one step from the engine's event timing; next to each row, from the same
session, the stationary bank's step re-measured and the loop of one ``reduce_noise(context + block, stationary=False,
chunk_size=None, padding=0)`` per stream and block on a device tensor of ``latency_samples + block`` samples.  Writes
profiles/stream_ns_v1.json (``--out``) and prints it.

    python tools/bench_stream_ns.py [--streams 1,16,256,1024] [--steps 30] [--loop-repeats 3] [--out profiles/stream_ns_v1.json]
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

CONFIGS = {"16k_512_400_160": dict(sr=16000, n_fft=512, win_length=400, hop_length=160),
           "48k_defaults": dict(sr=48000, n_fft=1024, win_length=None, hop_length=None)}
LOOKAHEADS_MS = (0.0, 100.0)


def _timed(fn, repeats):
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def split_us(stages):
    """decide / fsmooth / apply / finish of a step's stage times (booked under the batched path's stage names)."""
    return [next(v for k, v in stages.items() if k.startswith(n)) for n in ("k_rg_decide", "k_rg_fsmooth", "k_rg_apply", "k_rg_ola")]


def step_ms(bank, blocks, steps, warmup):
    """(median step ms, per-stage ms of one more step)"""
    for _ in range(warmup):
        bank.push(blocks)
    torch.cuda.synchronize()
    ms = _timed(lambda: bank.push(blocks), steps)
    g = bank.gate
    g.profile_enable(True)
    g.profile_read(reset=True)
    bank.push(blocks)
    stages = {k: v[0] for k, v in g.profile_read(reset=True).items()}
    g.profile_enable(False)
    return ms, stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,256,1024")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_ns_v1.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "loop_repeats": a.loop_repeats,
              "lookaheads_ms": list(LOOKAHEADS_MS), "configs": {}}
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
            bank = nr.StreamBank(sr, S, y_noise=noise, max_block=block, **kw)
            st_ms, st_stages = step_ms(bank, blocks, a.steps, a.warmup)
            bank.close()
            row = {"block_ms": 1000.0 * block / sr, "stationary_step_ms": st_ms, "stationary_stage_ms": st_stages,
                   "lookahead": {}}
            for ms in LOOKAHEADS_MS:
                bank = nr.StreamBank(sr, S, stationary=False, lookahead_ms=ms, max_block=block, **kw)
                ns_ms, ns_stages = step_ms(bank, blocks, a.steps, a.warmup)
                ctx = torch.from_numpy(O.synth_signal(bank.latency_samples + block, sr=sr, seed=1, dtype=np.float32)).cuda()
                call = lambda: nr.reduce_noise(ctx, sr, stationary=False, chunk_size=None, padding=0, device="cuda", **kw)
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                loop = _timed(lambda: [call() for _ in range(S)], a.loop_repeats)
                row["lookahead"]["%g" % ms] = {"lookahead_frames": bank.lookahead_frames, "step_ms": ns_ms,
                                               "stage_ms": ns_stages, "latency_samples": bank.latency_samples,
                                               "state_bytes": bank.state_bytes, "loop_ms": loop,
                                               "loop_over_step": loop / ns_ms}
                print(f"[bench_stream_ns] {name} S={S} lookahead {ms:g} ms (L={bank.lookahead_frames}): step {ns_ms:.3f} ms "
                      f"(stationary {st_ms:.3f}), loop {loop:.3f} ms, decide / fsmooth / apply / finish "
                      + " / ".join("%.0f" % (1000 * v) for v in split_us(ns_stages)) + " us", flush=True)
                bank.close()
            rows[str(S)] = row
        result["configs"][name] = rows
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"stream_ns_bench": result["configs"]}))


if __name__ == "__main__":
    main()
