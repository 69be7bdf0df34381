#!/usr/bin/env python
"""Cost of moving streams between banks: ``snapshot`` of S mono slots followed by ``restore`` into another bank, for the
three kinds of bank at the 48 kHz defaults, next to a ``push`` step of the same bank (whose code the state transfer does
not touch: the figure is there to be compared with the parent commit's, tools/bench_stream.py's timing).

Median of event-timed calls after warm-up, the streams mid-way (one second received).  Writes profiles/stream_state.json
(``--out``) and prints it.

    python tools/bench_stream_state.py [--streams 256] [--steps 30] [--out profiles/stream_state.json]
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

SR = 48000
KINDS = {"fixed": dict(), "nonstationary": dict(stationary=False, lookahead_ms=100.0, time_constant_s=0.1),
         "adaptive": dict(noise_from_stream=True, noise_memory_s=2.0)}


def _timed(fn, steps):
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def measure(kind, S, steps, warmup):
    kw = dict(KINDS[kind])
    if kind == "fixed":
        kw["y_noise"] = 0.1 * np.random.default_rng(7).standard_normal(3 * SR // 4)
    block = SR // 50
    src = nr.StreamBank(SR, S, max_block=block, **kw)
    kw.pop("y_noise", None)
    dst = nr.StreamBank(SR, S, max_block=2 * block, **kw)
    x = torch.from_numpy(np.stack([O.synth_signal(block, sr=SR, seed=s, dtype=np.float32) for s in range(min(S, 32))])).cuda()
    blocks = {s: x[s % x.shape[0]] for s in range(S)}
    for _ in range(50):                       # one second of audio: every ring is full
        src.push(blocks)
    slots = list(range(S))
    for _ in range(warmup):
        dst.restore(src.snapshot(slots))
        src.push(blocks)
    torch.cuda.synchronize()
    res = {"slots": S, "payload_bytes_per_slot": src.state_bytes_of(0), "lookahead_frames": src.lookahead_frames}
    res["snapshot_restore_ms"] = _timed(lambda: dst.restore(src.snapshot(slots)), steps)
    res["snapshot_ms"] = _timed(lambda: src.snapshot(slots), steps)
    states = src.snapshot(slots)
    res["restore_ms"] = _timed(lambda: dst.restore(states), steps)
    res["push_step_ms"] = _timed(lambda: src.push(blocks), steps)
    g = src.gate
    g.profile_enable(True)
    g.profile_read(reset=True)
    states = src.snapshot(slots)
    res["export_kernel_ms"] = sum(v[0] for v in g.profile_read(reset=True).values())
    g.profile_enable(False)
    g = dst.gate
    g.profile_enable(True)
    g.profile_read(reset=True)
    dst.restore(states)
    res["import_kernel_ms"] = sum(v[0] for v in g.profile_read(reset=True).values())
    g.profile_enable(False)
    src.close()
    dst.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_state.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "config": "48k_defaults", "kinds": {}}
    for kind in KINDS:
        r = measure(kind, a.streams, a.steps, a.warmup)
        result["kinds"][kind] = r
        print(f"[bench_stream_state] {kind} S={a.streams}: snapshot + restore {r['snapshot_restore_ms']:.3f} ms "
              f"(kernels {r['export_kernel_ms']:.3f} + {r['import_kernel_ms']:.3f} ms), {r['payload_bytes_per_slot']} bytes per "
              f"slot, push step {r['push_step_ms']:.3f} ms", flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"stream_state_bench": result["kinds"]}))


if __name__ == "__main__":
    main()
