#!/usr/bin/env python
"""Steady-state cost of one step of a ``StreamBank(algorithm="torchgate")`` next to the existing non-stationary bank.

One step of 256 mono streams fed 10 ms blocks at 16 kHz as device tensors, n_fft 1024 (hop 256).  Two banks at the same
lookahead of 10 frames, so that both hold the same ring of samples and apply the same frames per step:

* ``torchgate``      TorchGate's non-stationary gate, ``n_movemean_nonstationary=20`` (the moving mean reads 9 frames behind
                     and 10 ahead of the frame it decides);
* ``nonstationary``  the scipy-style non-stationary gate at ``lookahead_ms=160`` (the backward pass of a decided frame walks
                     the 11 forward rows ahead of it): the bank the package had before.

Each bank is timed in its ``push`` and, with an 80-band mel filterbank, its ``push_features`` form.  Method
(tools/bench_stream_features.py's): every form is warmed up, then the forms are timed in turn, round after round, so that a
drift of the machine hits all alike; a round times ``--steps`` steps of a form, each between two device events, and keeps
their median.  Reported per form: the median of the round medians and their smallest and largest value.

Writes profiles/stream_tg.json (``--out``) and prints one JSON line.

    python tools/bench_stream_tg.py [--streams 256] [--steps 40] [--warmup 15] [--rounds 7] [--out ...]"""
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
from noisereduce_amd.torchgate import mel_filterbank  # noqa: E402
from oracle import spectralgate_oracle as O  # noqa: E402

SR, N_FFT, N_MELS, K = 16000, 1024, 80, 20


def round_median(fn, steps):
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def measure(S, steps, warmup, rounds):
    block, H = SR // 100, N_FFT // 4
    x = torch.from_numpy(np.stack([O.synth_signal(block, sr=SR, seed=s, dtype=np.float32) for s in range(min(S, 32))])).cuda()
    blocks = {s: x[s % x.shape[0]] for s in range(S)}
    fb = mel_filterbank(SR, N_FFT, N_MELS)
    L = K - 1 - (K - 1) // 2

    def tg():
        return nr.StreamBank(SR, S, n_fft=N_FFT, max_block=block, algorithm="torchgate", stationary=False, n_movemean_nonstationary=K)

    def ns():
        return nr.StreamBank(SR, S, n_fft=N_FFT, max_block=block, stationary=False, lookahead_ms=L * H / SR * 1000.0)

    banks = {"torchgate push": tg(), "nonstationary push": ns(), "torchgate push_features": tg(), "nonstationary push_features": ns()}
    assert all(b.lookahead_frames == L for b in banks.values())
    calls = {}
    for k, b in banks.items():
        if k.endswith("features"):
            b.set_filterbank(fb)
            calls[k] = (lambda b=b: b.push_features(blocks, log=True, eps=1e-6, scale="torch"))
        else:
            calls[k] = (lambda b=b: b.push(blocks))
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            per[k].append(round_median(fn, steps))
    res = {"streams": S, "block_ms": 1000.0 * block / SR, "frames_per_step": block / H, "lookahead_frames": L, "n_movemean": K,
           "state_bytes": {k: b.state_bytes for k, b in banks.items() if k.endswith("push")}, "forms": {}}
    for k, v in per.items():
        res["forms"][k] = {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    for b in banks.values():
        b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_tg.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_tg: needs the GPU (no CPU timing stands in for it)")
    r = measure(a.streams, a.steps, a.warmup, a.rounds)
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "result": r}
    for k, f in r["forms"].items():
        print("[bench_stream_tg] S=%d %-28s %.3f ms (rounds: %.3f .. %.3f)" % (a.streams, k, f["ms"], f["min_ms"], f["max_ms"]),
              flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"stream_tg_bench": r}))


if __name__ == "__main__":
    main()
