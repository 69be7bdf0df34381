#!/usr/bin/env python
"""Steady-state cost of a StreamBank feature step (``push_features``) next to the steps it replaces.

One step of 256 mono streams fed 10 ms blocks at 48 kHz as device tensors, n_fft 1024, an 80-band mel filterbank, log
features.  Four forms, each on a bank of its own:

* ``push``           the plain step;
* ``push_spectrum``  the step that stores every applied frame's (F, k) complex spectrum;
* ``spectrum_tail``  ``push_spectrum`` plus what a caller composed before ``push_features`` existed: per step one
                     ``abs() ** 2``, one matmul with the filterbank and one ``log`` over the step's spectrum buffer (the
                     cheapest composition: one buffer for all streams, three launches);
* ``push_features``  the step that reduces every applied frame over the filterbank on the device.

Method: every form is warmed up, then the forms are timed in turn, round after round (the forms alternate, so that a
drift of the machine hits all four alike); a round times ``--steps`` steps of a form, each between two device events, and
keeps their median.  Reported per form: the median of the round medians and their smallest and largest value -- the
run-to-run spread a difference has to exceed.  A tree without ``push_features`` (an older commit) reports the forms it
has, so the same tool compares ``push`` and ``push_spectrum`` across commits.

Writes profiles/stream_features.json (``--out``) and prints one JSON line.

    python tools/bench_stream_features.py [--streams 256] [--steps 40] [--warmup 15] [--rounds 7] [--out ...]"""
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

SR, N_FFT, N_MELS, EPS = 48000, 1024, 80, 1e-10
FORMS = ("push", "push_spectrum", "spectrum_tail", "push_features")


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
    block = SR // 100
    noise = 0.1 * np.random.default_rng(7).standard_normal(3 * SR // 4)
    x = torch.from_numpy(np.stack([O.synth_signal(block, sr=SR, seed=s, dtype=np.float32) for s in range(min(S, 32))])).cuda()
    blocks = {s: x[s % x.shape[0]] for s in range(S)}
    fb = mel_filterbank(SR, N_FFT, N_MELS)
    fbd = fb.cuda()
    banks = {k: nr.StreamBank(SR, S, y_noise=noise, n_fft=N_FFT, max_block=block) for k in FORMS}
    have_features = hasattr(banks["push_features"], "push_features")
    if have_features:
        banks["push_features"].set_filterbank(fb)

    def tail():
        out = banks["spectrum_tail"].push_spectrum(blocks)
        # every stream's (F, k) view lies in one (rows, F) buffer of the step: one composition for all of them
        Y = next(iter(out.values()))[1]
        base = Y._base if Y._base is not None else Y
        spec = base.view(-1, N_FFT // 2 + 1) if base.numel() % (N_FFT // 2 + 1) == 0 else base[:0].view(0, N_FFT // 2 + 1)
        return out, torch.log((spec.abs() ** 2) @ fbd + EPS)

    calls = {"push": lambda: banks["push"].push(blocks),
             "push_spectrum": lambda: banks["push_spectrum"].push_spectrum(blocks),
             "spectrum_tail": tail}
    if have_features:
        calls["push_features"] = lambda: banks["push_features"].push_features(blocks, log=True, eps=EPS)
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            per[k].append(round_median(fn, steps))
    res = {"streams": S, "block_ms": 1000.0 * block / SR, "frames_per_step": block / banks["push"].hop_length,
           "n_mels": N_MELS, "forms": {}}
    for k, v in per.items():
        res["forms"][k] = {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
    for k in FORMS:
        res["forms"].setdefault(k, "not available in this tree")
    # what the two reporting steps write per step and stream
    res["spectrum_bytes_per_step"] = int(round(S * res["frames_per_step"] * (N_FFT // 2 + 1) * 8))
    res["feature_bytes_per_step"] = int(round(S * res["frames_per_step"] * N_MELS * 4))
    for b in banks.values():
        b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_features.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_features: needs the GPU (no CPU timing stands in for it)")
    r = measure(a.streams, a.steps, a.warmup, a.rounds)
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "result": r}
    for k in FORMS:
        f = r["forms"][k]
        print("[bench_stream_features] S=%d %-14s %s" % (a.streams, k, f if isinstance(f, str) else
              "%.3f ms (rounds: %.3f .. %.3f)" % (f["ms"], f["min_ms"], f["max_ms"])), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"stream_features_bench": r}))


if __name__ == "__main__":
    main()
