#!/usr/bin/env python
"""Steady-state cost of a StreamBank spectrum step (``push_spectrum``) next to a plain ``push`` step of the same tree, and
next to what a caller had to compose before it existed.

Same geometries, stream counts and timing method as tools/bench_stream.py: S mono streams fed 20 ms blocks as device
tensors, median of event-timed steps after warm-up.  Per configuration and S:

* ``push_ms`` / ``spectrum_ms`` / ``spectrum_mask_ms``: one ``push`` / ``push_spectrum`` / ``push_spectrum(return_mask=True)``
  step;
* ``stage_ms``: the engine's own per-stage event times of one step of each kind (the stream kernels are booked under the
  batched path's stage names; the spectrum step reuses the apply stage);
* ``composed_ms``: ``push``, then one ``torch.stft`` of the emitted audio per stream.  This is a DIFFERENT QUANTITY: the
  spectrum of the overlap-added audio of the step, framed afresh (centre-padded, each step on its own), not the gated
  spectrum ``Z * mask`` the engine inverts -- it is what a caller could get, and it arrives ``win_length`` samples later;
* ``apply_added_ms`` against ``spectrum_bytes``: the time the apply stage gains and the bytes it now writes per step.

Writes profiles/stream_spectrum.json (``--out``) and prints it.

    python tools/bench_stream_spectrum.py [--streams 1,16,256,1024] [--steps 30] [--warmup 10] [--out ...]"""
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


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def stages(bank, fn):
    g = bank.gate
    g.profile_enable(True)
    g.profile_read(reset=True)
    fn()
    out = {k.split(" ")[0]: v[0] for k, v in g.profile_read(reset=True).items() if v[1] > 0}
    g.profile_enable(False)
    return out


def measure(cfg, S, steps, warmup):
    sr = cfg["sr"]
    kw = {k: v for k, v in cfg.items() if k != "sr"}
    block = sr // 50
    noise = 0.1 * np.random.default_rng(7).standard_normal(3 * sr // 4)
    x = torch.from_numpy(np.stack([O.synth_signal(block, sr=sr, seed=s, dtype=np.float32) for s in range(min(S, 32))])).cuda()
    blocks = {s: x[s % x.shape[0]] for s in range(S)}
    res = {"block_ms": 1000.0 * block / sr}
    banks = {k: nr.StreamBank(sr, S, y_noise=noise, max_block=block, **kw) for k in ("push", "spectrum", "mask", "composed")}
    W, H, n_fft = banks["push"].win_length, banks["push"].hop_length, banks["push"].n_fft
    window = torch.hann_window(W, periodic=True, device="cuda")

    def composed():
        out = banks["composed"].push(blocks)
        return [torch.stft(o, n_fft, hop_length=H, win_length=W, window=window, return_complex=True)
                for o in out.values() if o.numel() >= n_fft // 2 + 1]

    calls = {"push": lambda: banks["push"].push(blocks),
             "spectrum": lambda: banks["spectrum"].push_spectrum(blocks),
             "mask": lambda: banks["mask"].push_spectrum(blocks, return_mask=True),
             "composed": composed}
    res["push_ms"] = timed(calls["push"], steps, warmup)
    res["spectrum_ms"] = timed(calls["spectrum"], steps, warmup)
    res["spectrum_mask_ms"] = timed(calls["mask"], steps, warmup)
    res["composed_ms"] = timed(calls["composed"], steps, warmup)
    # per-stage event times: the median over a few single steps (one step's events are noisy)
    split = {k: [stages(banks[k], calls[k]) for _ in range(9)] for k in ("push", "spectrum", "mask")}
    res["stage_ms"] = {k: {name: statistics.median(s[name] for s in v) for name in v[0]} for k, v in split.items()}
    f0 = banks["spectrum"].frames(0)
    banks["spectrum"].push_spectrum(blocks)
    frames = banks["spectrum"].frames(0) - f0      # (frames per 20 ms step: block / hop on average)
    res["frames_per_step"] = block / H
    res["spectrum_bytes"] = int(round(S * (block / H) * (n_fft // 2 + 1) * 8))
    res["frames_last_step"] = frames
    res["apply_added_ms"] = res["stage_ms"]["spectrum"]["k_rg_apply"] - res["stage_ms"]["push"]["k_rg_apply"]
    res["apply_added_mask_ms"] = res["stage_ms"]["mask"]["k_rg_apply"] - res["stage_ms"]["push"]["k_rg_apply"]
    for b in banks.values():
        b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,256,1024")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_spectrum.json"))
    a = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
              "composed_is": "push + one torch.stft of the emitted audio per stream: the spectrum of the overlap-added "
                             "audio, not the gated spectrum the engine inverts; a different quantity",
              "configs": {}}
    for name, cfg in CONFIGS.items():
        rows = {}
        for S in [int(s) for s in a.streams.split(",")]:
            r = rows[str(S)] = measure(cfg, S, a.steps, a.warmup)
            print(f"[bench_stream_spectrum] {name} S={S}: push {r['push_ms']:.3f} ms, push_spectrum {r['spectrum_ms']:.3f} ms "
                  f"(+mask {r['spectrum_mask_ms']:.3f}), push + torch.stft per stream {r['composed_ms']:.3f} ms; apply stage "
                  f"+{1000 * r['apply_added_ms']:.1f} us for {r['spectrum_bytes']} bytes", flush=True)
        result["configs"][name] = rows
    if os.path.exists(a.out):   # keep what other tools put there
        try:
            old = json.load(open(a.out))
            for k in old:
                result.setdefault(k, old[k])
        except ValueError:
            pass
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"stream_spectrum_bench": result["configs"]}))


if __name__ == "__main__":
    main()
