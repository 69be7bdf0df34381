#!/usr/bin/env python
"""Time TorchGate.gated_stft against the two ways to get a gated spectrogram without it.

  native     (i)   tg.gated_stft(x)                                   -- sg_gate_spectrum, csrc/spec.hip
  waveform   (ii)  torch.stft(tg(x), ...)                             -- what a user writes today (not the same spectrogram:
                                                                         STFT(ISTFT(Y)) != Y)
  composed   (iii) torch.stft(x, ...) * mask, mask from process_batch(save_mask=True) -- the fallback route of gated_stft
  native_lds       (i) with SG_OPT_FORCE_NOFAST: the decisions from the general kernels (k_colstats, k_decide) instead of the
                   row-fused bit-mask kernels (A/B of the decision route; the mask is bitwise the same)

256 x 16000 (BASELINE config 5), 32 x 16000 and 8 x 160000 float32 rows at the defaults, stationary and non-stationary,
forward and forward + backward.  Device events after warm-up; the candidates are ALTERNATED within each round, so that
whatever else the machine does hits all of them alike; median, min, 10th / 90th percentile of >= 20 rounds, each round
timing `--inner` back-to-back calls.  (ii) and (iii) run only TorchGate.forward / process_batch and torch.

    python tools/bench_gated_stft.py --out profiles/gated_stft_v1.json
    python tools/bench_gated_stft.py --profile-shape 256x16000     # one shape, (i) only, a few calls: for rocprofv3
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(256, 16000), (32, 16000), (8, 160000)]


def make_candidates(tg, x, backward):
    from noisereduce_amd import _ffi
    n, W, H = tg.n_fft, tg.win_length, tg.hop_length
    win = torch.hann_window(W, device=x.device)
    gate = tg._gate_for(x.device)
    F = n // 2 + 1
    T = 1 + x.shape[1] // H
    G = torch.randn(x.shape[0], F, T, 2, device=x.device)
    xg = x.clone().requires_grad_() if backward else x

    def finish(Y):
        if backward:
            xg.grad = None
            (torch.view_as_real(Y) * G).sum().backward()
        return Y

    def stft(sig):
        return torch.stft(sig, n, H, W, window=win, center=True, pad_mode="constant", return_complex=True)

    def native():
        return finish(tg.gated_stft(xg))

    def native_lds():
        with gate.with_options([(_ffi.SG_OPT_FORCE_NOFAST, 1)]):
            return finish(tg.gated_stft(xg))

    def waveform():
        return finish(stft(tg(xg)))

    def composed():
        with torch.no_grad():
            _, mask = gate.process_batch(x, None, save_mask=True)
        return finish(stft(xg) * mask[:, :, :F].transpose(1, 2))

    return {"native": native, "waveform": waveform, "composed": composed, "native_lds": native_lds}


def alternate(cands, warmup, rounds, inner):
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    out = {}
    for k, v in ms.items():
        v.sort()
        out[k] = {"median_ms": statistics.median(v), "min_ms": v[0], "p10_ms": v[int(0.1 * (len(v) - 1))],
                  "p90_ms": v[int(0.9 * (len(v) - 1))], "rounds": rounds, "inner": inner}
        out[k]["spread"] = (out[k]["p90_ms"] - out[k]["p10_ms"]) / out[k]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-shape", default=None, help="BxL: run (i) a few times at one shape and exit (for a profiler)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from noisereduce_amd.torchgate import TorchGate

    if args.profile_shape:
        B, L = (int(v) for v in args.profile_shape.split("x"))
        x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(0))).cuda()
        for nonstat in (False, True):
            tg = TorchGate(sr=16000, nonstationary=nonstat).cuda()
            for backward in (False, True):
                fn = make_candidates(tg, x, backward)["native"]
                for _ in range(6):
                    fn()
        torch.cuda.synchronize()
        return

    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "sr": 16000, "n_fft": 1024, "cases": []}
    for B, L in SHAPES:
        x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(0))
             + 0.5 * torch.sin(2 * torch.pi * 440 * torch.arange(L) / 16000)).cuda()
        for nonstat in (False, True):
            tg = TorchGate(sr=16000, nonstationary=nonstat).cuda()
            for backward in (False, True):
                cands = make_candidates(tg, x, backward)
                if nonstat:
                    cands.pop("native_lds")     # the non-stationary mask has one route
                r = alternate(cands, args.warmup, args.rounds, args.inner)
                case = {"rows": B, "samples": L, "nonstationary": nonstat, "backward": backward, "ms": r,
                        "native_over_waveform": r["native"]["median_ms"] / r["waveform"]["median_ms"],
                        "native_over_composed": r["native"]["median_ms"] / r["composed"]["median_ms"]}
                result["cases"].append(case)
                print(json.dumps(case), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
