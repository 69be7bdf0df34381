#!/usr/bin/env python
"""Time TorchGate.gated_filterbank against the two ways to get gated log-mel features without it.

  native     tg.gated_filterbank(x, fb, log=True)                          -- sg_gate_features, csrc/feat.hip
  composed   log((tg.gated_stft(x).abs() ** 2).transpose(1, 2) @ fb + eps) -- the spectrogram materialised, the tail in torch
  waveform   the same tail on torch.stft(tg(x), ...)                       -- what a user wrote before either existed (not
                                                                              the same features: STFT(ISTFT(Y)) != Y)

256 x 16000 float32 rows, TorchGate(sr=16000) at its defaults, 80 mel bands, power 2, log; forward, and forward + backward
with a scalar loss.  Device events after warm-up; the candidates are ALTERNATED within each round, so that whatever else the
machine does hits all of them alike; median, min, 10th / 90th percentile of the rounds, each round timing `--inner`
back-to-back calls.  The three columns come from one process on one card.

    python tools/bench_gated_filterbank.py --out profiles/gated_filterbank_v1.json
    python tools/bench_gated_filterbank.py --profile           # native only, a few calls: for rocprofv3 --kernel-trace
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_gated_stft import alternate  # noqa: E402  (the same timing loop)

B, L, N_MELS, EPS = 256, 16000, 80, 1e-6


def make_candidates(tg, x, fb, backward):
    n, W, H = tg.n_fft, tg.win_length, tg.hop_length
    win = torch.hann_window(W, device=x.device)
    fbd = fb.to(x.device)
    xg = x.clone().requires_grad_() if backward else x

    def finish(feat):
        if backward:
            xg.grad = None
            feat.sum().backward()
        return feat

    def tail(Y):
        return torch.log(torch.matmul((Y.abs() ** 2).transpose(1, 2), fbd) + EPS).transpose(1, 2)

    def native():
        return finish(tg.gated_filterbank(xg, fb, power=2.0, log=True, eps=EPS))

    def composed():
        return finish(tail(tg.gated_stft(xg)))

    def waveform():
        return finish(tail(torch.stft(tg(xg), n, H, W, window=win, center=True, pad_mode="constant", return_complex=True)))

    return {"native": native, "composed": composed, "waveform": waveform}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="run native a few times, forward and backward, and exit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from noisereduce_amd.torchgate import TorchGate, mel_filterbank

    x = (0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(0))
         + 0.5 * torch.sin(2 * torch.pi * 440 * torch.arange(L) / 16000)).cuda()
    fb = mel_filterbank(16000, 1024, N_MELS)
    tg = TorchGate(sr=16000).cuda()
    if args.profile:
        for backward in (False, True):
            cands = make_candidates(tg, x, fb, backward)
            for name in ("native", "composed"):
                for _ in range(6):
                    cands[name]()
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "sr": 16000, "n_fft": 1024, "rows": B, "samples": L,
              "n_mels": N_MELS, "power": 2, "log": True, "cases": []}
    for backward in (False, True):
        r = alternate(make_candidates(tg, x, fb, backward), args.warmup, args.rounds, args.inner)
        case = {"backward": backward, "ms": r,
                "native_over_composed": r["native"]["median_ms"] / r["composed"]["median_ms"],
                "native_over_waveform": r["native"]["median_ms"] / r["waveform"]["median_ms"]}
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
