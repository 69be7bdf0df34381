"""reduce_noise_batch against a reduce_noise loop over the same clips: one JSON line per workload, gate and I/O mode.

Workloads (synthetic, seeded tone + noise, mono float32): speech -- 4 096 clips, 16 kHz, 0.5-4 s; field -- 256 clips,
48 kHz, 1-30 s (clips above the default chunk_size exercise the chunk grid).  Both timings end in a device synchronise.
Launches per batched call come from Gate.profile_read in a separate run.

    python tools/bench_batch.py [--workloads speech,field] [--reps 3] [--io numpy,tensor]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import noisereduce_amd as nr  # noqa: E402
from noisereduce_amd import batch  # noqa: E402

WORKLOADS = {"speech": (4096, 16000, 0.5, 4.0), "field": (256, 48000, 1.0, 30.0)}


def make(name):
    n_clips, sr, lo, hi = WORKLOADS[name]
    rng = np.random.default_rng(2024)
    ys = []
    for i in range(n_clips):
        n = int(rng.uniform(lo, hi) * sr)
        t = np.arange(n) / sr
        ys.append((0.1 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * (300 + 5 * (i % 100)) * t)).astype(np.float32))
    return ys, sr


def timed(fn, reps):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="speech,field")
    ap.add_argument("--io", default="tensor,numpy")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for wl in a.workloads.split(","):
        ys_np, sr = make(wl)
        samples = sum(y.size for y in ys_np)
        ys_t = [torch.from_numpy(y).cuda() for y in ys_np]
        for stationary in (True, False):
            for io in a.io.split(","):
                ys = ys_t if io == "tensor" else ys_np
                loop_out = [nr.reduce_noise(y, sr, stationary=stationary) for y in ys]       # warm-up + reference
                outs = nr.reduce_noise_batch(ys, sr, stationary=stationary)
                err = 0.0
                for o, r in zip(outs, loop_out):
                    o = o.cpu().numpy() if isinstance(o, torch.Tensor) else o
                    r = r.cpu().numpy() if isinstance(r, torch.Tensor) else r
                    err = max(err, float(np.max(np.abs(o.astype(np.float64) - r)) / max(np.max(np.abs(r)), 1e-30)))
                t_loop = timed(lambda: [nr.reduce_noise(y, sr, stationary=stationary) for y in ys], a.reps)
                t_batch = timed(lambda: nr.reduce_noise_batch(ys, sr, stationary=stationary), a.reps)
                p = batch.plan(ys_np, sr)
                g = batch._gate_for(sr, stationary, p, dict(
                    freq_mask_smooth_hz=500, time_mask_smooth_ms=50, chunk_size=600000, prop_decrease=1.0,
                    n_std_thresh_stationary=1.5, time_constant_s=2.0, thresh_n_mult_nonstationary=2,
                    sigmoid_slope_nonstationary=10), "cuda")
                g.profile_enable(True)
                g.profile_read(reset=True)
                nr.reduce_noise_batch(ys, sr, stationary=stationary)
                prof = g.profile_read(reset=True)
                g.profile_enable(False)
                launches = int(sum(v[1] for v in prof.values()))
                print(json.dumps(dict(workload=wl, gate="stationary" if stationary else "nonstationary", io=io,
                                      clips=len(ys), samples=int(samples), sub_batches=g.clip_batches(),
                                      batch_ms=round(t_batch * 1e3, 3), loop_ms=round(t_loop * 1e3, 3),
                                      batch_msamples_s=round(samples / t_batch / 1e6, 1),
                                      loop_msamples_s=round(samples / t_loop / 1e6, 1),
                                      speedup=round(t_loop / t_batch, 2), launches_per_call=launches,
                                      launches_per_sub_batch=launches // max(1, g.clip_batches()),
                                      kernel_ms={k: round(v[0], 3) for k, v in prof.items()},
                                      max_err_rel_peak=err)), flush=True)


if __name__ == "__main__":
    main()
