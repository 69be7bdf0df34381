"""Time per step of a fixed-profile StreamBank, default against exact: 256 mono streams at 48 kHz,
default geometry, 480-sample blocks.  Per case 20 steps of warm-up, then 200 steps end to end with numpy blocks (host clock;
the step synchronises) and 200 steps with device tensors whose four launches are timed by the engine's events; p10 / median /
p90 of each.

usage: bench_stream_exact.py <label> <case>...    case = default-f32 | exact-i16 | exact-f64; one JSON line per case.
The default-f32 case runs on any commit that has StreamBank (put that commit's tree first on PYTHONPATH)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

def main():
    label, cases = sys.argv[1], sys.argv[2:]
    from noisereduce_amd import stream
    sr, S, n = 48000, 256, 480
    rng = np.random.default_rng(0)
    noise = 0.1 * rng.standard_normal(3 * sr // 4)
    base = 0.1 * rng.standard_normal((S, 64 * n)) + 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(64 * n) / sr)
    for case in cases:
        kw, dt, scale = {}, np.float32, 1.0
        if case == "exact-i16":
            kw, dt, scale = dict(precision="float64"), np.int16, 20000.0
        elif case == "exact-f64":
            kw, dt = dict(precision="float64"), np.float64
        y = np.round(base * scale).astype(dt) if dt == np.int16 else base.astype(dt)
        bank = stream.StreamBank(sr, S, y_noise=noise * scale, max_block=n, **kw)
        blocks = [{s: y[s, i * n:(i + 1) * n] for s in range(S)} for i in range(64)]
        dev_blocks = [{s: torch.from_numpy(np.array(v)).cuda() for s, v in b.items()} for b in blocks[:8]]
        for i in range(20):                      # warm-up: allocations, first launches, the streams reach steady state
            bank.push(blocks[i % 64])
        torch.cuda.synchronize()
        e2e = []
        for i in range(200):
            t0 = time.perf_counter()
            bank.push(blocks[i % 64])            # numpy in, numpy out: synchronises
            e2e.append((time.perf_counter() - t0) * 1e3)
        g = bank.gate
        g.profile_enable(True)
        g.profile_read(reset=True)
        dev = []
        for i in range(200):
            bank.push(dev_blocks[i % 8])
            torch.cuda.synchronize()
            dev.append(sum(v[0] for v in g.profile_read(reset=True).values()))
        g.profile_enable(False)
        q = lambda a: [float(np.percentile(a, p)) for p in (10, 50, 90)]
        print(json.dumps(dict(label=label, case=case, streams=S, block=n, reps=200, e2e_ms_p10_p50_p90=q(e2e),
                              device_ms_p10_p50_p90=q(dev))), flush=True)
        bank.close()

main()
