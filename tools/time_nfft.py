"""Device-resident throughput of reduce_noise (stationary / non-stationary) over n_fft, including
frame lengths that run on the chirp-z kernels.  Usage: [MINUTES=2] [NFFT=512,1024,...] [SPLIT=1] python tools/time_nfft.py
SPLIT=1 sets SG_OPT_FORCE_SPLIT on the gates it times: the stationary gate then runs decide + smooth + apply (k_decide_fastN at
n_fft = 256 / 512 / 2048) instead of the one-pass kernel; the keys of the result file then end in ",split"."""
import json
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import noisereduce_amd as nr
from noisereduce_amd import _ffi

sr = 48000
SPLIT = os.environ.get("SPLIT", "0") == "1"
n = int(sr * 60 * float(os.environ.get("MINUTES", "2")))
rng = np.random.default_rng(0)
y = (0.1 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 1000 * np.arange(n) / sr)).astype(np.float32)
yd = torch.from_numpy(y).cuda()
res = {}
NFFTS = [int(a) for a in os.environ["NFFT"].split(",")] if os.environ.get("NFFT") else (256, 400, 512, 1000, 1024, 1536, 2048, 3000, 4096, 8192, 5000, 16384, 32768)
for n_fft in NFFTS:
    for stationary in (True, False):
        kw = dict(stationary=stationary, n_fft=n_fft, time_mask_smooth_ms=(400 if n_fft > 16384 else 200) if n_fft > 2048 else 50)
        if SPLIT:   # the first call creates the (cached) gate that serves this configuration
            nr.reduce_noise(y=yd, sr=sr, **kw)
            for g in list(_ffi._GATE_CACHE.values()):
                g.set_option(_ffi.SG_OPT_FORCE_SPLIT, 1)
        for _ in range(int(os.environ.get("WARM", "2"))):
            nr.reduce_noise(y=yd, sr=sr, **kw)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = int(os.environ.get("REPS", "5"))
        a.record()
        for _ in range(reps):
            nr.reduce_noise(y=yd, sr=sr, **kw)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        res[f"n_fft={n_fft},{'stat' if stationary else 'nonstat'}{',split' if SPLIT else ''}"] = dict(ms=round(ms, 3), Msamples_s=round(n / ms / 1e3, 1))
        print(n_fft, stationary, round(ms, 3), "ms", round(n / ms / 1e3, 1), "Msamples/s", flush=True)
os.makedirs("gpurun_out", exist_ok=True)
json.dump(res, open("gpurun_out/time_nfft.json", "w"), indent=1)
