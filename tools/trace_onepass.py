#!/usr/bin/env python3
"""Phase trace of k_gate_onepass on configs[1] (library built with -DOP_TRACE=1: tools/ab_build.sh trace -DOP_TRACE=1).
   SG_LIB_PATH=noisereduce_amd/_ab/lib_trace.so MODE=<SG_OPT_TILE_ORDER> python tools/trace_onepass.py [--table]
The library prints the per-phase average shader cycles of the last launch at exit (stderr): over all waves, and per wave index
(wave 0 draws the next ticket, waves 0 - 2 publish the trailing partial hops and finish the open seam, wave 3 does neither).
--table: runs the trace in a child process and prints the per-wave table with the two figures read off it --
  exposed ticket round trip         = phase 9 of wave 0 - mean of waves 1 - 3
  exposed store ack. + seam loads   = phase 13, mean of waves 0 - 2 - wave 3
each also as a share of a tile's summed phases (all waves)."""
import os, re, subprocess, sys, time


def table():
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    sys.stderr.write("".join(ln + "\n" for ln in r.stderr.splitlines() if "OP_TRACE" in ln or ln.startswith("MODE")))
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        sys.exit(r.returncode)
    rows, total = {}, None
    for ln in r.stderr.splitlines():
        m = re.match(r"\[OP_TRACE\] wave (\d) \((\d+) completed\):(.*)", ln)
        if m:
            rows[int(m.group(1))] = [float(x.split(":")[1]) for x in m.group(3).split()]
        m = re.match(r"\[OP_TRACE\] completed waves .*?phase:(.*?)\s+sum (\d+)", ln)
        if m:
            total = float(m.group(2))
    if len(rows) != 4 or not total:
        sys.exit("no per-wave trace on stderr: is SG_LIB_PATH a -DOP_TRACE=1 library?")
    print("library %s" % os.environ.get("SG_LIB_PATH", "(default)"))
    print("phase   " + " ".join("%6d" % k for k in range(14)) + "     sum")
    for w in range(4):
        print("wave %d  " % w + " ".join("%6.0f" % x for x in rows[w]) + "  %6.0f" % sum(rows[w]))
    tk = rows[0][9] - sum(rows[w][9] for w in (1, 2, 3)) / 3
    ep = sum(rows[w][13] for w in (0, 1, 2)) / 3 - rows[3][13]
    print("phase 9, wave 0 - mean of waves 1-3: %.0f cycles = %.2f %% of a tile's summed phases (%.0f)" % (tk, 100 * tk / total, total))
    print("phase 13, mean of waves 0-2 - wave 3: %.0f cycles = %.2f %%" % (ep, 100 * ep / total))


def trace():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from noisereduce_amd import _ffi
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    import bench
    dev = torch.device("cuda", 0)
    y = bench.synth_on_device(bench.N_PER_GPU, 1234, dev)
    KW = dict(y_noise=None, prop_decrease=1.0, n_std_thresh_stationary=1.5, clip_noise_stationary=True, chunk_size=600000,
              padding=30000, n_fft=1024, win_length=None, hop_length=None, time_constant_s=2.0, freq_mask_smooth_hz=500,
              time_mask_smooth_ms=50, tmp_folder=None, use_tqdm=False, n_jobs=1)
    sg = SpectralGateStationary(y=y, sr=48000, **KW)
    sg._gate.set_option(_ffi.SG_OPT_TILE_ORDER, int(os.environ.get("MODE", "0")))
    for _ in range(200): sg.get_traces()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(50): sg.get_traces()
    torch.cuda.synchronize()
    print("MODE", os.environ.get("MODE", "0"), "ms per call (trace build)", round((time.perf_counter() - t0) / 50 * 1e3, 4), file=sys.stderr)


if __name__ == "__main__":
    table() if "--table" in sys.argv[1:] else trace()
