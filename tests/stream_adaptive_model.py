"""Float64 model of the streaming stationary gate that learns its noise profile from the stream (a helper, not a test):
the yardstick of tests/test_stream_adaptive_host.py and tests/test_gpu_stream_adaptive.py.  Built only from
oracle/spectralgate_oracle.py, in the manner of tests/stream_model.py: it recomputes every frame from scratch at every
step and applies the recurrence of the definition literally, one frame after the other."""
import numpy as np

from oracle import spectralgate_oracle as O
from tests.stream_model import emitted, geometry, t_dec  # noqa: F401  (re-exported: the bank's host arithmetic)


def forget_factor(noise_memory_s, sr, H):
    """lam per frame: 1 for cumulative statistics, else exp(-H / (sr * noise_memory_s))."""
    return 1.0 if noise_memory_s is None else float(np.exp(-H / (sr * noise_memory_s)))


def learn_frames(noise_learn_s, sr, H):
    """Frames that update the statistics (None: all of them)."""
    return None if noise_learn_s is None else int(noise_learn_s * sr / H)


def recurrence(db, n_std=1.5, lam=1.0, learn=None, top_db=80.0):
    """db (F, T) -> (x, thr, raw), each (F, T): the definition, frame by frame.

    rmax = max(rmax, db); x = max(db, rmax - top_db); while learning Wn = lam Wn + 1, d = x - mu, mu += d / Wn,
    M2 = lam M2 + d (x - mu); thr = mu + n_std sqrt(M2 / Wn); raw = x > thr."""
    F, T = db.shape
    x = np.empty((F, T))
    thr = np.empty((F, T))
    raw = np.zeros((F, T), dtype=bool)
    rmax = np.full(F, -np.inf)
    Wn, mu, M2 = 0.0, np.zeros(F), np.zeros(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            rmax = np.maximum(rmax, db[:, t])
            xt = np.maximum(db[:, t], rmax - top_db)
            if learn is None or t < learn:
                Wn = lam * Wn + 1.0
                d = xt - mu
                mu = mu + d / Wn
                M2 = lam * M2 + d * (xt - mu)
            th = mu + n_std * np.sqrt(M2 / Wn)
            x[:, t], thr[:, t], raw[:, t] = xt, th, xt > th
    return x, thr, raw


def spectrum(x_all, T, n_fft, W, H):
    """Frames 0 .. T - 1 of the stream (zeros before sample 0 and after the last one): Z (F, T) and its dB field."""
    h = W // 2
    w = O.hann_periodic(W)
    ext = np.concatenate([np.zeros(h), x_all, np.zeros(max(0, (T - 1) * H + W - h - len(x_all)))])
    idx = np.arange(W)[None, :] + H * np.arange(T)[:, None]
    Z = (np.fft.rfft(ext[idx] * w, n=n_fft, axis=-1) / w.sum()).T
    with np.errstate(invalid="ignore", divide="ignore"):
        db = 20 * np.log10(np.abs(Z) + O.EPS64)
    return Z, db


def final_mask(raw, p, nf, nt, smooth, direct=False):
    m = raw * p + (1 - p)
    if not smooth:
        return m
    filt = O.smoothing_filter(nf, nt)
    return O.conv2_same_direct(m, filt) if direct else O.conv2_same(m, filt)


def adaptive_model(blocks, n_fft, W, H, p, nf, nt, smooth, n_std=1.5, lam=1.0, learn=None, top_db=80.0):
    """blocks: list of 1-D arrays.  Returns (outs, thr, raw): one output per block plus the flush tail, and the
    threshold / decision fields (F, T) of the whole stream."""
    h = W // 2
    ntl = nt if smooth else 0
    x = np.zeros(0)
    outs, done = [], 0

    def run(x_all, T):
        Z, db = spectrum(x_all, T, n_fft, W, H)
        _, thr, raw = recurrence(db, n_std, lam, learn, top_db)
        return Z, final_mask(raw, p, nf, nt, smooth), thr, raw

    for b in blocks:
        x = np.concatenate([x, np.asarray(b, dtype=np.float64)])
        n = len(x)
        e = emitted(n, W, H, ntl)
        if e > done:
            Z, m, _, _ = run(x, t_dec(n, W, H) + 1)
            with np.errstate(invalid="ignore"):
                y = O.istft_scipy(Z * m, n_fft, W, H)
            outs.append(y[done:e])
            done = e
        else:
            outs.append(np.zeros(0))
    N = len(x)
    if N < W:
        raise ValueError("stream shorter than win_length")
    T = (N + 2 * h - W) // H + 1
    Z, m, thr, raw = run(x, T)
    with np.errstate(invalid="ignore"):
        y = O.istft_scipy(Z * m, n_fft, W, H)
    full = np.zeros(N)
    full[:min(N, len(y))] = y[:N]
    outs.append(full[done:])
    return outs, thr, raw


def unit(y, sr, n_fft, W, H, freq_hz=500, time_ms=50, p=1.0, n_std=1.5, lam=1.0, learn=None):
    """The whole stream as a tests/parity_budget.py unit (the stationary gate with the model's decisions)."""
    n_fft, W, H, nf, nt, smooth, _ = geometry(sr, n_fft, W, H, freq_hz, time_ms)
    y64 = np.asarray(y, dtype=np.float64)
    N = len(y64)
    T = (N + 2 * (W // 2) - W) // H + 1
    Z, db = spectrum(y64, T, n_fft, W, H)
    _, thr, raw = recurrence(db, n_std, lam, learn)
    mask = final_mask(raw, p, nf, nt, smooth, direct=True)
    yy = O.istft_scipy(Z * mask, n_fft, W, H)
    full = np.zeros(N)
    full[:min(N, len(yy))] = yy[:N]
    cfg = dict(variant="S", stationary=True, n_fft=n_fft, W=W, H=H, prop=float(p), nf=nf, nt=nt,
               filt=O.smoothing_filter(nf, nt) if smooth else None)
    return dict(ch=0, chunk=0, x=y64, Z=Z, raw=raw, mask=mask, thresh=thr, db=db, y=full, keep=(0, N), dst=(0, N),
                want=full, cfg=cfg)


# ---- the inputs of the GPU tests (tests/test_stream_adaptive_host.py holds them to the input conditions) ---------------
# (sr, n_fft, win_length, hop_length): the one-wavefront team, W < n_fft, the 256-thread team, the 68 KB LDS case
GEOMS = [(16000, 256, 256, 64), (16000, 512, 400, 160), (48000, 1024, 1024, 256), (48000, 4096, 4096, 1024)]
MEMORY_S = (None, 0.25)
LEARN_S = (None, 0.3)


def swell(n, sr, seed, dtype=np.float32):
    """Tone + noise whose level rises by 20 dB over the stream: the profile has something to follow."""
    y = O.synth_signal(n, sr=sr, seed=seed, dtype=np.float64)
    return (y * np.linspace(0.1, 1.0, n)).astype(dtype)


def two_level(n, sr, seed=1, quiet_first=False):
    """Tone + noise; one half 30 dB down (float32-valued): the second, or the first."""
    rng = np.random.default_rng(seed)
    y = 0.1 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)
    quiet = slice(0, n // 2) if quiet_first else slice(n // 2, n)
    y[quiet] *= 10.0 ** (-30.0 / 20.0)
    return y.astype(np.float32)


# the per-hop-block cases: (quiet half first, prop_decrease).  Quiet first: the quiet half passes cells at its own level.
# Quiet second: it lies wholly below the profile the loud half left, and prop_decrease = 0.7 keeps 0.3 of it in the output.
TWO_LEVEL = ((True, 1.0), (False, 0.7))


def parity_length(geom):
    return int(1.2 * geom[0])


def parity_seed(geom, channel=0):
    return 1000 + 10 * GEOMS.index(geom) + channel


def margin_db(x, thr):
    """Smallest |x - thr| over the finite cells of frames t >= 1 (frame 0 has thr == x exactly, on any machine)."""
    d = np.abs(x[:, 1:] - thr[:, 1:])
    d = d[np.isfinite(d)]
    return float(d.min()) if d.size else np.inf
