"""Float64 model of the streaming stationary gate (a helper, not a test): the yardstick of tests/test_stream_host.py and
tests/test_gpu_stream.py.  Built only from oracle/spectralgate_oracle.py; it recomputes everything from scratch at every
step, which is what makes it a yardstick rather than a second implementation."""
import numpy as np

from oracle import spectralgate_oracle as O


def t_dec(n, W, H):
    a = n + W // 2 - W
    return a // H if a >= 0 else -1


def emitted(n, W, H, nt):
    """E(n): samples whose covering frames all have their final mask after n received."""
    return max(0, (t_dec(n, W, H) - nt + 1) * H - W // 2)


def geometry(sr, n_fft, W, H, freq_hz=500, time_ms=50):
    """(n_fft, W, H, nf, nt, smooth, nt_eff): nt_eff is the lookahead in frames (0 with smoothing off)."""
    n_fft, W, H = O.resolve_stft_params(n_fft, W, H)
    nf, nt, smooth = O.mask_smoothing_widths(sr, n_fft, H, freq_hz, time_ms)
    return n_fft, W, H, nf, nt, smooth, (nt if smooth else 0)


def stream_model(blocks, thresh, n_fft, W, H, p, nf, nt, smooth, top_db=80.0):
    """blocks: list of 1-D float64 arrays.  Returns (outs, floor_live): one output per block plus the flush tail."""
    h = W // 2
    w = O.hann_periodic(W)
    filt = O.smoothing_filter(nf, nt) if smooth else None
    ntl = nt if smooth else 0
    x = np.zeros(0)
    outs, done = [], 0

    def run(x_all, T):
        ext = np.concatenate([np.zeros(h), x_all, np.zeros(max(0, (T - 1) * H + W - h - len(x_all)))])
        idx = np.arange(W)[None, :] + H * np.arange(T)[:, None]
        Z = (np.fft.rfft(ext[idx] * w, n=n_fft, axis=-1) / w.sum()).T
        with np.errstate(invalid="ignore", divide="ignore"):
            db = 20 * np.log10(np.abs(Z) + O.EPS64)
            raw = np.maximum(db, np.maximum.accumulate(db, axis=1) - top_db) > thresh[:, None]
        m = raw * p + (1 - p)
        return Z, (O.conv2_same(m, filt) if filt is not None else m), db

    for b in blocks:
        x = np.concatenate([x, np.asarray(b, dtype=np.float64)])
        n = len(x)
        e = emitted(n, W, H, ntl)
        if e > done:
            Z, m, _ = run(x, t_dec(n, W, H) + 1)
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
    Z, m, db = run(x, T)
    with np.errstate(invalid="ignore"):
        y = O.istft_scipy(Z * m, n_fft, W, H)
    full = np.zeros(N)
    full[:min(N, len(y))] = y[:N]
    outs.append(full[done:])
    with np.errstate(invalid="ignore"):
        live = bool(np.any(db.max(axis=1) - top_db > thresh))
    return outs, live
