"""Float64 model of the streaming non-stationary gate (a helper, not a test): the yardstick of
tests/test_stream_ns_host.py and tests/test_gpu_stream_ns.py.  Built only from oracle/spectralgate_oracle.py; like
tests/stream_model.py it recomputes everything from scratch at every step.

The level of frame ``t`` is the oracle's forward-backward smoother of the signal as known ``L`` frames later: with ``e =
min(t + L, T - 1)``, ``s = fwd[f, e]``, then ``s = b fwd[f, k] + (1 - b) s`` for ``k = e, ..., t``."""
import numpy as np

from oracle import spectralgate_oracle as O
from tests.stream_model import emitted, geometry, t_dec  # noqa: F401  (the emission arithmetic is the stationary model's)


def forward_pass(b, A):
    """O.filtfilt_onepole's forward pass: fwd[f, -1] = A[f, 0], fwd[f, t] = b A[f, t] + (1 - b) fwd[f, t - 1]."""
    A = np.asarray(A, dtype=np.float64)
    fwd = np.empty_like(A)
    prev = A[..., 0].copy()
    for t in range(A.shape[-1]):
        prev = b * A[..., t] + (1.0 - b) * prev
        fwd[..., t] = prev
    return fwd


def smoothed_level(b, fwd, L):
    """S_L (F, T) from the forward pass of all T frames: every (band, frame) runs its own recursion k = e .. t in that
    order (vectorised over bands and frames; the operations per cell are the contract's, in its order)."""
    T = fwd.shape[-1]
    t = np.arange(T)
    s = fwd[..., np.minimum(t + L, T - 1)].copy()
    for j in range(min(L, T - 1), -1, -1):
        act = t + j <= T - 1
        s[..., act] = b * fwd[..., t[act] + j] + (1.0 - b) * s[..., act]
    return s


def stream_ns_model(blocks, n_fft, W, H, p, nf, nt, smooth, b, L, thresh_n_mult=2, slope=10, direct=False):
    """blocks: list of 1-D float64 arrays.  Returns one output per block plus the flush tail.  ``direct``: sum the mask
    smoothing directly (O.conv2_same_direct) instead of through an FFT, which would spread one NaN cell over the mask."""
    h = W // 2
    w = O.hann_periodic(W)
    filt = O.smoothing_filter(nf, nt) if smooth else None
    lag = (nt if smooth else 0) + L
    conv = O.conv2_same_direct if direct else O.conv2_same
    x = np.zeros(0)
    outs, done = [], 0

    def run(x_all, T):
        """The gate of the first T frames as if the stream ended with frame T - 1.  Rows after T - 1 - L are not decided
        yet when it does not; no sample emitted so far reads them."""
        ext = np.concatenate([np.zeros(h), x_all, np.zeros(max(0, (T - 1) * H + W - h - len(x_all)))])
        idx = np.arange(W)[None, :] + H * np.arange(T)[:, None]
        Z = (np.fft.rfft(ext[idx] * w, n=n_fft, axis=-1) / w.sum()).T
        A = np.abs(Z)
        S = smoothed_level(b, forward_pass(b, A), L)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            m = O.sigmoid_shifted((A - S) / S, -thresh_n_mult, slope)
        if filt is not None:
            m = conv(m, filt)
        m = m * p + np.ones(m.shape) * (1.0 - p)
        with np.errstate(invalid="ignore"):
            return O.istft_scipy(Z * m, n_fft, W, H)

    for blk in blocks:
        x = np.concatenate([x, np.asarray(blk, dtype=np.float64)])
        n = len(x)
        e = emitted(n, W, H, lag)
        if e > done:
            y = run(x, t_dec(n, W, H) + 1)
            outs.append(y[done:e])
            done = e
        else:
            outs.append(np.zeros(0))
    N = len(x)
    if N < W:
        raise ValueError("stream shorter than win_length")
    y = run(x, (N + 2 * h - W) // H + 1)
    full = np.zeros(N)
    full[:min(N, len(y))] = y[:N]
    outs.append(full[done:])
    return outs
