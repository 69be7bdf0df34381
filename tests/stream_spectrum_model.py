"""Float64 model of the spectrum steps of a stream bank (a helper, not a test): the yardstick of
tests/test_stream_spectrum_host.py and tests/test_gpu_stream_spectrum.py.  Built only from oracle/spectralgate_oracle.py;
like tests/stream_model.py it recomputes everything from scratch at every step.

After ``n`` samples a stream has applied ``A(n) = max(0, t_dec(n) - lag + 1)`` frames (``lag`` = nt + lookahead).  A step
that takes the stream from ``n0`` to ``n1`` samples reports ``(Z * m)[:, A(n0):A(n1)]`` of the gate of the first
``t_dec(n1) + 1`` frames; the flush reports ``[:, A(n):T]`` of the whole stream's ``T`` frames.  Frame ``t`` is the frame
of samples ``[t H - h, t H - h + W)``, ``Z`` is scipy.signal.stft's (1 / sum(window))."""
import numpy as np

from oracle import spectralgate_oracle as O


def t_dec(n, W, H):
    a = n + W // 2 - W
    return a // H if a >= 0 else -1


def frames_applied(n, W, H, lag):
    """A(n): frames whose final mask is known after n samples."""
    return max(0, t_dec(n, W, H) - lag + 1)


def frames_total(N, W, H):
    return (N + 2 * (W // 2) - W) // H + 1


def transform(x_all, T, n_fft, W, H):
    """Z (F, T) of the first T frames, zeros after the last sample."""
    h = W // 2
    w = O.hann_periodic(W)
    ext = np.concatenate([np.zeros(h), x_all, np.zeros(max(0, (T - 1) * H + W - h - len(x_all)))])
    idx = np.arange(W)[None, :] + H * np.arange(T)[:, None]
    return (np.fft.rfft(ext[idx] * w, n=n_fft, axis=-1) / w.sum()).T


def stationary_gate(thresh, n_fft, W, H, p, nf, nt, smooth, top_db=80.0):
    """gate(x_all, T) -> (Z, m) of the stationary stream gate: the causal -top_db floor, prop_decrease, then the
    smoothing (summed directly: a fully gated cell is exactly 0)."""
    filt = O.smoothing_filter(nf, nt) if smooth else None

    def gate(x_all, T):
        Z = transform(x_all, T, n_fft, W, H)
        with np.errstate(invalid="ignore", divide="ignore"):
            db = 20 * np.log10(np.abs(Z) + O.EPS64)
            raw = np.maximum(db, np.maximum.accumulate(db, axis=1) - top_db) > thresh[:, None]
        m = raw * p + (1 - p)
        return Z, (O.conv2_same_direct(m, filt) if filt is not None else m)
    return gate


def nonstationary_gate(n_fft, W, H, p, nf, nt, smooth, b, L, thresh_n_mult=2, slope=10):
    """gate(x_all, T) -> (Z, m) of the non-stationary stream gate with L frames of lookahead (tests/stream_ns_model.py's
    definition), as if the stream ended with frame T - 1."""
    filt = O.smoothing_filter(nf, nt) if smooth else None

    def gate(x_all, T):
        Z = transform(x_all, T, n_fft, W, H)
        A = np.abs(Z)
        fwd = np.empty_like(A)
        prev = A[:, 0].copy()
        for t in range(T):
            prev = b * A[:, t] + (1.0 - b) * prev
            fwd[:, t] = prev
        t = np.arange(T)
        s = fwd[:, np.minimum(t + L, T - 1)].copy()
        for j in range(min(L, T - 1), -1, -1):
            act = t + j <= T - 1
            s[:, act] = b * fwd[:, t[act] + j] + (1.0 - b) * s[:, act]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            m = O.sigmoid_shifted((A - s) / s, -thresh_n_mult, slope)
        if filt is not None:
            m = O.conv2_same_direct(m, filt)
        return Z, m * p + (1.0 - p)
    return gate


def spectrum_model(blocks, gate, W, H, lag):
    """blocks: list of 1-D float64 arrays.  Returns ``[(Y, m, Z)]``, one (F, k) triple per block plus the flush's:
    the gated spectrum, the final mask and the transform of the newly applied frames."""
    x = np.zeros(0)
    F = None
    steps, done = [], 0

    def part(T, a0, a1):
        nonlocal F
        Z, m = gate(x, T)
        F = Z.shape[0]
        with np.errstate(invalid="ignore"):
            return (Z * m)[:, a0:a1], m[:, a0:a1], Z[:, a0:a1]

    for blk in blocks:
        x = np.concatenate([x, np.asarray(blk, dtype=np.float64)])
        a = frames_applied(len(x), W, H, lag)
        if a > done:
            steps.append(part(t_dec(len(x), W, H) + 1, done, a))
            done = a
        else:
            steps.append(None)
    if len(x) < W:
        raise ValueError("stream shorter than win_length")
    T = frames_total(len(x), W, H)
    steps.append(part(T, done, T))
    empty = (np.zeros((F, 0), complex), np.zeros((F, 0)), np.zeros((F, 0), complex))
    return [empty if s is None else s for s in steps]


def _pool(v, r):
    n = len(v)
    out = np.array(v, dtype=np.float64)
    for d in range(1, min(r, n - 1) + 1):
        out[d:] = np.maximum(out[d:], v[:n - d])
        out[:n - d] = np.maximum(out[:n - d], v[d:])
    return out


def frame_error(Y, want):
    """Per frame t: max_k |Y[k, t] - want[k, t]| (NaN where either is NaN counts as infinite unless both are)."""
    Y = np.asarray(Y).astype(np.complex128)
    want = np.asarray(want, dtype=np.complex128)
    assert Y.shape == want.shape, (Y.shape, want.shape)
    if Y.shape[1] == 0:
        return np.zeros(0)
    d = np.abs(Y - want)
    both = np.isnan(Y) & np.isnan(want)
    d = np.where(both, 0.0, np.where(np.isnan(d), np.inf, d))
    return d.max(axis=0)


def frame_bound(want, Z, narrow, f64_rel, eps32, pool):
    """What a frame may be off by.  The transforms and the mask are float64, so only the output's own rounding is
    allowed: ``f64_rel * max(frame peak of |Z|, 1e-3 * global peak)``; a complex64 result adds ``4 eps32 max_k |want|``
    pooled over t - pool .. t + pool."""
    if want.shape[1] == 0:
        return np.zeros(0)
    with np.errstate(invalid="ignore"):
        zpk = np.nan_to_num(np.abs(Z)).max(axis=0)
        wpk = np.nan_to_num(np.abs(want)).max(axis=0)
    b = f64_rel * np.maximum(zpk, 1e-3 * zpk.max())
    if narrow:
        b = b + 4.0 * eps32 * _pool(wpk, pool)
    return b


def bad_frames(Y, want, Z, narrow, f64_rel, eps32, pool, im_edges=True):
    """Indices of the frames over their bound, or whose bin 0 / bin F - 1 carries an imaginary part that is not +0.0."""
    err = frame_error(Y, want)
    bad = err > frame_bound(want, Z, narrow, f64_rel, eps32, pool)
    if im_edges and Y.shape[1]:
        im = np.asarray(Y).imag[[0, -1], :]
        bad = bad | np.any((im != 0) | np.signbit(im), axis=0)
    return np.flatnonzero(bad)
