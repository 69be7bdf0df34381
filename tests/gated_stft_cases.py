"""Inputs, float64 references and the numpy adjoint for TorchGate.gated_stft, shared by tests/test_gated_stft_host.py
(which holds every stationary input to its conditions on the oracle alone) and tests/test_gpu_gated_stft.py.

Signals are white noise plus a 440 Hz tone, seeded (numpy), generated in float64 and rounded to the dtype under test; the
oracle sees exactly the rounded samples and the float32-rounded Hann table TorchGate builds."""
import functools

import numpy as np
import torch

from oracle import spectralgate_oracle as O

# case -> sr, n_fft, win_length, hop_length (None: TorchGate's defaults), B, L
CASES = {
    "a": dict(sr=16000, n_fft=1024, win=None, hop=None, B=3, L=2300),     # T = 9: the minimum row + a 252-sample tail
    "b": dict(sr=16000, n_fft=512, win=400, hop=100, B=3, L=1000),        # centred short window, hop not n/4
    "c": dict(sr=16000, n_fft=256, win=None, hop=None, B=3, L=700),       # four-frames-per-transform geometry
    "d": dict(sr=48000, n_fft=2048, win=None, hop=None, B=2, L=4500),
    "e": dict(sr=48000, n_fft=4096, win=None, hop=None, B=2, L=8300),     # LDS transform shared by a whole workgroup
    "f": dict(sr=16000, n_fft=1024, win=None, hop=None, B=2, L=17000),    # T = 67 > 64 frames
    "g": dict(sr=16000, n_fft=1024, win=None, hop=None, B=161, L=2300),   # > 160 rows, several workgroup rounds
    "h": dict(sr=16000, n_fft=400, win=None, hop=None, B=2, L=1700),      # composed route
}
XN_LEN = 2100

# variant -> TorchGate keyword arguments on top of the case, and the kind of xn
VARIANTS = {
    "plain": (dict(), None),
    "nonstat": (dict(nonstationary=True), None),
    "xn1": (dict(), "one"),
    "xnB": (dict(), "batch"),
    "prop": (dict(prop_decrease=0.7), None),
    "nosmooth": (dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=None), None),
}

# every variant at case a and at one case that is not n_fft = 1024
RUNS = [("a", v) for v in VARIANTS] + [
    ("b", "plain"), ("b", "nonstat"), ("b", "xnB"), ("b", "prop"),
    ("c", "plain"), ("c", "xn1"), ("c", "nosmooth"),
    ("d", "plain"), ("d", "nonstat"),
    ("e", "plain"), ("e", "prop"),
    ("f", "plain"), ("f", "nonstat"),
    ("g", "plain"),
    ("h", "plain"), ("h", "nonstat"),
]
RUN_IDS = [f"{c}-{v}" for c, v in RUNS]
BACKWARD_RUNS = [("a", "plain"), ("a", "nonstat"), ("a", "xn1"), ("a", "prop"), ("b", "plain"), ("c", "plain"),
                 ("d", "plain"), ("e", "plain"), ("f", "plain"), ("g", "plain"), ("h", "plain")]
BACKWARD_IDS = [f"{c}-{v}" for c, v in BACKWARD_RUNS]
# chosen so that no cell of a stationary run lies within 1e-6 dB of its threshold (test_gated_stft_host.py checks it)
SEEDS = dict(a=100, b=101, c=102, d=103, e=104, f=105, g=107, h=107)


def geometry(case):
    c = CASES[case]
    return O.resolve_stft_params(c["n_fft"], c["win"], c["hop"])


def window64(case):
    """The float32 Hann table TorchGate hands the engine, as float64."""
    return torch.hann_window(geometry(case)[1]).double().numpy()


def make_x(case, dtype=np.float64):
    c = CASES[case]
    rng = np.random.default_rng(SEEDS[case])
    t = np.arange(c["L"], dtype=np.float64) / c["sr"]
    # Stationary noise alone puts 2 - 3 % of the cells above mean + 1.5 std of their band: too few for a fair mask test.
    # A ten times louder noise burst over 12 % of the row lifts that to 6 % or more in every row of every case.
    s = np.arange(c["L"])
    env = 1.0 + 9.0 * ((s >= int(0.40 * c["L"])) & (s < int(0.52 * c["L"])))
    x = 0.1 * env * rng.standard_normal((c["B"], c["L"])) + 0.5 * np.sin(2 * np.pi * 440.0 * t)
    return x.astype(dtype)


def make_xn(case, kind, dtype=np.float64):
    """Noise-only rows, a little quieter than the noise in x: (1, XN_LEN) or (B, XN_LEN)."""
    if kind is None:
        return None
    rng = np.random.default_rng(SEEDS[case] + 1000)
    rows = 1 if kind == "one" else CASES[case]["B"]
    return (0.08 * rng.standard_normal((rows, XN_LEN))).astype(dtype)


def gate_kwargs(case, variant):
    c = CASES[case]
    kw = dict(n_fft=c["n_fft"], win_length=c["win"], hop_length=c["hop"])
    kw.update(VARIANTS[variant][0])
    return kw


@functools.lru_cache(maxsize=None)
def oracle(case, variant, dtype_name):
    """(y, stages) of O.torchgate_T for the run at the given input dtype: computed once, shared, never modified."""
    dtype = np.dtype(dtype_name)
    x = make_x(case, dtype).astype(np.float64)
    xn = make_xn(case, VARIANTS[variant][1], dtype)
    y, st = O.torchgate_T(x, CASES[case]["sr"], xn=None if xn is None else xn.astype(np.float64),
                          window=window64(case), return_stages=True, **gate_kwargs(case, variant))
    for a in (y, st["X"], st["mask"], st["raw"]):
        a.setflags(write=False)
    return y, st


def adjoint_np(G, M, n_fft, W, H, L, window=None):
    """Adjoint of x -> STFT(x) * M for the real inner product (sum Re a Re b + Im a Im b), float64:
    grad_x = frames^T( w * Re sum_{k=0}^{n/2} M[k] G[k] e^{+2 pi i k j / n} ), every bin with weight 1, un-normalised
    overlap-add onto the n_fft/2-extended row, cropped to [0, L).  G, M: (B, F, T)."""
    G = np.asarray(G, dtype=np.complex128)
    M = np.asarray(M, dtype=np.float64)
    B, F, T = G.shape
    wf = O._centered_window(n_fft, W, window)
    full = np.zeros((B, n_fft, T), dtype=np.complex128)
    full[:, :F, :] = M * G
    frames = np.real(np.fft.ifft(full, axis=1)) * n_fft * wf[None, :, None]
    p = n_fft // 2
    ext = np.zeros((B, max(n_fft + (T - 1) * H, p + L)))
    for t in range(T):
        ext[:, t * H:t * H + n_fft] += frames[:, :, t]
    return ext[:, p:p + L]


def merge_model(G, M, n_fft):
    """The half-size route the adjoint kernel takes, in numpy: Y = M .* G with bins 0 and n/2 doubled and made real, read as
    the Hermitian half of a length-n spectrum; N * irfft(Y) with N = n/2 is the un-windowed adjoint frame.  (B, n, T)."""
    Y = np.asarray(M, dtype=np.float64) * np.asarray(G, dtype=np.complex128)
    Y[:, 0, :] = 2.0 * Y[:, 0, :].real
    Y[:, -1, :] = 2.0 * Y[:, -1, :].real
    return np.fft.irfft(Y, n=n_fft, axis=1) * (n_fft // 2)
