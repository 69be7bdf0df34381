"""Inputs, float64 references and the numpy adjoint for TorchGate.gated_stft, shared by tests/test_gated_stft_host.py
(which holds every stationary input to its conditions on the oracle alone) and tests/test_gpu_gated_stft.py; further down
the per-frame metrics and the team-edge, geometry, adjoint and route cells of tests/test_gated_stft_budget_host.py and
tests/test_gpu_gated_stft_budget.py.

Signals are white noise plus a 440 Hz tone, seeded (numpy), generated in float64 and rounded to the dtype under test; the
oracle sees exactly the rounded samples and the float32-rounded Hann table TorchGate builds."""
import functools

import numpy as np
import scipy.fft
import torch

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB

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


# ----------------------------------------------------------------------------------------------------------------
# the per-frame budget: metrics, team-edge / geometry / adjoint / route cells
# (tests/test_gated_stft_budget_host.py: conditions on the oracle and planted defects; tests/test_gpu_gated_stft_budget.py)
# ----------------------------------------------------------------------------------------------------------------
# The bars of tests/test_gpu_gated_stft.py divide by the row's peak, the 440 Hz tone (~128 at n_fft = 1024) where a noise
# bin is ~2.  Here every frame of the spectrogram, and every hop block of the gradient, is held against what a float32
# pocketfft evaluation of the same operation is off by there -- the rule of tests/parity_budget.py, with its constants.
F32 = np.float32
# frames one workgroup of k_spec_fwd / k_spec_bwd handles: teams x SPEC_FPW (csrc/spec.hip: spec_teams<n_fft / 2>() x 4)
SPEC_Q = {256: 64, 512: 32, 1024: 16, 2048: 16, 4096: 4}


def spec_q_from_source():
    """SPEC_Q recomputed from spec_nt / spec_teams / SPEC_FPW as csrc/spec.hip states them (the host test compares)."""
    out = {}
    for n_fft in SPEC_Q:
        N = n_fft // 2
        nt = 256 if N >= 2048 else 16 if N <= 128 else 32 if N == 256 else 64
        teams = 1 if N >= 2048 else 256 // nt if nt < 64 else 2 if N * 8 > 16384 else 4
        out[n_fft] = teams * 4
    return out


def _frame_max(a):
    return np.max(np.abs(a), axis=0) if a.size else np.zeros(a.shape[1])


def spectrum_check(got, X64, M, cfg, x=None, emu=None):
    """One row of a gated spectrogram, frame by frame.  got: (F, T) complex, what the kernel returned; X64: the oracle's
    float64 spectrum; M: the mask THE KERNEL returned (mask error is judged separately and can neither hide nor fake a
    transform error); cfg: the unit's (``PB.torchgate_units``); ``x`` the row's samples, or ``emu`` the (F, T) complex64
    ``PB.spectrum_f32`` of the row where the caller holds it already.

    want = X64 * M in float64; the emulation is the float32 spectrum (x rounded to float32 as the kernel rounds it -- the
    transforms are float32 in both containers, so a float64 input is held to the same bound -- float32 window, pocketfft on
    float32) times M in float32.  Per frame t: err[t] = max_k |got - want| against FACTOR x (max_k |emu - want| pooled over
    t - POOL .. t + POOL) + 4 eps32 x the pooled max_k |want|.  Returns ``(frames over their bound, largest err / bud)``."""
    got = np.asarray(got, dtype=np.complex128)
    M32 = np.asarray(M, dtype=F32)
    want = np.asarray(X64, dtype=np.complex128) * M32.astype(np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if emu is None:
        emu = PB.spectrum_f32(dict(x=x, cfg=cfg))
    e = (np.asarray(emu, dtype=np.complex64) * M32).astype(np.complex64)
    err = _frame_max(got - want)
    bud = PB._pool(_frame_max(e.astype(np.complex128) - want))
    allowed = PB.FACTOR * bud + 4.0 * PB.EPS32 * PB._pool(_frame_max(want))
    nz = bud > 0
    ratio = float(np.max(err[nz] / bud[nz])) if np.any(nz) else 0.0
    return np.flatnonzero(err > allowed), ratio


def emulate_spec_adjoint_f32(G, M, cfg, L, drop_last=False, nyquist_imag=0.0):
    """``adjoint_np`` of one row in the kernels' arithmetic: M .* G in float32 (complex64), bins 0 and n/2 doubled and made
    real (``merge_model``), scipy.fft.irfft on complex64, x n/2, the float32 window, float32 overlap-add in ascending frame
    order.  G, M: (F, T).  Returns (L,) float32.  Two switches plant defects: ``drop_last`` leaves frame T - 1 out of the sums
    of the last hop block, ``nyquist_imag`` lets that share of Im G[n/2] into the real Nyquist bin."""
    n, W, H = cfg["n_fft"], cfg["W"], cfg["H"]
    F, T = np.shape(G)
    G32 = np.asarray(G).astype(np.complex64)
    Y = (G32 * np.asarray(M, dtype=F32)).astype(np.complex64)
    Y[0] = F32(2.0) * Y[0].real
    Y[-1] = F32(2.0) * (Y[-1].real + F32(nyquist_imag) * Y[-1].imag)
    fr = scipy.fft.irfft(Y.T, n=n, axis=-1)
    assert fr.dtype == F32, "scipy.fft left float32"
    wf = O._centered_window(n, W, cfg["window"]).astype(F32)
    fr = fr * F32(n // 2) * wf[None, :]
    p = n // 2
    ext = np.zeros(max(n + (T - 1) * H, p + L), dtype=F32)
    last = ((L - 1) // H) * H + p           # where the last hop block starts in ext
    for t in range(T):
        if drop_last and t == T - 1:
            a = last - t * H                # samples of the frame before the last hop block
            if a > 0:
                ext[t * H:t * H + a] += fr[t, :a]
            if t * H + n > p + L:
                ext[p + L:t * H + n] += fr[t, p + L - t * H:]
            continue
        ext[t * H:t * H + n] += fr[t]
    return ext[p:p + L]


def spec_adjoint_unit(G, M, cfg, L):
    """``want`` (``adjoint_np`` in float64, with the G and M given), the emulation and its pooled per-hop-block error, laid
    out for ``PB.local_check``."""
    want = adjoint_np(np.asarray(G)[None], np.asarray(M, dtype=np.float64)[None], cfg["n_fft"], cfg["W"], cfg["H"], L,
                      cfg["window"])[0]
    u = dict(want=want, keep=(0, L), cfg=cfg)
    u["emu"] = emulate_spec_adjoint_f32(G, M, cfg, L)
    u["bud"] = PB.budget(u, emu=u["emu"])
    return u


def spec_adjoint_check(gx, G, M, cfg, L, unit=None):
    """One row of sg_gate_spectrum_backward per hop block of H samples -- ``PB.adjoint_check_rows``' rule unchanged: G is
    what the kernel saw (rounded to its dtype), M the mask it was given.  Returns ``(hop blocks over their bound, largest
    error / budget)``."""
    u = spec_adjoint_unit(G, M, cfg, L) if unit is None else unit
    return PB.local_check(np.asarray(gx, dtype=np.float64), u, bud=u["bud"])


# ---- team-edge and geometry cells --------------------------------------------------------------------------------
# Stationary, prop_decrease = 0.5 (no cell of the mask is 0: every bin of every frame is held), B = 2, float32 and float64.
# E: win = n_fft, hop = n_fft / 4, T = Q - 1, Q, Q + 1, 2 Q + 1 (4096: the minimum row has 9 = 2 Q + 1 frames; 9, 12, 13 and
# 5 frames at hop 2048).  G: other windows and hops at T = Q + 1, or the minimum row where that is longer.
# L = (T - 1) H + r with 0 < r < H and r % 4 != 0.
EG_PROP = 0.5
EG_B = 2


def _eg(name, sr, n_fft, win, hop, T, r):
    W, H = (n_fft if win is None else win), None
    H = W // 4 if hop is None else hop
    assert 0 < r < H and r % 4 != 0
    L = (T - 1) * H + r
    assert L >= 2 * W and 1 + L // H == T, (name, L, W, T)
    return dict(name=name, sr=sr, n_fft=n_fft, win=win, hop=hop, W=W, H=H, T=T, L=L, Q=SPEC_Q[n_fft])


def _e_cells():
    cells = []
    for n_fft, sr in ((256, 16000), (512, 16000), (1024, 16000), (2048, 48000)):
        Q = SPEC_Q[n_fft]
        for T in (Q - 1, Q, Q + 1, 2 * Q + 1):
            cells.append(_eg("E-%d-T%d" % (n_fft, T), sr, n_fft, None, None, T, n_fft // 8 + 1 + 2 * (T % 3)))
    for T in (9, 12, 13):
        cells.append(_eg("E-4096-T%d" % T, 48000, 4096, None, None, T, 513 + 2 * (T % 3)))
    cells.append(_eg("E-4096-h2048-T5", 48000, 4096, None, 2048, 5, 1027))
    return cells


E_CELLS = _e_cells()
G_CELLS = [
    _eg("G-256-200-37", 16000, 256, 200, 37, 65, 21),
    _eg("G-512-400-100", 16000, 512, 400, 100, 33, 57),
    _eg("G-1024-1000-333", 16000, 1024, 1000, 333, 17, 201),
    _eg("G-1024-1024-512", 16000, 1024, 1024, 512, 17, 259),
    _eg("G-2048-1500-333", 48000, 2048, 1500, 333, 17, 150),
    _eg("G-4096-3000-700", 48000, 4096, 3000, 700, 9, 401),      # Q + 1 = 5 frames are under the minimum row of 9
]
EG_CELLS = E_CELLS + G_CELLS
# every G cell and the T = Q + 1 E cell of each n_fft (4096: the hop-2048 cell has Q + 1 = 5 frames)
ADJ_CELLS = G_CELLS + [c for c in E_CELLS if c["T"] == c["Q"] + 1]
_EG_RESEED = {}        # name -> seed offset (tests/test_gated_stft_budget_host.py holds the conditions a seed must meet)


def eg_cell_id(c):
    return c["name"]


def eg_kwargs(c):
    return dict(n_fft=c["n_fft"], win_length=c["win"], hop_length=c["hop"], prop_decrease=EG_PROP)


def eg_window64(c):
    return torch.hann_window(c["W"]).double().numpy()


@functools.lru_cache(maxsize=None)
def _eg_x(name):
    c = next(c for c in EG_CELLS if c["name"] == name)
    L, n = c["L"], c["n_fft"]
    rng = np.random.default_rng(7100 + [d["name"] for d in EG_CELLS].index(name) + _EG_RESEED.get(name, 0))
    s = np.arange(L)
    # make_x's noise, ten times louder burst and tone ...
    env = 1.0 + 9.0 * ((s >= int(0.40 * L)) & (s < int(0.52 * L)))
    x = 0.1 * env * rng.standard_normal((EG_B, L)) + 0.5 * np.sin(2 * np.pi * 440.0 * s / c["sr"])
    # ... plus half a frame of DC offset and half a frame of (-1)^s, away from the noise burst: bins 0 and n/2 carry energy
    # in the frames that reach them
    a, b = int(0.08 * L), int(0.70 * L)
    x[:, a:a + n // 2] += 0.5
    x[:, b:b + n // 2] += 0.5 * (1.0 - 2.0 * (s[b:b + n // 2] % 2))
    x.setflags(write=False)
    return x


def eg_x(c, dtype=np.float64):
    """(EG_B, L) samples of an E / G cell, generated in float64 and rounded to the dtype under test."""
    return _eg_x(c["name"]).astype(dtype)


@functools.lru_cache(maxsize=None)
def _eg_units(name, dtype_name):
    c = next(c for c in EG_CELLS if c["name"] == name)
    x = eg_x(c, np.dtype(dtype_name)).astype(np.float64)
    units = PB.torchgate_units(x, c["sr"], window=eg_window64(c), **eg_kwargs(c))[1]
    for u in units:
        u["emu_spec"] = PB.spectrum_f32(u)
        for k in ("Z", "mask", "raw", "emu_spec"):
            u[k].setflags(write=False)
    return units


def eg_units(c, dtype_name="float32"):
    """The oracle's units (one per row, ``PB.torchgate_units``) of an E / G cell on the samples rounded to ``dtype_name``,
    each with ``emu_spec``, the float32 spectrum of the row; computed once, shared, read-only."""
    return _eg_units(c["name"], dtype_name)


# ---- adjoint cells -----------------------------------------------------------------------------------------------
def adj_inputs(c, dtype=np.float64):
    """``(G (2, F, T) complex of ``dtype``'s precision, M (2, T, FS) float32)``: the mask uniform in [0.25, 1] with NaN in
    the padding columns F .. FS - 1 (never read); row 0 of G dense complex normal, row 1 zero but for 1 + 1j at six cells --
    the corners of the team loop and of the bin range; the imaginary parts at bins 0 and n/2 must leave no trace."""
    n, T, Q = c["n_fft"], c["T"], c["Q"]
    F = n // 2 + 1
    FS = (F + 15) // 16 * 16
    rng = np.random.default_rng(9300 + [d["name"] for d in EG_CELLS].index(c["name"]))
    M = np.full((2, T, FS), np.nan, dtype=F32)
    M[:, :, :F] = rng.uniform(0.25, 1.0, size=(2, T, F)).astype(F32)
    G = np.zeros((2, F, T), dtype=np.complex128)
    G[0] = rng.standard_normal((F, T)) + 1j * rng.standard_normal((F, T))
    for t, k in adj_impulses(c):
        G[1, k, t] = 1.0 + 1.0j
    return G.astype(np.complex64 if np.dtype(dtype) == np.float32 else np.complex128), M


def adj_impulses(c):
    n, T, Q = c["n_fft"], c["T"], c["Q"]
    return [(0, 0), (0, n // 2), (T - 1, n // 2), (Q, 1), (Q - 1, n // 2 - 1), (T // 2, n // 4)]


# ---- route cells -------------------------------------------------------------------------------------------------
# float32, prop_decrease = 1, rows that differ (PB.route_rows / route_noise; the width cells bring their own input).
def _rc(name, T, win=None, hop=None, xn=None):
    W = 1024 if win is None else win
    return dict(name=name, kind="own", n_fft=1024, win=win, hop=hop, W=W, H=W // 4 if hop is None else hop, T=T, B=3, xn=xn)


_OWN_R = [_rc("R-t128", 128), _rc("R-t129", 129), _rc("R-t128-xnB", 128, xn="rows"), _rc("R-t129-xnB", 129, xn="rows"),
          _rc("R-1024-1024-200", 40, 1024, 200), _rc("R-1024-800-200", 40, 800, 200),
          # ktot = 15^2 18^2 = 72900 > 65535: off the bit path at widths that are otherwise inside it (the width matrix holds
          # this edge on row-gate cells only, which sg_gate_spectrum never takes)
          dict(_rc("R-ktot", 104), widths=(14, 17))]
_TW_R = [dict(name="R-tw-" + c["name"], kind="tw", src=c) for c in PB.TW_CELLS if not c.get("rowgate")]
_M_R = [dict(name="R-" + c["name"], kind="mm", src=c) for c in PB.M_CELLS if not c["lengths"]]
R_CELLS = _OWN_R + _TW_R + _M_R
_R_RESEED = {}         # name -> seed offset (tests/test_gated_stft_budget_host.py holds the conditions a seed must meet)


def r_cell_id(c):
    return c["name"]


@functools.lru_cache(maxsize=None)
def _r_case(name):
    c = next(c for c in R_CELLS if c["name"] == name)
    if c["kind"] == "tw":
        case = PB.tw_case(c["src"])
        return dict(x=case["x"], xn=case["xn"], kw=case["kw"], sr=PB.SR, nonstationary=c["src"]["gate"] == "TNS")
    if c["kind"] == "mm":
        case = PB.m_case(c["src"])
        return dict(x=case["x"], xn=None, kw=case["kw"], sr=PB.SR, nonstationary=True)
    L = (c["T"] - 1) * c["H"] + 13
    seed = 8200 + 37 * [d["name"] for d in _OWN_R].index(name) + _R_RESEED.get(name, 0)
    x = PB.route_rows(c["B"], L, seed)
    xn = PB.route_noise(c["B"], 40 * c["H"] + 13, seed) if c["xn"] else None
    if xn is None:
        # a row that takes its thresholds from itself passes 2 - 3 % of its cells on stationary noise and a tone (make_x):
        # a ten times louder stretch over 12 % of the row, from a row-dependent sample on
        for b in range(c["B"]):
            a = int(L * (0.30 + 0.17 * b))
            x[b, a:a + int(0.12 * L)] *= F32(10.0)
    kw = dict(n_fft=1024, win_length=c["win"], hop_length=c["hop"])
    if "widths" in c:
        nf, nt = c["widths"]
        kw.update(freq_mask_smooth_hz=(nf + 0.02) * PB.R_SR / 512.0, time_mask_smooth_ms=(nt + 0.02) * 1000.0 * c["H"] / PB.R_SR)
    return dict(x=x, xn=xn, kw=kw, sr=PB.R_SR, nonstationary=False)


def r_case(c):
    """``x`` (B, L) and ``xn`` (None, (1, Ln) or (B, Ln)) float32, ``kw`` for TorchGate / ``PB.torchgate_units``, ``sr``."""
    return _r_case(c["name"])


@functools.lru_cache(maxsize=4)
def _r_units(name):
    c = next(c for c in R_CELLS if c["name"] == name)
    if c["kind"] == "tw":
        return PB.tw_oracle(c["src"])
    if c["kind"] == "mm":
        return PB.m_oracle(c["src"])
    case = _r_case(name)
    xn = None if case["xn"] is None else case["xn"].astype(np.float64)
    W = 1024 if c["win"] is None else c["win"]
    return PB.torchgate_units(case["x"].astype(np.float64), case["sr"], xn=xn, window=PB.tile_window(W), **case["kw"])[1]


def r_units(c):
    return _r_units(c["name"])


def spec_route_label(cfg, T, kbox=20, with_mask=True, nofast=False):
    """The routing of process_batch_impl with spec_dev set (csrc/api.hip; the box-mask limits: csrc/nonstat_mask.hpp),
    restated: ``(Gate.spectrum_route() without its sub-batch count, Gate.smooth_route())`` for a unit configuration
    ``cfg`` (``PB.torchgate_units``) on rows of T frames.

    * stationary, default geometry (1024 / 1024 / 256), prop_decrease = 1, ktot <= 65535 and, where it smooths,
      n_grad_time <= 96 and -- only searched for n_grad_freq <= 30 -- a k_smooth_bits2 tile that fits: decision bits, by
      k_row_decide while a (row, 64 bands) tile of float64 powers fits 64 KiB (T <= 128) and by k_t2_rows + k_decide_bits_t2
      beyond, handed to the float smoothing kernels through k_spec_bits_to_raw;
    * every other stationary gate: stage_decide;
    * non-stationary: k_box_mask<nt> for n_movemean = 20 and (no smoothing, or n_grad_freq <= 24 and 1 <= n_grad_time <=
      12), which writes the engine's own field (the mask is copied out); else stage_nonstat_raw and the float smoothing.
    The float smoothing (k_smooth_tiled where its tile fits, else the two passes) writes straight into the caller's mask."""
    smooth = cfg["filt"] is not None
    nf, nt = cfg["nf"], cfg["nt"]
    general = ("off", 4, 0) if not smooth else ("k_smooth_tiled", 4, 64) if PB.smooth_tiled_ok(nf, nt) else \
        ("k_smooth_f+k_smooth_t", 4, 0)
    if not cfg["stationary"]:
        if kbox == 20 and (not smooth or (nf <= PB.NS_MAX_NF and 1 <= nt <= 12)):
            return ("stage_box_mask", False, False), ("k_box_mask", 4, 64)
        return ("stage_nonstat_raw", False, with_mask), general
    ktot = (nf + 1) ** 2 * (nt + 1) ** 2 if smooth else 1
    fast = (cfg["n_fft"], cfg["W"], cfg["H"]) == (1024, 1024, 256)
    sm2 = True
    if smooth and nf <= 30 and ktot <= 65535 and nt <= 96:
        sm2 = PB.sm2_tile(cfg["n_fft"] // 2 + 1, nf, nt, tt_max=64) is not None
    bits = fast and not nofast and cfg["prop"] == 1.0 and ktot <= 65535 and (not smooth or (nt <= 96 and sm2))
    if not bits:
        return ("stage_decide", False, with_mask), general
    return ("k_row_decide" if T * 64 * 8 <= 64 * 1024 else "k_t2_rows+k_decide_bits_t2", True, with_mask), general
