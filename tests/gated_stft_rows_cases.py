"""Cells, inputs, float64 references and the numpy row model for ``TorchGate.gated_stft(x, lengths=...)``, shared by
tests/test_gated_stft_rows_host.py (the inputs' conditions on the oracle alone, planted defects) and
tests/test_gpu_gated_stft_rows.py.

What can go wrong on this route is set by the tile edges of csrc/rows.hip -- FPT = 8 frames per transform tile, RPT = 16
per smoothing tile -- so one padded batch per cell holds rows of T_i = 9 (the minimum row, and FPT + 1), 9, 16, 17, 18 and
25 frames, the last one filling the tensor.  Inputs are tests/test_gpu_rows.py's ``make_rows``; the oracle sees each row
alone, cut at its own length, rounded to the dtype under test, with the float32 Hann table TorchGate builds.  No tolerance
is defined here: the metrics are tests/gated_stft_cases.py's and tests/parity_budget.py's."""
import functools

import numpy as np
import torch

from tests import gated_stft_cases as C
from tests import parity_budget as PB
from tests.test_gpu_rows import make_rows

SR = 16000
FPT, RPT = 8, 16
PROP = 0.5             # no cell of the mask is 0: every bin of every frame is held
GATES = ("stat", "nonstat")
DTYPES = ("float32", "float64")
NATIVE = (256, 512, 1024, 2048, 4096)


def row_lengths(W, H):
    """2 W, 2 W + 1, 16 H - 1, 16 H, 18 H - 1 and 24 H + H / 2 + 1 samples (the padded length), clamped to >= 2 W."""
    return [max(2 * W, n) for n in (2 * W, 2 * W + 1, 16 * H - 1, 16 * H, 18 * H - 1, 24 * H + H // 2 + 1)]


def _cell(kind, n_fft, W, H):
    lens = row_lengths(W, H)
    return dict(name="%s-%d-%d-%d" % (kind, n_fft, W, H), kind=kind, n_fft=n_fft, W=W, H=H, lens=lens, L=max(lens),
                seed=n_fft + H)


E_CELLS = [_cell("E", n, n, n // 4) for n in NATIVE]
G_CELLS = [_cell("G", *g) for g in ((256, 200, 37), (512, 400, 100), (1024, 1000, 333), (2048, 1500, 333),
                                    (4096, 3000, 700), (4096, 4096, 2048))]
CELLS = E_CELLS + G_CELLS
_RESEED = {}           # name -> seed offset (tests/test_gated_stft_rows_host.py holds the conditions a seed must meet)


def cell_id(c):
    return c["name"]


def cell(name):
    return next(c for c in CELLS if c["name"] == name)


def frames_of(c):
    return [1 + n // c["H"] for n in c["lens"]]


def gate_kwargs(c, gate="stat", prop=PROP):
    kw = dict(n_fft=c["n_fft"], win_length=c["W"], hop_length=c["H"], prop_decrease=prop)
    if c["n_fft"] == 4096:
        kw["time_mask_smooth_ms"] = 200      # the default 50 ms is under one hop of 1024 samples at 16 kHz
    if gate == "nonstat":
        kw["nonstationary"] = True
    return kw


def window64(c):
    """The float32 Hann table TorchGate hands the engine, as float64."""
    return torch.hann_window(c["W"]).double().numpy()


def rows(c, dtype="float32", pad=0.0):
    """(B, L) torch tensor of the cell, row i valid on [0, lens[i]) and ``pad`` after it."""
    dt = torch.float32 if dtype == "float32" else torch.float64
    return make_rows(c["lens"], c["L"], c["seed"] + _RESEED.get(c["name"], 0), dt, pad=pad)


@functools.lru_cache(maxsize=None)
def _units(name, gate, dtype):
    c = cell(name)
    x = rows(c, dtype).double().numpy()
    units = []
    for i, n in enumerate(c["lens"]):
        u = PB.torchgate_units(x[i:i + 1, :n], SR, window=window64(c), **gate_kwargs(c, gate))[1][0]
        u["emu_spec"] = PB.spectrum_f32(u)
        for k in ("Z", "mask", "raw", "emu_spec"):
            u[k].setflags(write=False)
        units.append(u)
    return units


def units(c, gate="stat", dtype="float32"):
    """The oracle's unit of every row ALONE (``PB.torchgate_units`` on ``x[i, :lens[i]]`` rounded to ``dtype``), each with
    ``emu_spec``; computed once, shared, read-only."""
    return _units(c["name"], gate, dtype)


# ---- the route in numpy: what the kernels must return, and the defects a wrong one would show --------------------------
def model_forward(c, us, out_dtype="float32", defect=None, x_pad=None, gate="stat"):
    """``(Y (B, F, T) complex, M (B, F, T) float32)`` of the contract, from the oracle's per-row units: row i's own frames
    hold X64 * float32(mask), rounded once to complex64 for a float32 result; the frames after them are zero.

    ``defect`` plants what a wrong rows pipeline would do:
      "stats_padded"   the row's mask is the one of the zero-padded row of L samples (statistics over the padding frames);
      "last_frame"     frame T_i - 1 is transformed from ``x_pad`` (B, L), whose padding is not zero;
      "smooth_1mp"     the mask smoothing sees cells of value 1 - p (blocked cells) beyond T_i instead of nothing."""
    B, F, T = len(us), c["n_fft"] // 2 + 1, 1 + c["L"] // c["H"]
    Y = np.zeros((B, F, T), dtype=np.complex128)
    M = np.zeros((B, F, T), dtype=np.float32)
    for i, u in enumerate(us):
        Ti = u["Z"].shape[1]
        X, m = np.array(u["Z"]), np.array(u["mask"])
        if defect == "stats_padded" and c["lens"][i] < c["L"]:
            xz = np.zeros((1, c["L"]))
            xz[0, :c["lens"][i]] = u["x"]
            m = PB.torchgate_units(xz, SR, window=window64(c), **gate_kwargs(c, gate))[1][0]["mask"][:, :Ti]
        if defect == "smooth_1mp" and Ti < T:
            nt = u["cfg"]["nt"]
            ext = np.concatenate([u["raw"], np.zeros((F, min(nt, T - Ti)))], axis=1)
            m = PB._final_mask(ext, u["cfg"])[:, :Ti]
        if defect == "last_frame" and c["lens"][i] < c["L"]:
            Xp = PB.torchgate_units(np.asarray(x_pad[i:i + 1], dtype=np.float64), SR, window=window64(c),
                                    **gate_kwargs(c, gate))[1][0]["Z"]
            X[:, Ti - 1] = Xp[:, Ti - 1]
        M[i, :, :Ti] = m.astype(np.float32)
        Y[i, :, :Ti] = X * M[i, :, :Ti].astype(np.float64)
    if out_dtype == "float32":
        Y = Y.astype(np.complex64)
    return Y, M


def model_backward(c, G, M, defect=None):
    """grad_x (B, L) float64 of the contract: ``adjoint_np`` of every row alone on [0, len_i) with its own T_i frames, 0
    from len_i on.  G, M: (B, F, T).  ``defect`` "leak": the first sample at len_i holds what the adjoint of the padded
    row would put there."""
    B, L = len(c["lens"]), c["L"]
    gx = np.zeros((B, L))
    for i, n in enumerate(c["lens"]):
        Ti = 1 + n // c["H"]
        full = C.adjoint_np(G[i:i + 1, :, :Ti], M[i:i + 1, :, :Ti], c["n_fft"], c["W"], c["H"], min(L, n + 1), window64(c))[0]
        gx[i, :n] = full[:n]
        if defect == "leak" and n < L:
            gx[i, n] = full[n]
    return gx


def grad_fields(c, dtype="float32", seed=0):
    """name -> G (B, F, T) complex of ``dtype``'s precision: a dense complex normal field, and per row one cell 1 + 1j at
    its frame T_i - 1, bin 0 / bin n/2 (the imaginary part there must leave no trace).  Frames at or beyond T_i hold NaN:
    the backward never reads them."""
    B, F, T = len(c["lens"]), c["n_fft"] // 2 + 1, 1 + c["L"] // c["H"]
    rng = np.random.default_rng(9700 + c["seed"] + seed)
    ct = np.complex64 if dtype == "float32" else np.complex128
    out = {"dense": rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T)),
           "last_dc": np.zeros((B, F, T), dtype=np.complex128), "last_nyquist": np.zeros((B, F, T), dtype=np.complex128)}
    for i, Ti in enumerate(frames_of(c)):
        out["last_dc"][i, 0, Ti - 1] = 1.0 + 1.0j
        out["last_nyquist"][i, F - 1, Ti - 1] = 1.0 + 1.0j
    for G in out.values():
        for i, Ti in enumerate(frames_of(c)):
            G[i, :, Ti:] = np.nan
    return {k: v.astype(ct) for k, v in out.items()}
