"""Cells, banks, the numpy row model and the checks for ``TorchGate.gated_filterbank(x, fb, lengths=...)`` on the native
route (sg_gate_features_rows / sg_gate_features_rows_backward, csrc/rows.hip: k_rw_feat, k_rw_feat_bwd), shared by
tests/test_gated_filterbank_rows_host.py (the model's own check, planted defects) and
tests/test_gpu_gated_filterbank_rows.py.

The cells, inputs and per-row oracle units are tests/gated_stft_rows_cases.py's (rows of 9, 9, 16, 17, 18 and 25 frames
around the tiles of 8 and 16 frames); the features' statement, the per-frame rule and the log allowance are
tests/gated_filterbank_cases.py's; FACTOR and F64_REL are tests/parity_budget.py's.  No tolerance is defined here."""
import functools

import numpy as np

from noisereduce_amd.torchgate import mel_filterbank
from tests import gated_filterbank_cases as K
from tests import gated_stft_cases as C
from tests import gated_stft_rows_cases as R
from tests import parity_budget as PB

F32 = np.float32
EPS = K.EPS
POWERS = K.POWERS
CELLS = R.CELLS
BWD_CELLS = R.E_CELLS + [R.cell("G-256-200-37"), R.cell("G-2048-1500-333")]
# (cell, bank) of the bank variation: NT = 64 (n_fft = 512) and NT = 256 (n_fft = 2048); M = 1024 on the smallest and the
# largest frame, the LDS maximum of the backward
VARIATION = [(n, b) for n in ("E-512-512-128", "E-2048-2048-512") for b in ("mel80", "one", "dense24", "zero_last", "neg")]
VARIATION += [("E-256-256-64", "mel1024"), ("E-4096-4096-1024", "mel1024")]


@functools.lru_cache(maxsize=None)
def bank(name, n_fft):
    """(F, M) float32, read-only: tests/gated_filterbank_cases.py's banks on ``mel_filterbank(R.SR, n_fft, M)``."""
    F = n_fft // 2 + 1
    if name.startswith("mel"):
        fb = mel_filterbank(R.SR, n_fft, int(name[3:])).numpy()
    elif name == "one":
        fb = mel_filterbank(R.SR, n_fft, 1).numpy()
    elif name == "dense24":
        fb = np.random.default_rng(4100).uniform(0.05, 1.0, size=(F, 24)).astype(F32)
    elif name == "zero_last":
        fb = mel_filterbank(R.SR, n_fft, 80).numpy().copy()
        fb[:, -1] = 0.0
    elif name == "neg":
        fb = mel_filterbank(R.SR, n_fft, 40).numpy().copy()
        fb[:, ::3] *= -1.0
    else:
        raise KeyError(name)
    fb = np.ascontiguousarray(fb, dtype=F32)
    fb.setflags(write=False)
    return fb


def bank_powers(name):
    return (1,) if name == "neg" else POWERS


def dead_value(log, dtype="float64", eps=EPS):
    """What a frame at or beyond T_i holds: 0, or ln(eps) rounded to the output type."""
    v = np.log(np.float64(eps)) if log else np.float64(0.0)
    return np.array(v).astype(np.float32 if dtype == "float32" else np.float64)


# ---- the route in numpy ----------------------------------------------------------------------------------------------
def model_forward(c, us, fb, power, log=False, out_dtype="float32", defect=None, x_pad=None, gate="stat", nt_lanes=None):
    """``(feat (B, M, T), mask (B, F, T) float32)`` of the contract from the oracle's per-row units: row i's own frames hold
    ``K.features64`` of X64 and the float32 mask (or its ln(. + eps)), rounded once for a float32 result; the frames after
    them hold ``dead_value``.

    ``defect``: "stats_padded" and "last_frame" are ``R.model_forward``'s (the mask of the zero-padded row; frame T_i - 1
    transformed from the padding).  "dead_swapped": the dead frames hold ln(eps) where 0 is due and the reverse.
    "no_nyquist": bin n/2 left out.  "drop_last_filter": filter M - 1 not written when M exceeds the ``nt_lanes`` lanes of
    a team (a loop that stops after one pass)."""
    B, M, T = len(us), fb.shape[1], 1 + c["L"] // c["H"]
    inner = defect if defect in ("stats_padded", "last_frame") else None
    Y, Mk = R.model_forward(c, us, "float64", defect=inner, x_pad=x_pad, gate=gate)
    dead = dead_value(not log if defect == "dead_swapped" else log)
    feat = np.full((B, M, T), float(dead), dtype=np.float64)
    for i, u in enumerate(us):
        Ti = u["Z"].shape[1]
        X = np.array(u["Z"])
        if inner == "last_frame":
            with np.errstate(divide="ignore", invalid="ignore"):
                X = np.where(Mk[i, :, :Ti] > 0, Y[i, :, :Ti] / Mk[i, :, :Ti].astype(np.float64), X)
        lin = K.features64(X, Mk[i, :, :Ti], fb, power, nyquist=defect != "no_nyquist")
        if defect == "drop_last_filter" and nt_lanes is not None and M > nt_lanes:
            lin[M - 1] = 0.0
        feat[i, :, :Ti] = np.log(lin + EPS) if log else lin
    if out_dtype == "float32":
        feat = feat.astype(F32)
    return feat, Mk


def forward_bad(c, us, feat, Mk, fb, power, log=False, dtype="float32"):
    """row -> (frames of its own [0, T_i) over ``K.feature_check``'s bound -- with log, frames whose ln is off by more than
    ``K.log_allowed`` from the float64 ln of the float64 statement plus the rule's allowance -- and whether its dead
    frames hold exactly ``dead_value``)."""
    out = {}
    for i, u in enumerate(us):
        Ti = u["Z"].shape[1]
        got = np.asarray(feat[i, :, :Ti], dtype=np.float64)
        if log:
            want, _, allowed = K.feature_budget(u["Z"], Mk[i, :, :Ti], fb, power, u["emu_spec"])
            lo, hi = np.log(np.maximum(want - allowed, 0.0) + EPS), np.log(want + allowed + EPS)
            tol = K.log_allowed(np.log(want + EPS))
            bad = np.flatnonzero(np.any((got < lo - tol) | (got > hi + tol), axis=0))
        else:
            bad, _ = K.feature_check(got, u["Z"], Mk[i, :, :Ti], fb, power, u["emu_spec"])
        dead_ok = bool(np.all(np.asarray(feat[i, :, Ti:]) == dead_value(log, dtype)))
        out[i] = (bad.tolist(), dead_ok)
    return out


# ---- the backward in numpy -------------------------------------------------------------------------------------------
def upstream(c, M, dtype="float32", seed=0):
    """Seeded normal upstream gradient (B, M, T) in ``dtype``'s precision, NaN in the frames at or beyond T_i (never read)."""
    T = 1 + c["L"] // c["H"]
    g = np.random.default_rng(5300 + c["seed"] + seed).standard_normal((len(c["lens"]), M, T))
    for i, Ti in enumerate(R.frames_of(c)):
        g[i, :, Ti:] = np.nan
    return g.astype(np.float32 if dtype == "float32" else np.float64)


def grad_unit(u, M32, fb, g, power, log, n):
    """One row's ``PB.local_check`` unit: want = ``C.adjoint_np`` of the float64 ``K.spectrum_grad`` on the row alone (mask 1:
    G is the gradient w.r.t. X already), the emulation ``C.emulate_spec_adjoint_f32`` of that same G -- the float32 adjoint
    tests/test_gpu_gated_stft_rows.py holds the spectrum's backward to -- and its pooled per-hop-block error."""
    cfg = u["cfg"]
    G = K.spectrum_grad(u["Z"], M32, fb, g, power, log, EPS)
    ones = np.ones(G.shape)
    unit = dict(want=C.adjoint_np(G[None], ones[None], cfg["n_fft"], cfg["W"], cfg["H"], n, cfg["window"])[0], keep=(0, n),
                cfg=cfg)
    unit["emu"] = C.emulate_spec_adjoint_f32(G, ones.astype(F32), cfg, n)
    unit["bud"] = PB.budget(unit, emu=unit["emu"])
    return unit


def grad_check(gx, unit):
    """``(hop blocks over their bound, largest error / budget)`` of one row's gradient on [0, len_i)."""
    return PB.local_check(np.asarray(gx, dtype=np.float64), unit, bud=unit["bud"])
