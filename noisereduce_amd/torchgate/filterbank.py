"""Filterbanks for ``TorchGate.gated_filterbank``: the mel bank from its formulas, the validation of a bank handed in, and
the support tables the engine derives from it (restated in numpy for the tests)."""
import math

import numpy as np
import torch

MAX_FILTERS = 1024   # FEAT_MAX_FILTERS of csrc/feat.hpp


def _hz_to_mel(f, scale):
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    # Slaney (Auditory Toolbox): linear below 1 kHz at 200 / 3 Hz per mel, logarithmic above with 27 steps per factor 6.4
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m, scale):
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels, f_min=0.0, f_max=None, scale="htk", norm=None):
    """Triangular mel filters on the ``n_fft // 2 + 1`` bin frequencies ``k * sr / n_fft``: (F, n_mels) float32 on the CPU.

    ``n_mels + 2`` points equally spaced on the mel scale between ``f_min`` and ``f_max`` (default ``sr / 2``) are the
    filters' edges: filter m rises linearly in Hz from edge m to its centre, edge m + 1, where it is 1, and falls to 0 at
    edge m + 2.  ``scale``: "htk" (``2595 log10(1 + f / 700)``) or "slaney" (linear below 1 kHz, logarithmic above).
    ``norm="slaney"`` divides filter m by half its width in Hz, ``2 / (f[m + 2] - f[m])``: unit area."""
    if scale not in ("htk", "slaney"):
        raise ValueError(f"scale must be 'htk' or 'slaney', got {scale!r}")
    if norm not in (None, "slaney"):
        raise ValueError(f"norm must be None or 'slaney', got {norm!r}")
    n_mels = int(n_mels)
    if n_mels < 1:
        raise ValueError("n_mels must be at least 1")
    f_max = sr / 2.0 if f_max is None else float(f_max)
    if not 0.0 <= f_min < f_max:
        raise ValueError("need 0 <= f_min < f_max")
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * (float(sr) / n_fft)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(f_min, scale), _hz_to_mel(f_max, scale), n_mels + 2), scale)
    width = np.diff(edges)                                    # (n_mels + 1,)
    slopes = edges[None, :] - freqs[:, None]                  # (F, n_mels + 2)
    up = -slopes[:, :-2] / width[None, :-1]
    down = slopes[:, 2:] / width[None, 1:]
    fb = np.maximum(0.0, np.minimum(up, down))
    if norm == "slaney":
        fb = fb * (2.0 / (edges[2:] - edges[:-2]))[None, :]
    return torch.from_numpy(fb.astype(np.float32))


def check_filterbank(fb, n_bins):
    """The bank as a C-contiguous (F, M) float32 numpy array, or ValueError: a wrong shape, M outside 1 .. 1024, a
    non-finite entry, or a tensor that asks for a gradient (the bank is a constant: a missing gradient is never silent).  A
    device tensor is copied to the host here, which synchronises."""
    if isinstance(fb, torch.Tensor):
        if fb.requires_grad:
            raise ValueError("the filterbank is a constant: fb.requires_grad must be False")
        if fb.is_complex():
            raise ValueError("the filterbank must be real")
        if fb.ndim != 2 or fb.shape[0] != n_bins:
            raise ValueError(f"the filterbank must be ({n_bins}, M), got {tuple(fb.shape)}")
        if not 1 <= fb.shape[1] <= MAX_FILTERS:
            raise ValueError(f"the filterbank must have 1 to {MAX_FILTERS} filters, got {fb.shape[1]}")
        a = fb.detach().to(device="cpu", dtype=torch.float32).contiguous().numpy()
    else:
        a = np.asarray(fb)
        if a.dtype.kind not in "fiub":
            raise ValueError("the filterbank must be real")
        if a.ndim != 2 or a.shape[0] != n_bins:
            raise ValueError(f"the filterbank must be ({n_bins}, M), got {a.shape}")
        if not 1 <= a.shape[1] <= MAX_FILTERS:
            raise ValueError(f"the filterbank must have 1 to {MAX_FILTERS} filters, got {a.shape[1]}")
        a = np.ascontiguousarray(a, dtype=np.float32)
    if not np.isfinite(a).all():
        raise ValueError("the filterbank has a non-finite entry")
    return a


def support_tables(fb):
    """``(khull (M, 2), mhull (F, 2))`` int32 of an (F, M) bank, as csrc/feat_tables.hpp builds them: the hull
    ``[k_lo, k_hi)`` of every filter's non-zero bins and the hull ``[m_lo, m_hi)`` of the filters that are non-zero at
    every bin; (0, 0) where there is none."""
    nz = np.asarray(fb) != 0
    F, M = nz.shape

    def hulls(a):                      # a: (rows, n) bool -> (rows, 2)
        any_ = a.any(axis=1)
        lo = np.where(any_, a.argmax(axis=1), 0)
        hi = np.where(any_, a.shape[1] - a[:, ::-1].argmax(axis=1), 0)
        return np.stack([lo, hi], axis=1).astype(np.int32)

    return hulls(nz.T), hulls(nz)
