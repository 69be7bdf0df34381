"""TorchGate.gated_stft without a GPU: the surface (method, headers, prototypes, exported symbols), the float64 model (the
gated spectrogram is what the oracle inverts; the adjoint formula of DESIGN section 14 is an adjoint), the conditions every
stationary input of tests/test_gpu_gated_stft.py has to meet for "same mask as the oracle" to be a fair demand, and the
Python-level validation that runs before any device work."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import spectralgate_oracle as O
from tests import gated_stft_cases as C

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = {"sg_gate_spectrum", "sg_gate_spectrum_backward"}
STATIONARY_RUNS = [(c, v) for c, v in C.RUNS if v != "nonstat"]


def test_surface():
    import __graft_entry__
    __graft_entry__.build()
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    assert callable(getattr(TorchGate, "gated_stft", None))
    declared = set()
    for name in ("mi355gate.h", "mi355gate_debug.h"):
        declared |= set(re.findall(r"\b(sg_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", name)).read()))
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= set(_ffi._PROTOTYPES)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.strip()}
    assert NEW_SYMBOLS <= exported
    assert callable(getattr(_ffi.Gate, "gate_spectrum", None)) and callable(getattr(_ffi.Gate, "gate_spectrum_backward", None))


@pytest.mark.parametrize("case,variant", [("a", "plain"), ("b", "xnB"), ("c", "nosmooth"), ("a", "nonstat")])
def test_model_gated_spectrogram_is_what_the_oracle_inverts(case, variant):
    y, st = C.oracle(case, variant, "float64")
    n, W, H = C.geometry(case)
    again = O.istft_torch(st["X"] * st["mask"], n, W, H, C.window64(case))
    assert again.shape == y.shape
    assert np.array_equal(again, y)


@pytest.mark.parametrize("n,W,H", [(1024, 1024, 256), (512, 400, 100), (256, 256, 64)])
def test_model_adjoint_identity(n, W, H):
    """<STFT(x) * m, g> == <x, adjoint(g)> for the real inner product, to 1e-12 relative; and the half-size merge the kernel
    takes (bins 0 and n/2 doubled and made real, N * irfft) is the same frame as the weight-1 sum."""
    rng = np.random.default_rng(n + H)
    L = 2 * W + 77
    x = rng.standard_normal((2, L))
    w = torch.hann_window(W).double().numpy()
    X = O.stft_torch(x, n, W, H, w)
    m = rng.random(X.shape)
    g = rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)
    Y = X * m
    lhs = np.sum(Y.real * g.real + Y.imag * g.imag)
    rhs = np.sum(x * C.adjoint_np(g, m, n, W, H, L, w))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    full = np.zeros((2, n, X.shape[2]), dtype=np.complex128)
    full[:, :n // 2 + 1] = m * g
    direct = np.real(np.fft.ifft(full, axis=1)) * n
    assert np.abs(direct - C.merge_model(g, m, n)).max() <= 1e-12 * np.abs(direct).max()


@pytest.mark.parametrize("case,variant", STATIONARY_RUNS, ids=[f"{c}-{v}" for c, v in STATIONARY_RUNS])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_input_conditions_of_the_stationary_gpu_cases(case, variant, dtype):
    """Between 5 % and 95 % of the cells pass the gate (overall and in every row), and no cell's dB value lies within
    1e-6 dB of its threshold: no decision can hinge on float rounding."""
    _, st = C.oracle(case, variant, dtype)
    X_db = O.amp_to_db(st["X"], 40.0)
    thresh = st["thresh"]
    if thresh.shape[0] == 1:
        thresh = np.broadcast_to(thresh, X_db.shape[:2])
    assert np.array_equal(st["raw"], (X_db > thresh[:, :, None]).astype(np.float64))
    frac = st["raw"].mean()
    rows = st["raw"].mean(axis=(1, 2))
    assert 0.05 <= frac <= 0.95, frac
    assert 0.05 <= rows.min() and rows.max() <= 0.95, (rows.min(), rows.max())
    margin = np.abs(X_db - thresh[:, :, None]).min()
    assert margin > 1e-6, margin


def test_every_variant_is_exercised_at_case_a_and_off_1024():
    for v in C.VARIANTS:
        assert ("a", v) in C.RUNS
        assert any(c != "a" and C.CASES[c]["n_fft"] != 1024 and vv == v for c, vv in C.RUNS), v


def test_python_validation_needs_no_device():
    from noisereduce_amd.torchgate import TorchGate
    tg = TorchGate(sr=16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tg.gated_stft(torch.zeros(2, 4096))
    with pytest.raises(Exception, match="x must be bigger than 2048"):
        tg.gated_stft(torch.zeros(2, 2047))
    with pytest.raises(Exception, match="xn must be bigger than 2048"):
        tg.gated_stft(torch.zeros(2, 4096), torch.zeros(100))
    # (a short row on the device is refused before any device work too: the check precedes the device test)
    with pytest.raises(Exception, match="x must be bigger than 800"):
        TorchGate(sr=16000, n_fft=512, win_length=400, hop_length=100).gated_stft(torch.zeros(1, 799))
