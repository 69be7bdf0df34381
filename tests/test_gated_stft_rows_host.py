"""``TorchGate.gated_stft(x, lengths=...)`` without a GPU: the public surface, the validation that runs before any device
work, the routing that can be seen from a CPU tensor, the conditions every input of tests/gated_stft_rows_cases.py has
to meet on the oracle alone, and -- in numpy -- that the metrics of tests/test_gpu_gated_stft_rows.py pass the contract's
own model and flag a planted defect in exactly the rows and frames it touches."""
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import spectralgate_oracle as O
from tests import gated_stft_cases as C
from tests import gated_stft_rows_cases as R
from tests import parity_budget as PB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tg(**kw):
    from noisereduce_amd.torchgate import TorchGate
    return TorchGate(sr=R.SR, **kw)


# ---- 1. the surface ----------------------------------------------------------------------------------------------------
def test_signature_and_stft_lengths():
    from noisereduce_amd.torchgate import TorchGate
    names = list(inspect.signature(TorchGate.gated_stft).parameters)
    assert names == ["self", "x", "xn", "return_mask", "lengths", "xn_lengths"], names
    p = inspect.signature(TorchGate.gated_stft).parameters
    assert p["lengths"].default is None and p["xn_lengths"].default is None and p["return_mask"].default is False
    tg = _tg(n_fft=512, win_length=400, hop_length=90)
    got = tg.stft_lengths([800, 899, 900, 901])
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == [9, 10, 11, 11]
    got = tg.stft_lengths(np.array([800, 5000], dtype=np.int32))
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == [1 + 800 // 90, 1 + 5000 // 90]
    t = tg.stft_lengths(torch.tensor([800, 901], dtype=torch.int32))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.device.type == "cpu" and t.tolist() == [9, 11]
    for c in R.CELLS:
        assert _tg(**R.gate_kwargs(c)).stft_lengths(c["lens"]).tolist() == R.frames_of(c)


def test_header_library_and_bindings_agree():
    from noisereduce_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    for name, nargs in (("sg_gate_spectrum_rows", 15), ("sg_gate_spectrum_rows_backward", 10)):
        assert "SG_API int %s(" % name in hdr
        assert name in _ffi.exported_symbols() and len(_ffi._PROTOTYPES[name][1]) == nargs
    assert callable(getattr(_ffi.Gate, "gate_spectrum_rows", None))
    assert callable(getattr(_ffi.Gate, "gate_spectrum_rows_backward", None))
    assert list(inspect.signature(_ffi.Gate.gate_spectrum_rows).parameters) == ["self", "x", "lengths", "xn", "xn_lengths",
                                                                                 "save_mask"]
    assert list(inspect.signature(_ffi.Gate.gate_spectrum_rows_backward).parameters) == ["self", "grad", "mask", "L", "lengths"]


# ---- 2. / 3. validation and routing, on CPU tensors ----------------------------------------------------------------------
def test_validation_errors_come_before_any_device_work():
    tg = _tg()
    x = torch.zeros((3, 8000))
    with pytest.raises(ValueError, match=r"lengths\[1\] = 2047"):
        tg.gated_stft(x, lengths=[8000, 2047, 4000])
    with pytest.raises(ValueError, match=r"lengths\[2\] = 8001"):
        tg.gated_stft(x, lengths=[8000, 4000, 8001])
    with pytest.raises(ValueError, match="must be integers"):
        tg.gated_stft(x, lengths=[8000.0, 4000.5, 4000.0])
    with pytest.raises(ValueError, match="must hold 3 integers"):
        tg.gated_stft(x, lengths=[8000, 4000])
    with pytest.raises(ValueError, match="xn_lengths given without xn"):
        tg.gated_stft(x, lengths=[8000, 4000, 4000], xn_lengths=[3000])
    with pytest.raises(ValueError, match=r"xn rows \(2\) must be 1 or the batch size"):
        tg.gated_stft(x, torch.zeros((2, 5000)), lengths=[8000, 4000, 4000], xn_lengths=[3000, 3000])
    with pytest.raises(ValueError, match=r"xn rows \(2\) must be 1 or the batch size"):
        tg.gated_stft(x, torch.zeros((2, 5000)), lengths=[8000, 4000, 4000])
    with pytest.raises(ValueError, match=r"xn_lengths\[0\] = 100"):
        tg.gated_stft(x, x[:1], lengths=[8000, 4000, 4000], xn_lengths=[100])
    # the same calls through forward raise the same errors
    with pytest.raises(ValueError, match=r"lengths\[1\] = 2047"):
        tg(x, lengths=[8000, 2047, 4000])
    with pytest.raises(ValueError, match="xn_lengths given without xn"):
        tg(x, lengths=[8000, 4000, 4000], xn_lengths=[3000])


@pytest.mark.parametrize("kw", [dict(), dict(nonstationary=True), dict(n_fft=400)])
def test_valid_lengths_on_a_cpu_tensor_reach_the_no_fallback_error(kw):
    tg = _tg(**kw)
    x = torch.zeros((3, 8000))
    for lengths in ([8000] * 3, torch.full((3,), 8000), [8000, 4000, 2 * tg.win_length]):
        with pytest.raises(RuntimeError, match="GPU only"):
            tg.gated_stft(x, lengths=lengths)
    with pytest.raises(RuntimeError, match="GPU only"):
        tg.gated_stft(x, x[:1, :5000], lengths=[8000] * 3, xn_lengths=[5000], return_mask=True)


# ---- 4. the inputs' conditions, on the oracle alone ----------------------------------------------------------------------
def test_cells_cover_the_tile_edges():
    names = [c["name"] for c in R.CELLS]
    assert len(set(names)) == len(names) == 11
    assert [c["n_fft"] for c in R.E_CELLS] == list(R.NATIVE)
    for c in R.E_CELLS:
        assert (c["W"], c["H"]) == (c["n_fft"], c["n_fft"] // 4) and c["seed"] == c["n_fft"] + c["H"]
        assert R.frames_of(c) == [R.FPT + 1, R.FPT + 1, R.RPT, R.RPT + 1, R.RPT + 2, 3 * R.FPT + 1]
    assert {(c["n_fft"], c["W"], c["H"]) for c in R.G_CELLS} == {(256, 200, 37), (512, 400, 100), (1024, 1000, 333),
                                                                 (2048, 1500, 333), (4096, 3000, 700), (4096, 4096, 2048)}
    for c in R.CELLS:
        assert c["L"] == c["lens"][-1] == max(c["lens"]) and min(c["lens"]) == 2 * c["W"]
        assert R.frames_of(c)[-1] == 1 + c["L"] // c["H"] == 25
        assert sum(n < c["L"] for n in c["lens"]) == 5
    src = open(os.path.join(ROOT, "noisereduce_amd", "csrc", "rows.hip")).read()
    assert "constexpr int FPT = 8;" in src and "constexpr int RPT = 16;" in src


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("gate", R.GATES)
@pytest.mark.parametrize("c", R.CELLS, ids=R.cell_id)
def test_input_conditions(c, gate, dtype):
    for i, u in enumerate(R.units(c, gate, dtype)):
        cfg = u["cfg"]
        assert cfg["prop"] == R.PROP and cfg["filt"] is not None and cfg["stationary"] == (gate == "stat")
        assert u["Z"].shape == (c["n_fft"] // 2 + 1, R.frames_of(c)[i])
        frac = float(np.mean(u["raw"] > 0.5))
        assert 0.01 <= frac <= 0.99, (c["name"], gate, i, frac)
        if gate == "stat":
            margin = PB.nearest_margin_db(u)
            left = float(np.mean(np.abs(u["db"] - u["thresh"][:, None]) <= PB.DELTA_DB))
            assert left <= PB.LEFT_OUT_CAP, (c["name"], i, left)
            assert margin > PB.DELTA_DB, (c["name"], i, margin)     # nothing is left out: mask_diff may compare every cell
        # prop_decrease = 0.5 and zero padding beyond the field: a cell keeps at least half the filter's weight that lies
        # inside the row's own field (tests/test_gated_stft_budget_host.py) -- no cell of the mask is anywhere near 0
        inside = O.conv2_same_direct(np.ones(u["mask"].shape), cfg["filt"])
        assert np.all(u["mask"] >= R.PROP * inside - 1e-12) and u["mask"].min() >= 0.05, (c["name"], i, u["mask"].min())


# ---- 5. the metrics: the contract's model passes, a planted defect is flagged where it is ----------------------------------
def _spectrum_bad(c, us, Y, M):
    """row -> frames of its own [0, T_i) flagged by spectrum_check; the frames after them must be exactly zero."""
    out = {}
    for i, u in enumerate(us):
        Ti = u["Z"].shape[1]
        assert not Y[i, :, Ti:].any() and not M[i, :, Ti:].any()
        bad, _ = C.spectrum_check(Y[i, :, :Ti], u["Z"], M[i, :, :Ti], u["cfg"], emu=u["emu_spec"])
        out[i] = bad.tolist()
    return out


def _mask_bad(us, M):
    out = {}
    for i, u in enumerate(us):
        Ti = u["Z"].shape[1]
        cells, _ = PB.mask_diff(M[i, :, :Ti], u, bound=PB.mask_bound(u["cfg"], integer_taps=False))
        out[i] = sorted(set(cells[:, 1].tolist()))
    return out


@pytest.mark.parametrize("c", R.E_CELLS, ids=R.cell_id)
def test_planted_forward_defects_are_flagged_where_they_are(c):
    us = R.units(c, "stat", "float32")
    short = [i for i, n in enumerate(c["lens"]) if n < c["L"]]
    full = [i for i, n in enumerate(c["lens"]) if n == c["L"]]
    assert short and full
    for out_dtype in R.DTYPES:
        Y, M = R.model_forward(c, us, out_dtype)
        assert all(v == [] for v in _spectrum_bad(c, us, Y, M).values())
        assert all(v == [] for v in _mask_bad(us, M).values())
    # complex128: the float64 bar itself
    Y, M = R.model_forward(c, us, "float64")
    for i, u in enumerate(us):
        Ti = u["Z"].shape[1]
        assert np.abs(Y[i, :, :Ti] - u["Z"] * M[i, :, :Ti].astype(np.float64)).max() <= PB.F64_REL * np.abs(u["Z"]).max()

    # statistics over the padded row: the transform is right, the mask is not, in every short row and in no full one
    Y, M = R.model_forward(c, us, "float32", defect="stats_padded")
    assert all(v == [] for v in _spectrum_bad(c, us, Y, M).values())
    mb = _mask_bad(us, M)
    assert all(mb[i] for i in short) and all(mb[i] == [] for i in full), mb

    # frame T_i - 1 transformed from the padding: that frame of every short row, nothing else
    xp = R.rows(c, "float32", pad=0.5).double().numpy()
    Y, M = R.model_forward(c, us, "float32", defect="last_frame", x_pad=xp)
    sb = _spectrum_bad(c, us, Y, M)
    for i in short:
        assert sb[i] == [R.frames_of(c)[i] - 1], (i, sb[i])
    assert all(sb[i] == [] for i in full) and all(v == [] for v in _mask_bad(us, M).values())

    # smoothing that sees 1 - p beyond T_i: the last n_grad_time frames of every short row, nothing else
    Y, M = R.model_forward(c, us, "float32", defect="smooth_1mp")
    assert all(v == [] for v in _spectrum_bad(c, us, Y, M).values())
    mb = _mask_bad(us, M)
    nt = us[0]["cfg"]["nt"]
    for i in short:
        Ti = R.frames_of(c)[i]
        assert mb[i] == list(range(max(0, Ti - nt), Ti)), (i, mb[i], Ti, nt)
    assert all(mb[i] == [] for i in full)


@pytest.mark.parametrize("c", R.E_CELLS, ids=R.cell_id)
def test_planted_backward_defect_is_flagged_where_it_is(c):
    us = R.units(c, "stat", "float32")
    _, M = R.model_forward(c, us, "float32")
    G = R.grad_fields(c, "float32")["dense"]
    F = M.shape[1]
    for defect in (None, "leak"):
        gx = R.model_backward(c, np.nan_to_num(G), M, defect=defect)
        assert np.isfinite(gx).all()
        for i, n in enumerate(c["lens"]):
            Ti = R.frames_of(c)[i]
            bad, _ = C.spec_adjoint_check(gx[i, :n].astype(np.float32), G[i, :, :Ti], M[i, :, :Ti], us[i]["cfg"], n)
            assert len(bad) == 0, (c["name"], i, bad)
            tail_zero = not gx[i, n:].any()
            assert tail_zero == (defect is None or n == c["L"]), (c["name"], defect, i)
    # the single-cell gradients: the imaginary part at bins 0 and n/2 leaves no trace in the model either
    for name in ("last_dc", "last_nyquist"):
        g = np.nan_to_num(R.grad_fields(c, "float64")[name])
        a = R.model_backward(c, g, M)
        b = R.model_backward(c, g.real.astype(np.complex128), M)
        assert a.any() and np.abs(a - b).max() <= PB.F64_REL * np.abs(a).max()
    assert F == c["n_fft"] // 2 + 1
