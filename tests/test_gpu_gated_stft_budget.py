"""TorchGate.gated_stft on the GPU (csrc/spec.hip; process_batch_impl with a spectrum to write, csrc/api.hip) held to the
float64 oracle frame by frame and hop block by hop block, on every route and edge (tests/gated_stft_cases.py):

* ``E-*`` / ``G-*``  rows of Q - 1, Q, Q + 1 and 2 Q + 1 frames for the Q frames a workgroup of k_spec_fwd / k_spec_bwd
                 handles, and windows and hops off win = n_fft, hop = n_fft / 4: every frame by ``spectrum_check``;
* adjoint cells  sg_gate_spectrum_backward by ``spec_adjoint_check`` on a dense gradient and on six single cells, under a
                 mask whose padding columns hold NaN;
* ``R-*``        every branch of the routing, asserted from ``Gate.spectrum_route()`` (sg_debug_counter 18) and
                 ``Gate.smooth_route()`` against the predicates restated in ``spec_route_label``; the mask as
                 tests/stagewise_checks.py holds forward's, and bitwise the SG_OPT_FORCE_NOFAST mask of process_batch.

tests/test_gated_stft_budget_host.py holds the inputs' conditions and that the metrics flag planted defects.  No tolerance
is defined here: FACTOR, POOL, EPS32, DELTA_DB, LEFT_OUT_CAP are tests/parity_budget.py's, MASK_TOL is
tests/test_gpu_gated_stft.py's.  The figures per cell go to the file named by PARITY_BUDGET_OUT, if set
(profiles/parity_budget_gated_stft.json is that file from an MI355X run of this module alone)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import gated_stft_cases as C
from tests import parity_budget as PB
from tests import stagewise_checks as SC
from tests.test_gpu_gated_stft import MASK_TOL

pytestmark = pytest.mark.gpu

_RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_record():
    yield
    path = os.environ.get("PARITY_BUDGET_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "cells": dict(sorted(_RECORD.items()))}, f, indent=1)


def _note(name, **kw):
    rec = _RECORD.setdefault(name, {})
    for k, v in kw.items():
        rec[k] = max(rec.get(k, 0.0), float(v)) if isinstance(v, float) else v


def _torch_dtype(name):
    return torch.float32 if name == "float32" else torch.float64


def _check_spectrum_rows(tag, Y, mask, units):
    """Every row, every frame; returns (largest err / bud, the masks as (F, T) float32 arrays)."""
    Y, mask = Y.cpu().numpy(), mask.cpu().numpy()
    worst, Ms = 0.0, []
    for b, u in enumerate(units):
        assert np.isfinite(mask[b]).all() and np.isfinite(Y[b].real).all() and np.isfinite(Y[b].imag).all(), (tag, b)
        bad, ratio = C.spectrum_check(Y[b], u["Z"], mask[b], u["cfg"], x=u["x"], emu=u.get("emu_spec"))
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s row %d: frames %s of %d over their bound (largest error / budget in the row %.2f)" % (
            tag, b, bad[:12].tolist(), Y.shape[2], ratio)
        Ms.append(mask[b])
    return worst, Ms


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("cell", C.EG_CELLS, ids=C.eg_cell_id)
def test_edge_and_geometry_cell(cell, dtype):
    from noisereduce_amd.torchgate import TorchGate
    units = C.eg_units(cell, dtype)
    tg = TorchGate(sr=cell["sr"], **C.eg_kwargs(cell)).cuda()
    x = torch.from_numpy(C.eg_x(cell, np.dtype(dtype))).cuda()
    Y, mask = tg.gated_stft(x, return_mask=True)
    gate = tg._gate_for(x.device)
    assert tuple(Y.shape) == (C.EG_B, cell["n_fft"] // 2 + 1, cell["T"])
    assert Y.dtype == (torch.complex64 if dtype == "float32" else torch.complex128)
    spec, smooth = C.spec_route_label(units[0]["cfg"], cell["T"])
    assert gate.spectrum_route() == spec + (1,) and gate.smooth_route() == smooth, (gate.spectrum_route(), gate.smooth_route())
    tag = "%s %s" % (cell["name"], dtype)
    worst, Ms = _check_spectrum_rows(tag, Y, mask, units)
    mask_err = 0.0
    for b, (u, M) in enumerate(zip(units, Ms)):
        # (prop_decrease = 0.5: the float kernels' bound, parity_budget.mask_bound)
        cells, w = PB.mask_diff(M, u, bound=PB.mask_bound(u["cfg"], integer_taps=False))
        mask_err = max(mask_err, w)
        assert len(cells) == 0, "%s row %d: mask off by up to %.3g at %d cells, first %s" % (tag, b, w, len(cells), cells[:6].tolist())
    print("[gated_stft budget] %s: largest spectrum err / bud %.2f, mask err %.3g" % (tag, worst, mask_err))
    _note(cell["name"], **{"spectrum_" + dtype: worst, "mask_err_" + dtype: mask_err, "spectrum_route": list(spec),
                           "smooth_route": list(smooth)})


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("cell", C.ADJ_CELLS, ids=C.eg_cell_id)
def test_adjoint_cell(cell, dtype):
    from noisereduce_amd.torchgate import TorchGate
    tg = TorchGate(sr=cell["sr"], **C.eg_kwargs(cell)).cuda()
    gate = tg._gate_for(torch.device("cuda", torch.cuda.current_device()))
    G, M = C.adj_inputs(cell, np.dtype(dtype))
    L, F = cell["L"], cell["n_fft"] // 2 + 1
    pairs = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(G.transpose(0, 2, 1)))).cuda()      # (B, T, F, 2)
    assert pairs.dtype == _torch_dtype(dtype)
    gx = gate.gate_spectrum_backward(pairs, torch.from_numpy(M).cuda(), L)
    assert gx.shape == (2, L) and gx.dtype == _torch_dtype(dtype)
    gx = gx.cpu().numpy()
    assert np.isfinite(gx).all(), "%s: the NaN of the mask's padding columns reached the gradient" % cell["name"]
    cfg = C.eg_units(cell, "float32")[0]["cfg"]
    worst = 0.0
    for b in range(2):
        u = C.spec_adjoint_unit(G[b], M[b, :, :F].T, cfg, L)
        bad, ratio = C.spec_adjoint_check(gx[b], G[b], M[b, :, :F].T, cfg, L, unit=u)
        worst = max(worst, ratio)
        if len(bad):
            err = PB.local_error(gx[b], u["want"], cfg["H"])
            raise AssertionError("%s %s row %d: hop blocks %s of %d over their bound: error %s, budget %s, largest error / "
                                 "budget %.2f" % (cell["name"], dtype, b, bad[:10].tolist(), len(err), err[bad[:10]],
                                                  u["bud"][bad[:10]], ratio))
    print("[gated_stft budget] %s %s: largest adjoint err / bud %.2f" % (cell["name"], dtype, worst))
    _note(cell["name"], **{"adjoint_" + dtype: worst})


def _mask_tol(cfg):
    """sg_gate_spectrum smooths a float 0 / 1 field with float taps at every width, so a stationary mask is held as
    tests/stagewise_checks.py holds the materialised route's: ``PB.mask_bound(integer_taps=False)``, (2 nf + 2 nt + 7)
    roundings of a sum of weights 1.  MASK_TOL (two float32 ulps at 1.0) is tests/test_gpu_gated_stft.py's figure for the
    filter TorchGate builds by default at 16 kHz, (16, 3): a cell with those widths keeps it.  It cannot hold at every
    width -- a float32 sum of 5 x 163 products is not within 4 roundings of the exact one: (2, 81) measures 3.7e-7."""
    if cfg["filt"] is None or (cfg["nf"], cfg["nt"]) == (16, 3):
        return MASK_TOL
    return PB.mask_bound(cfg, integer_taps=False)


# one cell per decide branch also runs without a mask buffer (smoothing into the engine's own field)
_NO_MASK_CELLS = {"R-t128", "R-t129", "R-1024-800-200", "R-tw-TNS-f2-t12", "R-tw-TNS-f2-t13"}


@pytest.mark.parametrize("cell", C.R_CELLS, ids=C.r_cell_id)
def test_route_cell(cell):
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    case, units = C.r_case(cell), C.r_units(cell)
    name = cell["name"]
    tg = TorchGate(sr=case["sr"], **case["kw"]).cuda()
    x = torch.from_numpy(case["x"]).cuda()
    xn = None if case["xn"] is None else torch.from_numpy(case["xn"]).cuda()
    gate = tg._gate_for(x.device)
    cfg = units[0]["cfg"]
    F, T = units[0]["mask"].shape
    kbox = case["kw"].get("n_movemean_nonstationary", 20)
    spec, smooth = C.spec_route_label(cfg, T, kbox=kbox)
    with gate.lock:
        Y, mask = tg.gated_stft(x, xn, return_mask=True)
        got_spec, got_smooth = gate.spectrum_route(), gate.smooth_route()
        assert got_spec == spec + (1,), "%s: routed %s, labelled %s" % (name, got_spec, spec + (1,))
        assert got_smooth == smooth, "%s: smoothed by %s, labelled %s" % (name, got_smooth, smooth)
        bits = None
        if cfg["stationary"]:
            bits = SC.fetch(gate, 3)
            if bits is None:
                raw = SC.fetch(gate, 0)
                assert raw is not None, "%s: neither the bit field nor the raw mask can be fetched" % name
                bits = raw > 0.5
        # bitwise the mask of forward's general route.  Stationary: SG_OPT_FORCE_NOFAST, which keeps forward off the integer
        # smoothing and decides in float64 either way.  Non-stationary: forward as it stands -- the option would swap the
        # float32 magnitude transform under the sigmoid (k_mag_fast for stft_any<float>, stage_mag), which moves the mask by
        # an ulp (R-tw-TNS-f2-t12 measured 6.3e-8 against the option's mask), and sg_gate_spectrum runs forward's kernels.
        with gate.with_options([(_ffi.SG_OPT_FORCE_NOFAST, 1)] if cfg["stationary"] else []):
            _, m2 = gate.process_batch(x, xn, save_mask=True)
        assert torch.equal(m2[:, :, :F], mask.transpose(1, 2)), \
            "%s: max diff to forward's mask %.3e" % (name, float((m2[:, :, :F] - mask.transpose(1, 2)).abs().max()))
        if name in _NO_MASK_CELLS:
            pairs = gate.gate_spectrum(x, xn)
            s2 = gate.spectrum_route()
            assert s2 == C.spec_route_label(cfg, T, kbox=kbox, with_mask=False)[0] + (1,) and not s2[2], (name, s2)
            assert torch.equal(pairs, torch.view_as_real(Y.transpose(1, 2).contiguous())), \
                "%s: the spectrum of the call without a mask buffer differs" % name
    worst, Ms = _check_spectrum_rows(name, Y, mask, units)
    mask_err = 0.0
    for b, (u, M) in enumerate(zip(units, Ms)):
        if cfg["stationary"]:
            cells, left = PB.bit_diff(bits[b], u)
            assert left <= PB.LEFT_OUT_CAP
            assert len(cells) == 0, "%s row %d: %d decision bits differ from the oracle, first (band, frame) %s" % (
                name, b, len(cells), cells[:6].tolist())
            cells, w = PB.mask_diff(M, u, bound=_mask_tol(u["cfg"]))
            print("[gated_stft budget] %s row %d: mask err %.3g" % (name, b, w))
            assert len(cells) == 0, "%s row %d: mask off by up to %.3g at %d cells, first %s" % (name, b, w, len(cells), cells[:6].tolist())
            mask_err = max(mask_err, w)
        else:
            emu = PB.emulate_stages_f32(u)
            PB._field_rule(M, u["mask"], emu[2], "%s row %d final mask" % (name, b))
            mask_err = max(mask_err, float(np.abs(M.astype(np.float64) - u["mask"]).max()))
    print("[gated_stft budget] %s: largest spectrum err / bud %.2f, mask err %.3g, route %s %s" % (name, worst, mask_err, got_spec, got_smooth))
    _note(name, spectrum_float32=worst, mask_err_float32=mask_err, spectrum_route=list(got_spec), smooth_route=list(got_smooth))


def test_route_counter_counts_sub_batches_and_forgets_a_failed_call():
    """Bits 16.. of sg_debug_counter 18, and its 0 after a call that failed before any spectrum launch."""
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    cell = next(c for c in C.R_CELLS if c["name"] == "R-t128")
    case, units = C.r_case(cell), C.r_units(cell)
    tg = TorchGate(sr=case["sr"], **case["kw"]).cuda()
    x = torch.from_numpy(case["x"]).cuda()
    label = C.spec_route_label(units[0]["cfg"], units[0]["mask"].shape[1])[0]
    whole = tg._gate_for(x.device)
    small = _ffi.Gate("cuda", **PB.torchgate_gate_kwargs(tg, max_workspace_bytes=1 << 10))
    try:
        assert small.spectrum_route() == ("none", False, False, 0)           # no call yet
        Y1, m1 = small.gate_spectrum(x, save_mask=True)
        assert small.spectrum_route() == label + (x.shape[0],), small.spectrum_route()      # a row per sub-batch
        Y0, m0 = whole.gate_spectrum(x, save_mask=True)
        assert whole.spectrum_route() == label + (1,)
        assert torch.equal(Y0, Y1) and torch.equal(m0[:, :, :513], m1[:, :, :513])
        with pytest.raises(ValueError, match="x must be bigger than 2048"):
            small.gate_spectrum(x[:, :2047].contiguous())
        assert small.spectrum_route() == ("none", False, False, 0)
        small.process_batch(x)                                               # forward leaves the counter alone
        assert small.spectrum_route() == ("none", False, False, 0) and whole.spectrum_route() == label + (1,)
    finally:
        small.close()
