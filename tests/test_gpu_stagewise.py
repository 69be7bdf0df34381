"""Every gate path against the float64 oracle stage by stage and hop block by hop block (tests/parity_budget.py).

One matrix (parity_budget.CELLS: kernel family x column settings), three checks per cell:

a. decision bits (stationary): the kernel's bits inside ``debug_range()`` equal the oracle's ``raw`` of the same unit --
   every unit, every channel, all F bands; no differing cell outside the 1e-8 dB ambiguity margin, at most 1e-5 of a
   unit's cells inside it;
b. the smoothed mask, whole field incl. bands 0 and F - 1 and the first / last column, wherever a float mask exists
   (``debug_field(1)``; the non-stationary raw sigmoid through ``debug_field(0)``); which fields a route must keep
   follows from the kernels it launched, and each route must launch the kernels its cell is labelled with;
c. the output of every unit, per hop block of the kept range, within FACTOR x the float32 emulation's error there
   (``precision="float64"`` cells: 1e-12 of the block's own peak) -- for the default route and every forced route.

Then (a) / (c) for TorchGate.forward: row gate, four-kernel path, ``lengths=`` rows (those: the final mask the call
hands back, against the oracle's).

The largest local_error / budget per family and route goes to the file named by PARITY_BUDGET_OUT, if set
(profiles/parity_budget.json is that file from an MI355X run)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import parity_budget as PB
from tests import stagewise_checks as SC
from tests.stagewise_checks import (check_bits as _check_bits, check_stationary_mask as _check_stationary_mask,  # noqa: F401
                                    fetch as _fetch, make_sg as _make_sg, note, stages_of as _stages)  # (other GPU tests import these names)

pytestmark = pytest.mark.gpu

_RATIOS = SC.RATIOS          # (the checks themselves live in tests/stagewise_checks.py, shared with the width matrix)


def _note(family, route, ratio):
    note(family, route, ratio)


@pytest.fixture(scope="module", autouse=True)
def _dump_ratios():
    yield
    path = os.environ.get("PARITY_BUDGET_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "largest_local_error_over_budget": dict(sorted(_RATIOS.items()))},
                      f, indent=1)


def _routes(cell, case):
    from noisereduce_amd import _ffi
    routes = [("default", [])]
    if case["precision"] == "float64":
        return routes
    if cell["family"] == "register":
        routes.append(("force_split", [(_ffi.SG_OPT_FORCE_SPLIT, 1)]))
    routes.append(("force_nofast", [(_ffi.SG_OPT_FORCE_NOFAST, 1)]))
    routes.append(("force_unfused", [(_ffi.SG_OPT_FORCE_UNFUSED, 1)]))
    return routes


def _assert_route(cell, case, route, stages):
    """A cell must run the kernels its label claims (a shape that quietly routes elsewhere fails here)."""
    fam, stat = PB.kernel_family(cell), case["kw"]["stationary"]
    tag = "%s [%s]: launched %s" % (PB.cell_id(cell), route, sorted(stages))
    if case["precision"] == "float64":
        return
    register_only = {"k_gate_onepass", "k_decide_fast", "k_apply_fast"}
    if fam != "register":
        assert not (stages & register_only) and "k_apply_istft" in stages, tag
    if route == "force_unfused":
        assert ("k_decide" in stages and "k_stft<double>" in stages) if stat else "k_box_mask" in stages, tag
        return
    if not stat:
        assert "k_iir_mask<nt>" in stages, tag
        if fam == "register":
            assert ("k_apply_istft" if route == "force_nofast" else "k_apply_fast") in stages, tag
        return
    if fam == "register":
        if route == "default":
            assert "k_gate_onepass" in stages, tag
        elif route == "force_split":
            assert "k_decide_fast" in stages and "k_apply_fast" in stages and "k_gate_onepass" not in stages, tag
        else:
            assert "k_stft_bits<decide>" in stages and "k_apply_istft" in stages, tag
    elif fam == "mixed_radix":   # the fused bit-mask route exists for mixed radix, not for chirp-z
        assert ("k_stft_bits<decide>" in stages) == (route != "no_mixed_radix"), tag
    elif fam in ("chirp_z", "four_step"):
        assert "k_decide" in stages and "k_stft<double>" in stages, tag


def _run_cell(cell, case, out, units, sg, routes):
    """Every route of a cell: the route itself, then checks c, a, b (tests/stagewise_checks.py)."""
    SC.run_cell(PB.cell_id(cell), PB.kernel_family(cell), case, out, units, sg, routes,
                lambda name, stages, gate: _assert_route(cell, case, name, stages))


@pytest.mark.parametrize("cell", PB.CELLS, ids=PB.cell_id)
def test_cell(cell):
    case = PB.cell_case(cell)
    out, units = PB.cell_oracle(cell)
    _run_cell(cell, case, out, units, _make_sg(case), _routes(cell, case))


@pytest.mark.parametrize("cell", [c for c in PB.CELLS if c["family"] == "mixed_radix" and c.get("precision") != "float64"],
                         ids=PB.cell_id)
def test_cell_on_the_chirp_z_route(cell, monkeypatch):
    """The mixed-radix sizes once more with SG_NO_MIXED_RADIX=1 at handle creation (chirp-z kernels)."""
    from noisereduce_amd import _ffi
    case = PB.cell_case(cell)
    out, units = PB.cell_oracle(cell)
    monkeypatch.setenv("SG_NO_MIXED_RADIX", "1")
    _ffi.clear_gate_cache()
    try:
        sg = _make_sg(case)
        _run_cell(cell, case, out, units, sg, [("no_mixed_radix", [])])
        del sg
    finally:
        monkeypatch.delenv("SG_NO_MIXED_RADIX")
        _ffi.clear_gate_cache()


# ---- TorchGate.forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PB.T_CELLS)), ids=[PB.t_cell_id(c) for c in PB.T_CELLS])
def test_torchgate_cell(i):
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    case = PB.t_case(i)
    cell, kw = case["cell"], case["kw"]
    n_fft = kw["n_fft"]
    H = n_fft // 4
    window = torch.hann_window(n_fft).double().numpy()
    tg = TorchGate(sr=PB.T_SR, **kw).cuda()
    x = torch.from_numpy(case["x"]).cuda()
    xn = None if case["xn"] is None else torch.from_numpy(case["xn"]).cuda()
    xn64 = None if case["xn"] is None else case["xn"].astype(np.float64)
    lengths = case["lengths"]
    B, L = case["x"].shape
    gate = tg._gate_for(x.device)
    mask = None
    if lengths is None:
        got = tg(x, xn).cpu().numpy()
        _, units = PB.torchgate_units(case["x"].astype(np.float64), PB.T_SR, xn=xn64, window=window, **kw)
    else:
        got = tg(x, xn, lengths=lengths).cpu().numpy()
        if n_fft & (n_fft - 1) == 0:      # the table-driven kernels hand back their final mask (other sizes: one call per row)
            with gate.lock:
                got2, mask = gate.process_rows(x, lengths, xn, None, save_mask=True)
            assert np.array_equal(got2.cpu().numpy(), got)
            mask = mask.cpu().numpy()
        units = []
        for b in range(B):
            _, ub = PB.torchgate_units(case["x"][b:b + 1, :int(lengths[b])].astype(np.float64), PB.T_SR, xn=xn64,
                                       window=window, **kw)
            units.append(ub[0])
    tag = PB.t_cell_id(cell)
    worst = 0.0
    for b, u in enumerate(units):
        n = len(u["want"])
        bad, ratio = PB.local_check(got[b, :n], u)
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s row %d: hop blocks %s over their bound (largest error / budget %.2f)" % (tag, b, bad[:10].tolist(), ratio)
        assert np.all(got[b, n:] == 0)
        if mask is not None and u["cfg"]["stationary"]:
            T = u["mask"].shape[1]
            cells, w = PB.mask_diff(mask[b, :T, :n_fft // 2 + 1].T, u)
            assert len(cells) == 0, "%s row %d: final mask off by up to %.3g at %d cells, first %s" % (tag, b, w, len(cells), cells[:6].tolist())
            assert np.all(mask[b, T:, :n_fft // 2 + 1] == 0)
    print("%s: largest local_error / budget %.2f" % (tag, worst))
    _note("torchgate_%d" % n_fft, cell["path"], worst)
    if lengths is not None and mask is None and not kw["nonstationary"]:
        # one full-length call per row: the fields of the last call are the last row's
        raw = _fetch(gate, 0)
        assert raw is not None and raw.shape[0] == 1 and raw.shape[2] == units[-1]["raw"].shape[1], tag
        cells, left = PB.bit_diff(raw[0] > 0.5, units[-1])
        assert left <= PB.LEFT_OUT_CAP and len(cells) == 0, "%s last row: decision bits differ at %s" % (tag, cells[:6].tolist())
        M = _fetch(gate, 1)
        cells, w = PB.mask_diff(M[0], units[-1], bound=PB.mask_bound(units[-1]["cfg"], integer_taps=False))
        assert len(cells) == 0, "%s last row: final mask off by up to %.3g" % (tag, w)
    if lengths is None and not kw["nonstationary"]:
        bits = _fetch(gate, 3)
        if bits is None:
            raw = _fetch(gate, 0)
            assert raw is not None, "%s: neither the bit field nor the raw mask can be fetched" % tag
            bits = raw > 0.5
        assert bits.shape[0] == B
        for b, u in enumerate(units):
            cells, left = PB.bit_diff(bits[b], u)
            assert left <= PB.LEFT_OUT_CAP
            assert len(cells) == 0, "%s row %d: %d decision bits differ from the oracle, first (band, frame) %s" % (
                tag, b, len(cells), cells[:6].tolist())
