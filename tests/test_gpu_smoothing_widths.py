"""Mask smoothing at every width the engine routes on (tests/parity_budget.py: ``W_CELLS``), held to the float64 oracle
with the checks of tests/test_gpu_stagewise.py (tests/stagewise_checks.py: decision bits, smoothed mask, final mask / raw
sigmoid, every hop block of every unit) -- one cell on each side of every edge of csrc/api.hip's routing on
(n_grad_freq, n_grad_time).  tests/test_smoothing_widths_host.py holds the conditions on the inputs and restates the
routing; here every route of a cell must report the smoothing kernel, cell type and tile height its label names
(``Gate.smooth_route()``: sg_debug_counter 17), so that no cell quietly runs elsewhere.  Where the one-pass gate runs, its
output is bit-equal to the SG_OPT_FORCE_SPLIT output (prop_decrease = 1).

The largest local_error / budget per cell and route goes to the file named by PARITY_BUDGET_OUT, if set
(profiles/parity_budget_widths.json is that file from an MI355X run of this module alone)."""
import json
import os

import numpy as np
import pytest

from tests import parity_budget as PB
from tests import stagewise_checks as SC

pytestmark = pytest.mark.gpu

_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_ratios():
    yield
    path = os.environ.get("PARITY_BUDGET_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "largest_local_error_over_budget": dict(sorted(_RATIOS.items()))},
                      f, indent=1)


def _options(route):
    from noisereduce_amd import _ffi
    return {"default": [], "force_split": [(_ffi.SG_OPT_FORCE_SPLIT, 1)], "force_nofast": [(_ffi.SG_OPT_FORCE_NOFAST, 1)],
            "force_unfused": [(_ffi.SG_OPT_FORCE_UNFUSED, 1)]}[route]


@pytest.mark.parametrize("cell", PB.W_CELLS, ids=PB.w_cell_id)
def test_width_cell(cell):
    case = PB.w_case(cell)
    out, units = PB.w_oracle(cell)
    labels = {r: PB.w_route(cell, r) for r in cell["routes"]}

    def assert_route(route, stages, gate):
        got = gate.smooth_route()
        assert got == labels[route], "%s [%s]: smoothed by %s, labelled %s (launched %s)" % (
            cell["name"], route, got, labels[route], sorted(stages))

    family = cell["name"][:-4] if cell["name"].endswith("-f64") else cell["name"]       # (check_output appends _f64)
    outputs = SC.run_cell(cell["name"], family, case, out, units, SC.make_sg(case),
                          [(r, _options(r)) for r in cell["routes"]], assert_route,
                          raw_exists=lambda route, stages: labels[route][0] != "k_iir_mask<nt>", ratios=_RATIOS)
    if labels.get("default", ("",))[0].startswith("k_gate_onepass") and "force_split" in outputs:
        assert np.array_equal(outputs["default"], outputs["force_split"]), \
            "%s: the one-pass gate's output is not bit-equal to the three-kernel path's" % cell["name"]


# ---- TorchGate.forward -----------------------------------------------------------------------------------------------
def _torchgate_rows(tag, tg, gate, x, xn, units, lengths=None, integer_taps=False):
    """The way of tests/test_gpu_stagewise.py::test_torchgate_cell: every row per hop block, decision bits, and the final
    mask the call hands back (stationary: ``mask_bound``; non-stationary: ``_field_rule``)."""
    F = 513
    if lengths is None:
        got = tg(x, xn).cpu().numpy()
        route = gate.smooth_route()
        with gate.lock:
            got2, mask = gate.process_batch(x, xn, save_mask=True)
    else:
        got = tg(x, xn, lengths=lengths).cpu().numpy()
        route = None
        with gate.lock:
            got2, mask = gate.process_rows(x, lengths, xn, None, save_mask=True)
    assert np.array_equal(got2.cpu().numpy(), got), "%s: a second call gives other samples" % tag
    mask = mask.cpu().numpy()
    worst = 0.0
    for b, u in enumerate(units):
        n = len(u["want"])
        emu = PB.emulate_stages_f32(u)
        bad, ratio = PB.local_check(got[b, :n], u, bud=PB.budget(u, emu[0]))
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s row %d: hop blocks %s over their bound (largest error / budget %.2f)" % (
            tag, b, bad[:10].tolist(), ratio)
        assert np.all(got[b, n:] == 0)
        T = u["mask"].shape[1]
        M = mask[b, :T, :F].T
        if u["cfg"]["stationary"]:
            cells, w = PB.mask_diff(M, u, bound=PB.mask_bound(u["cfg"], integer_taps=integer_taps))
            assert len(cells) == 0, "%s row %d: final mask off by up to %.3g at %d cells, first %s" % (
                tag, b, w, len(cells), cells[:6].tolist())
        else:
            PB._field_rule(M, u["mask"], emu[2], "%s row %d final mask" % (tag, b))
        assert np.all(mask[b, T:, :F] == 0)
    print("%s: largest local_error / budget %.2f" % (tag, worst))
    SC.note(tag, "forward" if lengths is None else "lengths", worst, _RATIOS)
    return route


@pytest.mark.parametrize("cell", PB.TW_CELLS, ids=PB.tw_cell_id)
def test_torchgate_width_cell(cell):
    import torch
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    case, units = PB.tw_case(cell), PB.tw_oracle(cell)
    tg = TorchGate(sr=PB.SR, **case["kw"]).cuda()
    x = torch.from_numpy(case["x"]).cuda()
    xn = None if case["xn"] is None else torch.from_numpy(case["xn"]).cuda()
    gate = tg._gate_for(x.device)
    label = PB.tw_route(cell)
    opts = [(_ffi.SG_OPT_FORCE_NOROWGATE, 2)] if cell.get("rowgate") else []
    with gate.with_options(opts):
        got = _torchgate_rows(cell["name"], tg, gate, x, xn, units,
                              integer_taps=label[0] in ("k_row_gate", "k_smooth_bits2", "k_smooth_bits"))
        assert got == label, "%s: smoothed by %s, labelled %s" % (cell["name"], got, label)
        if cell["gate"] == "T":
            bits = SC.fetch(gate, 3)
            if bits is None:
                raw = SC.fetch(gate, 0)
                assert raw is not None, "%s: neither the bit field nor the raw mask can be fetched" % cell["name"]
                bits = raw > 0.5
            assert bits.shape[0] == len(units)
            for b, u in enumerate(units):
                cells, left = PB.bit_diff(bits[b], u)
                assert left <= PB.LEFT_OUT_CAP
                assert len(cells) == 0, "%s row %d: %d decision bits differ from the oracle, first (band, frame) %s" % (
                    cell["name"], b, len(cells), cells[:6].tolist())


@pytest.mark.parametrize("cell", PB.M_CELLS, ids=PB.m_cell_id)
def test_movemean_cell(cell):
    import torch
    from noisereduce_amd.torchgate import TorchGate
    case, units = PB.m_case(cell), PB.m_oracle(cell)
    tg = TorchGate(sr=PB.SR, **case["kw"]).cuda()
    x = torch.from_numpy(case["x"]).cuda()
    gate = tg._gate_for(x.device)
    route = _torchgate_rows(cell["name"], tg, gate, x, None, units, lengths=case["lengths"])
    if case["lengths"] is None:     # k_box_mask only knows the default length; every other one: k_boxcar_sigmoid + smoothing
        assert route == ("k_smooth_tiled", 4, 64), route
