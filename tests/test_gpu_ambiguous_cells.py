"""The exact re-evaluation of near-threshold cells, kernel by kernel, against the float64 oracle.

The inputs are tests/parity_budget.py's ``A_CELLS``: recordings built so that chosen cells -- every band, every frame
position of a workgroup, bins 0, n_fft / 4 and n_fft / 2 together in one crowded frame, the frames that read padding or
the neighbouring chunk -- lie within delta / 2 of their thresholds, on both sides.  Per cell and route:

* the kernels launched are the ones the route names (the stage-name rules of tests/test_gpu_stagewise.py);
* the decision bits equal the oracle's on EVERY cell of every unit inside ``debug_range()`` (TorchGate rows: every cell);
  differing target cells are named with band, frame, margin in units of delta, and unit;
* the output of every unit, per hop block, within the float32 budget (``local_check``; int16: equal to the truncated
  float64 result);
* a second run on the same handle gives the same bits and the same samples: the order in which the pending loop
  retires cells must not matter.

Which cells a kernel flagged ambiguous is not observable, and no counter is added to a kernel for it.  The delta / 2
condition tests/test_ambiguous_cells_host.py holds on the oracle stands in: the kernels' float32 error in |X|^2 and in
||x w||^2 is ~delta / 60 RMS, so a cell within delta / 2 is flagged whatever the rounding does.

Target counts, differing bits and the largest local_error / budget per cell and route go to the file named by
AMBIGUOUS_CELLS_OUT, if set (profiles/ambiguous_cells.json is that file from an MI355X run)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import parity_budget as PB
from tests.test_gpu_stagewise import _assert_route, _check_bits, _fetch, _make_sg, _stages

pytestmark = pytest.mark.gpu

_RESULTS = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_results():
    yield
    path = os.environ.get("AMBIGUOUS_CELLS_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "cells": dict(sorted(_RESULTS.items()))}, f, indent=1)


def _target_report(tag, case, bits, d0, d1):
    """Differing target cells of every unit inside frames [d0, d1): ``(targets compared, failure lines)``."""
    lines, n = [], 0
    for ui, u in enumerate(case["units"]):
        tf, tt = case["targets"][ui]
        inside = (tt >= d0) & (tt < d1)
        n += int(inside.sum())
        bad = inside & (bits[ui][tf, tt] != u["raw"][tf, tt].astype(bool))
        for i in np.flatnonzero(bad)[:8]:
            lines.append("unit %d (channel %d, chunk %d) band %d frame %d: margin %+.4f delta, kernel %d, oracle %d" % (
                ui, u["ch"], u["chunk"], tf[i], tt[i], case["margins"][ui][i], bits[ui][tf[i], tt[i]], u["raw"][tf[i], tt[i]]))
        if bad.sum() > 8:
            lines.append("unit %d: ... %d target cells in all" % (ui, int(bad.sum())))
    return n, lines


def _check_units(tag, case, got, bud):
    """Every unit's output per hop block; returns the largest local_error / budget."""
    got = np.atleast_2d(got)
    worst = 0.0
    for ui, u in enumerate(case["units"]):
        s0, e0 = u["dst"]
        bad, ratio = PB.local_check(got[u["ch"], s0:e0], u, bud=bud[ui])
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s unit %d (channel %d, chunk %d): hop blocks %s over their bound, largest error / budget " \
                              "%.2f" % (tag, ui, u["ch"], u["chunk"], bad[:10].tolist(), ratio)
    return worst


def _route_opts(name):
    from noisereduce_amd import _ffi
    return {"default": [], "force_split": [(_ffi.SG_OPT_FORCE_SPLIT, 1)], "force_nofast": [(_ffi.SG_OPT_FORCE_NOFAST, 1)]}[name]


S_CELLS = [c for c in PB.A_CELLS if c["family"] != "torchgate"]
R_CELLS = [c for c in PB.A_CELLS if c["family"] == "torchgate"]


@pytest.mark.parametrize("cell", S_CELLS, ids=PB.a_cell_id)
def test_cell(cell):
    from noisereduce_amd import _ffi
    case = PB.near_threshold_case(cell)
    units = case["units"]
    i16 = case["dtype"] == "int16"
    sg = _make_sg(case)
    gate = sg._gate
    bud = None if i16 else [PB.budget(u) for u in units]
    # (the stage-name rules of tests/test_gpu_stagewise.py take a cell of its own matrix)
    like = dict(family=cell["family"], n_fft=cell["n_fft"], col=1, short_window="W" in cell)
    gate.profile_enable(True)
    try:
        for route in cell["routes"]:
            tag = "%s [%s]" % (cell["name"], route)
            with gate.lock, gate.with_options(_route_opts(route)):
                gate.profile_read(reset=True)
                got = sg.get_traces()
                stages = _stages(gate)
                print("%s: launched %s" % (tag, sorted(stages)))
                assert got.dtype == np.dtype(case["dtype"])
                if case["dtype"] == "float32":
                    _assert_route(like, case, route, stages)
                elif i16:
                    assert "k_decide_fast" in stages and "k_gate_onepass" not in stages, (tag, sorted(stages))
                else:
                    assert "k_gate_onepass" in stages, (tag, sorted(stages))
                # the float32 decision kernels with the exact refinement, not the float64 ones (which share a stage name
                # with k_decide_lds / k_decide_mr): that route is taken by SG_OPT_FORCE_F64_DECIDE alone
                assert gate.get_option(_ffi.SG_OPT_FORCE_F64_DECIDE) == 0, tag
                if cell["family"] != "register" or "W" in cell:
                    assert ("k_stft_bits<decide>" in stages) == (cell["n_fft"] != 8192), (tag, sorted(stages))
                # (n_fft = 8192 has no float32 decision kernel: k_decide takes float64 decisions and keeps them as a float
                # field over every frame -- no ambiguity path there; the cell holds that route to the same bits)
                materialised = "k_decide" in stages
                assert materialised == (cell["n_fft"] == 8192), (tag, sorted(stages))

                def fetch_bits():
                    if materialised:
                        raw = _fetch(gate, 0)
                        assert raw is not None, "%s: the materialised kernels keep the raw mask" % tag
                        return raw > 0.5, (0, raw.shape[2])
                    b = _fetch(gate, 3)
                    assert b is not None, "%s: the bit-mask stages keep the decision bits" % tag
                    return b, gate.debug_range()
                bits, (d0, d1) = fetch_bits()
                n, lines = _target_report(tag, case, bits, d0, d1)
                diff = sum(len(PB.bit_diff(bits[ui], u, frames=(d0, d1))[0]) for ui, u in enumerate(units))
                if i16:
                    assert np.array_equal(got, np.trunc(case["out"]).astype(np.int16)), tag
                    worst = 0.0
                else:
                    worst = None
                _RESULTS["%s/%s" % (cell["name"], route)] = dict(targets=n, frames=[int(d0), int(d1)], differing_bits=diff,
                                                                 largest_local_error_over_budget=worst)
                assert not lines, "%s: %d decision bits differ from the oracle in frames [%d, %d); target cells among " \
                                  "them:\n%s" % (tag, diff, d0, d1, "\n".join(lines))
                assert n > 0
                _check_bits(tag, gate, units, materialised)
                if not i16:
                    worst = _check_units(tag, case, got, bud)
                    _RESULTS["%s/%s" % (cell["name"], route)]["largest_local_error_over_budget"] = worst
                print("%s: %d targets in frames [%d, %d), %d bits differ, largest local_error / budget %s" % (
                    tag, n, d0, d1, diff, worst))
                # once more on the same handle
                got2 = sg.get_traces()
                bits2 = fetch_bits()[0]
                assert np.array_equal(bits, bits2), "%s: a second run decides differently" % tag
                assert np.array_equal(got, got2), "%s: a second run gives other samples" % tag
    finally:
        gate.profile_enable(False)


@pytest.mark.parametrize("cell", R_CELLS, ids=PB.a_cell_id)
def test_torchgate_cell(cell):
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    case = PB.near_threshold_case(cell)
    units = case["units"]
    tag = cell["name"]
    tg = TorchGate(sr=PB.T_SR, **case["kw"]).cuda()
    x = torch.from_numpy(case["y"]).cuda()
    xn = None if case["xn"] is None else torch.from_numpy(case["xn"]).cuda()
    gate = tg._gate_for(x.device)
    # three rows are fewer than the row gate takes on its own: SG_OPT_FORCE_NOROWGATE = 2 routes every eligible shape to it
    own = xn is None
    opts = [(_ffi.SG_OPT_FORCE_NOROWGATE, 2)] if own else []

    def run():
        with gate.lock, gate.with_options(opts):
            return tg(x, xn).cpu().numpy()
    gate.profile_enable(True)
    try:
        gate.profile_read(reset=True)
        got = run()
        stages = _stages(gate)
    finally:
        gate.profile_enable(False)
    print("%s: launched %s" % (tag, sorted(stages)))
    if own:
        assert "k_row_gate" in stages and "k_decide" not in stages, (tag, sorted(stages))
    else:
        # with xn= TorchGate takes the four-kernel path and decides in float64 (k_decide): no ambiguity path, same bits
        assert "k_decide" in stages and "k_row_gate" not in stages, (tag, sorted(stages))

    def fetch_bits():
        b = _fetch(gate, 3)
        if b is None:
            raw = _fetch(gate, 0)
            assert raw is not None, "%s: neither the bit field nor the raw mask can be fetched" % tag
            b = raw > 0.5
        return b
    bits = fetch_bits()
    assert bits.shape[0] == len(units)
    T = units[0]["raw"].shape[1]
    n, lines = _target_report(tag, case, bits, 0, T)
    diff = 0
    for b, u in enumerate(units):
        cells, left = PB.bit_diff(bits[b], u)
        assert left == 0.0
        diff += len(cells)
    _RESULTS["%s/default" % tag] = dict(targets=n, frames=[0, T], differing_bits=diff, largest_local_error_over_budget=None)
    assert not lines and diff == 0, "%s: %d decision bits differ from the oracle; target cells among them:\n%s" % (
        tag, diff, "\n".join(lines))
    worst = 0.0
    for b, u in enumerate(units):
        k = len(u["want"])
        bad, ratio = PB.local_check(got[b, :k], u)
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s row %d: hop blocks %s over their bound (largest error / budget %.2f)" % (tag, b, bad[:10].tolist(), ratio)
    _RESULTS["%s/default" % tag]["largest_local_error_over_budget"] = worst
    print("%s: %d targets, %d bits differ, largest local_error / budget %.2f" % (tag, n, diff, worst))
    got2 = run()
    assert np.array_equal(bits, fetch_bits()), "%s: a second run decides differently" % tag
    assert np.array_equal(got, got2), "%s: a second run gives other samples" % tag
