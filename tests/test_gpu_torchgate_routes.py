"""TorchGate.forward's full-length routes (csrc/api.hip: sg_process_batch) against the float64 oracle, per row and per hop
block, on the route matrix of tests/parity_budget.py (``R_CELLS``): rows below / from 16 per unit batch, rows of up to 64 /
128 / more frames, thresholds from the rows, from one noise row, from a noise row per row, one and several unit batches.
tests/test_torchgate_routes_host.py holds the conditions that make a pass here mean something.

Every cell:

* the profiled stages of the call are exactly those of the cell's route, once per unit batch, and the handle reports the
  split the cell means to run in (launch counts per stage, rows of the last batch) -- a cell that ran in one batch when it
  meant three fails;
* every row's output within ``PB.local_check`` of its oracle unit, all rows of every unit batch;
* stationary: the decision bits of the last unit batch equal the oracle's on every cell (``bit_diff``), and the final mask
  of ALL rows (``process_batch(save_mask=True)``) is within ``mask_bound`` of the oracle's -- the smallest smoothing tap is
  far above that bound, so the mask holds the bits of the batches whose fields can no longer be fetched;
* non-stationary: ``_field_rule`` on the saved mask of every row;
* a second run on the same handle gives the same samples and mask;
* a ``split*`` cell once more with the default budget (one batch): bitwise the same samples and mask;
* ``b16`` once more with SG_OPT_FORCE_NOFAST: the same bits;
* ``b16`` / ``split``: a NaN sample in one row leaves the other rows bitwise alone and makes exactly the oracle's samples
  of that row non-finite (``b16``: the NaN-sticky atomic maximum of the transform; ``split``: a row of the 5-row batch,
  ``nanmax`` in k_colmax).

Stages share profiling scopes: k_row_decide, k_t2_rows + k_decide_bits_t2 and k_decide all count as "k_decide", the
single-pass k_colstats1 pair and k_colstats as "k_colstats".  Which of them ran follows from the frames per row and the
rows per batch that api.hip branches on; both are asserted from what the handle reports.

The largest local_error / budget per cell goes to the file named by TORCHGATE_ROUTES_OUT, if set
(profiles/torchgate_routes.json is that file from an MI355X run)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB

pytestmark = pytest.mark.gpu

_RATIOS = {}
_BITS_ROUTES = ("row_gate", "row_decide", "t2")


def _note(name, ratio):
    _RATIOS[name] = max(_RATIOS.get(name, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _dump_ratios():
    yield
    path = os.environ.get("TORCHGATE_ROUTES_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "largest_local_error_over_budget": dict(sorted(_RATIOS.items()))},
                      f, indent=1)


def expected_stages(cell, batches):
    """{first word of a profiled stage: launches} of one call of the cell run in ``batches`` (api.hip: sg_process_batch)."""
    n = len(batches)
    route, xn = cell["route"], cell["xn"]
    if route in ("box", "ns_raw"):
        want = {"k_box_mask": n, "k_apply_fast": n}
        if route == "ns_raw":
            want["mask"] = n
        return want
    if route == "row_gate":
        return {"k_row_gate": n}
    rows_stats = route in ("t2", "float")       # k_row_decide takes the statistics of its own tile
    want = {
        "k_stft<double>": (1 if xn == "one" else 0) + n * (2 if xn == "rows" else 1),
        "k_colstats": (1 if xn == "one" else 0) + (n if xn == "rows" else 0) + (n if rows_stats and xn is None else 0),
        "k_colmax": sum(1 for nb in batches if rows_stats and nb < 16),
        "k_decide": n,
        "mask": n,
    }
    if cell["apply"] == "ola":
        want.update({"k_apply_istft": n, "k_ola": n})
    else:
        want["k_apply_fast"] = n
    return {k: v for k, v in want.items() if v}


def _make(cell, budget):
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    case = PB.r_case(cell)
    tg = TorchGate(sr=PB.R_SR, **case["kw"])
    gate = _ffi.Gate("cuda", **PB.torchgate_gate_kwargs(tg, max_workspace_bytes=budget))
    if cell.get("nofast"):
        gate.set_option(_ffi.SG_OPT_FORCE_NOFAST, 1)
    return gate


def _dims(gate):
    d = (ctypes.c_int64 * 3)()
    gate._check(gate.lib.sg_debug_dims(gate._h, d))
    return int(d[0]), int(d[1])


def _call(gate, x, xn):
    """One profiled process_batch: (samples, mask, {stage: launches}, rows of the last batch, its frames)."""
    gate.profile_enable(True)
    try:
        gate.profile_read(reset=True)
        y, mask = gate.process_batch(x, xn, save_mask=True)
        stages = {k.split(" ")[0]: v[1] for k, v in gate.profile_read(reset=True).items() if v[1] > 0}
    finally:
        gate.profile_enable(False)
    return (y, mask, stages) + _dims(gate)


def _assert_split(tag, cell, batches, stages, last, T):
    """The call ran the cell's route in exactly ``batches``: one profiling scope per batch per stage, k_colmax only in
    batches below 16 rows, and the rows of the last batch as the handle reports them."""
    want = expected_stages(cell, batches)
    if cell["route"] in ("box", "ns_raw"):
        mag = stages.pop("k_mag_fast*", 0)
        assert mag >= len(batches), "%s: the magnitude transform ran %d times in %d batches" % (tag, mag, len(batches))
    assert stages == want, "%s: launched %s, the route in batches %s launches %s" % (tag, stages, batches, want)
    assert (last, T) == (batches[-1], cell["T"]), "%s: the last batch held %d rows of %d frames, not %d of %d" % (
        tag, last, T, batches[-1], cell["T"])


def _last_bits(gate, cell):
    """Decision bits of the last unit batch as (rows, F, T)."""
    if cell["route"] in _BITS_ROUTES:
        return np.swapaxes(gate.debug_field(3), 1, 2)
    return np.swapaxes(gate.debug_field(0), 1, 2) > 0.5


def _check_rows(tag, cell, units, got, mask):
    """Output per hop block and final mask of every row; returns the largest local_error / budget."""
    F = cell["n_fft"] // 2 + 1
    stationary = units[0]["cfg"]["stationary"]
    integer_taps = cell["route"] in _BITS_ROUTES
    worst = 0.0
    assert got.shape == (len(units), len(units[0]["want"])), (tag, got.shape)
    assert mask.shape[:2] == (len(units), cell["T"]), (tag, mask.shape)
    for b, u in enumerate(units):
        emu = PB.emulate_stages_f32(u)
        bud = PB.budget(u, emu[0])
        bad, ratio = PB.local_check(got[b], u, bud=bud)
        worst = max(worst, ratio)
        if len(bad):
            err = PB.local_error(got[b], u["want"], u["cfg"]["H"])
            raise AssertionError("%s row %d: hop blocks %s of %d over their bound: error %s, budget %s, largest error / budget "
                                 "in the row %.2f" % (tag, b, bad[:10].tolist(), len(err), err[bad[:10]], bud[bad[:10]], ratio))
        M = mask[b, :, :F].T
        if stationary:
            bound = PB.mask_bound(u["cfg"], integer_taps=integer_taps)
            cells, w = PB.mask_diff(M, u, bound=bound)
            assert len(cells) == 0, "%s row %d: final mask off by up to %.3g (bound %.3g) at %d cells, first (band, frame) %s" % (
                tag, b, w, bound, len(cells), cells[:6].tolist())
        else:
            PB._field_rule(M, u["mask"], emu[2], "%s row %d final mask" % (tag, b))
    return worst


def _nan_rows(tag, cell, case, gate, x, xn, y, row):
    """A NaN sample in ``row``: the other rows bitwise what they were, the row's non-finite samples the oracle's."""
    pos = case["L"] // 3
    bad = x.clone()
    bad[row, pos] = float("nan")
    yb = gate.process_batch(bad, xn)
    keep = [b for b in range(cell["B"]) if b != row]
    assert torch.equal(yb[keep], y[keep]), "%s: a NaN sample in row %d changed another row" % (tag, row)
    xr = case["x"][row:row + 1].astype(np.float64)
    xr[0, pos] = np.nan
    with np.errstate(all="ignore"):
        want = O.torchgate_T(xr, PB.R_SR, window=PB.tile_window(case["W"]), **case["kw"])[0]
    got = yb[row].cpu().numpy()
    assert 0 < np.sum(~np.isfinite(want)) < want.size
    assert np.array_equal(~np.isfinite(got), ~np.isfinite(want)), "%s: row %d has %d non-finite samples, the oracle %d" % (
        tag, row, int(np.sum(~np.isfinite(got))), int(np.sum(~np.isfinite(want))))


@pytest.mark.parametrize("cell", PB.R_CELLS, ids=PB.r_cell_id)
def test_route_cell(cell):
    from noisereduce_amd import _ffi
    tag = cell["name"]
    case, units = PB.r_case(cell), PB.r_oracle(cell)
    tdt = torch.float64 if case["dtype"] == "float64" else torch.float32
    x = torch.from_numpy(case["x"]).to(tdt).cuda()
    xn = None if case["xn"] is None else torch.from_numpy(case["xn"]).to(tdt).cuda()
    batches = cell["batches"]
    gate = _make(cell, PB.r_budget(cell))
    try:
        y, mask, stages, last, T = _call(gate, x, xn)
        _assert_split(tag, cell, batches, stages, last, T)
        assert y.dtype == tdt
        got, M = y.cpu().numpy(), mask.cpu().numpy()
        worst = _check_rows(tag, cell, units, got, M)
        print("%s: largest local_error / budget %.2f" % (tag, worst))
        _note(tag, worst)
        bits = None
        if case["stationary"]:
            bits = _last_bits(gate, cell)
            assert bits.shape[0] == batches[-1]
            for i, u in enumerate(units[cell["B"] - batches[-1]:]):
                cells, left = PB.bit_diff(bits[i], u)
                assert left <= PB.LEFT_OUT_CAP
                assert len(cells) == 0, "%s row %d: %d decision bits differ from the oracle, first (band, frame) %s" % (
                    tag, cell["B"] - batches[-1] + i, len(cells), cells[:6].tolist())
        # a second run on the same handle
        # (the mask's columns beyond bin F - 1 pad a row to a multiple of 16 and are never written)
        F = cell["n_fft"] // 2 + 1
        y2, mask2 = gate.process_batch(x, xn, save_mask=True)
        assert torch.equal(y2, y), "%s: a second run on the same handle gives other samples" % tag
        assert torch.equal(mask2[:, :, :F], mask[:, :, :F]), "%s: a second run on the same handle gives another mask" % tag
        if tag == "b16":
            with gate.with_options([(_ffi.SG_OPT_FORCE_NOFAST, 1)]):
                _, _, st2, last2, _ = _call(gate, x, xn)
                assert "k_apply_istft" in st2 and "k_colmax" not in st2 and last2 == 16, st2
                raw = np.swapaxes(gate.debug_field(0), 1, 2) > 0.5
            assert np.array_equal(raw, bits), "%s: the LDS transform's route decides %d cells otherwise" % (
                tag, int(np.sum(raw != bits)))
        if tag in ("b16", "split"):
            _nan_rows(tag, cell, case, gate, x, xn, y, row=5 if tag == "b16" else 34)
    finally:
        gate.close()
    if len(batches) > 1:
        one = _make(cell, 0)
        try:
            y1, mask1, stages1, last1, _ = _call(one, x, xn)
            _assert_split(tag + " [default budget]", cell, [cell["B"]], stages1, last1, cell["T"])
            assert torch.equal(y1, y), "%s: %d samples differ between %d batches and one" % (
                tag, int((y1 != y).sum()), len(batches))
            assert torch.equal(mask1[:, :, :F], mask[:, :, :F]), "%s: the saved mask differs between %d batches and one" % (tag, len(batches))
        finally:
            one.close()
