"""The route matrix of TorchGate.forward (tests/parity_budget.py: ``R_CELLS``) on the CPU: conditions on the oracle alone,
so that the GPU pass of tests/test_gpu_torchgate_routes.py cannot be an empty one, and planted defects in the oracle's own
stages, each of which the checks of that file (``bit_diff`` / ``mask_diff`` and ``local_check``) must report.

Planted defects (what a slip in csrc/api.hip's sg_process_batch or in the kernels it launches would compute):

(a) ``thr_prev_row``      thresholds of row b - 1;
(b) ``thr_batch_offset``  thresholds of row b - u0: the batch offset dropped (vn.unit0 / the row index of a later batch);
(c) ``thr_prev_batch``    the whole last batch decided with the previous batch's thresholds (a stale thr_rows);
(d) ``max_next_row``      band maxima of row b + 1 (floor of the dB field, in the statistics and in the decisions);
(e) ``xn_one_thr``        the single-row threshold layout (ustride = 0) where xn has B rows: a batch's first row for all;
(f) ``noise_row0``        row 0's noise for every row;
(g) ``stats_Tm1``         statistics over frames 0 .. T - 2;
(h) ``stats_last_slice``  the last statistics slice dropped;
(i) ``ddof0``             the standard deviation with ddof = 0;
(j) ``mask_offset``       the final mask of the second batch written at the first batch's offset;
(k) control: the oracle's own stages recomputed here give the oracle's bits.

For each, whether ``O.rel_err < 1e-4`` on the whole output of the same cell sees it is held as measured here
(``OLD_BAR``).  It sees every one of them: a single flipped decision of a cell that is not tiny moves the output by
~1e-2 of the peak, on these inputs (rel_err 1.7e-2 .. 2.5) and equally on 37 statistically identical rows (white noise
and one common tone: thresholds of row b - 1 flip >= 960 cells per row, rel_err 0.19; frames 0 .. T - 2: >= 40 cells,
0.14; ddof = 0: >= 22 cells, 0.07).  So the old bar was not blind to these defects -- no test ran the branches they live
in (several unit batches, 16 rows and more with long rows, a noise row per row).  What the local checks add on top is
the name of the (row, band, frame), and rows 24 dB under the loudest one held as tightly as that one."""
import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB

TOL = 1e-4
STATIONARY = [c for c in PB.R_CELLS if not c["kw"].get("nonstationary")]
NONSTATIONARY = [c for c in PB.R_CELLS if c["kw"].get("nonstationary")]


def _raw_db(Z):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.abs(Z) + O.EPS64)


def _floored(db, mx):
    return np.maximum(db, mx[:, None] - 40.0)


def _batch_start(c, b):
    """First row of the unit batch row b runs in."""
    u0 = 0
    for nb in c["batches"]:
        if b < u0 + nb:
            return u0, nb
        u0 += nb
    raise IndexError(b)


def _fields(c):
    """Per row: the row's unfloored dB field, and that of what its statistics are taken from (the row itself, the one
    noise row, the row's noise row)."""
    case, units = PB.r_case(c), PB.r_oracle(c)
    rows = [_raw_db(u["Z"]) for u in units]
    if case["xn"] is None:
        return rows, rows
    n_fft, W, H = PB.r_geometry(c)
    Zn = O.stft_torch(case["xn"].astype(np.float64), n_fft, W, H, PB.tile_window(W))
    noise = [_raw_db(Zn[b if Zn.shape[0] > 1 else 0]) for b in range(len(units))]
    return rows, noise


def _thresh(db_raw, mx=None, frames=None, ddof=1):
    """mean + 1.5 std over ``frames`` of the dB field floored at ``mx`` - 40 (default: its own maxima over all frames)."""
    f = _floored(db_raw, db_raw.max(axis=1) if mx is None else mx)
    f = f if frames is None else f[:, frames[0]:frames[1]]
    return f.mean(axis=1) + 1.5 * f.std(axis=1, ddof=ddof)


def plant(c, what):
    """Decision bits per row with the defect planted (None: row untouched by construction), or -- ``mask_offset`` -- the
    displaced final masks."""
    units = PB.r_oracle(c)
    rows, noise = _fields(c)
    B = len(units)
    own = [_thresh(noise[b]) for b in range(B)]
    mx = [rows[b].max(axis=1) for b in range(B)]

    def bits(b, th, m=None):
        return _floored(rows[b], mx[b] if m is None else m) > th[:, None]
    out = []
    for b in range(B):
        u0, nb = _batch_start(c, b)
        last_u0 = c["B"] - c["batches"][-1]
        if what == "control":
            out.append(bits(b, own[b]))
        elif what == "thr_prev_row":
            out.append(bits(b, own[b - 1]))
        elif what == "thr_batch_offset":
            out.append(bits(b, own[b - u0]) if u0 else None)
        elif what == "thr_prev_batch":
            out.append(bits(b, own[b - c["batches"][-2]]) if u0 == last_u0 and len(c["batches"]) > 1 else None)
        elif what == "max_next_row":
            nxt = (b + 1) % B
            th = _thresh(noise[b], mx=noise[nxt].max(axis=1))
            out.append(bits(b, th, m=mx[nxt]))
        elif what == "xn_one_thr":
            out.append(bits(b, own[u0]) if b != u0 else None)
        elif what == "noise_row0":
            out.append(bits(b, own[0]) if b else None)
        elif what == "stats_Tm1":
            out.append(bits(b, _thresh(noise[b], frames=(0, noise[b].shape[1] - 1))))
        elif what == "stats_last_slice":
            Tn = noise[b].shape[1]
            nts = PB.r_stat_slices(c, Tn, nb, single_pass=c["xn"] == "rows" and nb < 16)
            out.append(bits(b, _thresh(noise[b], frames=(0, Tn * (nts - 1) // nts))) if nts > 1 else None)
        elif what == "ddof0":
            out.append(bits(b, _thresh(noise[b], ddof=0)))
        elif what == "mask_offset":
            n0, n1 = c["batches"][0], c["batches"][1]
            if b < min(n0, n1):
                out.append(units[n0 + b]["mask"])
            elif n0 <= b < n0 + n1:
                out.append(np.zeros_like(units[b]["mask"]))
            else:
                out.append(None)
        else:
            raise KeyError(what)
    return out


_BUD = {}


def _budget(c, b):
    if (c["name"], b) not in _BUD:
        _BUD[(c["name"], b)] = PB.budget(PB.r_oracle(c)[b])
    return _BUD[(c["name"], b)]


def report(c, what, planted):
    """(rows touched, rows the bit / mask check names, rows failing local_check, fewest differing cells in a named row,
    rel_err of the whole output)."""
    units = PB.r_oracle(c)
    touched = named = failed = 0
    fewest = None
    got = []
    for b, (u, p) in enumerate(zip(units, planted)):
        if p is None:
            got.append(u["want"])
            continue
        touched += 1
        if what == "mask_offset":
            cells, _ = PB.mask_diff(p, u)
            g = PB.regate(u, mask=p) if len(cells) else u["want"]
        else:
            cells, left = PB.bit_diff(p, u)
            assert left == 0.0
            g = PB.regate(u, raw=p.astype(np.float64)) if len(cells) else u["want"]
        if len(cells):
            named += 1
            fewest = len(cells) if fewest is None else min(fewest, len(cells))
            failed += len(PB.local_check(g, u, bud=_budget(c, b))[0]) > 0
        got.append(g)
    return touched, named, failed, fewest or 0, O.rel_err(np.stack(got), np.stack([u["want"] for u in units]))


# ---- conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", STATIONARY, ids=PB.r_cell_id)
def test_stationary_cell_conditions(cell):
    case, units = PB.r_case(cell), PB.r_oracle(cell)
    B, T = cell["B"], cell["T"]
    assert len(units) == B and sum(cell["batches"]) == B
    assert all(u["raw"].shape == (cell["n_fft"] // 2 + 1, T) for u in units)
    assert case["x"].shape == (B, (T - 1) * case["H"] + 13)
    # nothing ambiguous: no cell within 1e-7 dB of its threshold, bit_diff leaves nothing out
    margin = min(PB.nearest_margin_db(u) for u in units)
    assert margin > 1e-7, margin
    for u in units:
        cells, left = PB.bit_diff(u["raw"], u)
        assert len(cells) == 0 and left == 0.0
    # every row passes some cells and gates some
    share = [float(np.mean(u["raw"])) for u in units]
    assert 0.005 <= min(share) and max(share) <= 0.99, (min(share), max(share))
    # floor rows: the 40 dB floor lifts cells of some bands and leaves others alone
    floor_rows = [b for b in range(B) if b % PB.R_FLOOR_EVERY == PB.R_FLOOR_EVERY - 1]
    assert floor_rows
    lifted_n = []
    for b in floor_rows:
        db = _raw_db(units[b]["Z"])
        lifted = db.min(axis=1) < db.max(axis=1) - 40.0
        assert lifted.any() and not lifted.all(), b
        lifted_n.append(int(lifted.sum()))
    # per-row thresholds: adjacent rows >= 1 dB apart in at least half the bands
    per_row = cell["xn"] != "one"
    apart = 1.0
    if per_row:
        th = np.stack([u["thresh"] for u in units])
        apart = min(float(np.mean(np.abs(th[b] - th[b - 1]) >= 1.0)) for b in range(1, B))
        assert apart >= 0.5, apart
    else:
        assert all(np.array_equal(u["thresh"], units[0]["thresh"]) for u in units)
    # the side of 64 / 128 frames, 160 rows, 16 rows per batch the route stands on
    bits_path = cell["route"] in ("row_gate", "row_decide", "t2")
    if cell["route"] == "row_gate":
        assert T <= 64 and B >= 160 and cell["xn"] is None
    elif cell["route"] == "row_decide":
        assert T <= 128 and (T > 64 or B < 160 or cell["xn"])
    elif cell["route"] == "t2":
        assert T > 128
    if cell["xn"] == "rows":
        assert case["xn"].shape == (B, (cell["xnT"] - 1) * case["H"] + 13) and cell["xnT"] != T
    # no statistics launch slices its frames evenly
    for what, Ts, nb, single in PB.r_stats_launches(cell):
        nts = PB.r_stat_slices(cell, Ts, nb, single)
        assert nts == 1 or Ts % nts != 0, (what, Ts, nb, nts)
    # a budgeted cell: the budget is for the split the table names
    if len(cell["batches"]) > 1:
        per = PB.r_unit_bytes(cell["n_fft"], max(T, cell["xnT"] or 0))
        ub = PB.r_budget(cell) // per
        assert ub == cell["batches"][0]
        assert cell["batches"] == [min(ub, B - u0) for u0 in range(0, B, ub)]
    print("%s: nearest cell %.2e dB from its threshold, passing share %.4f .. %.4f, lifted bands in the floor rows %d .. %d, "
          "adjacent thresholds >= 1 dB apart in %.0f %% of the bands%s" % (
              cell["name"], margin, min(share), max(share), min(lifted_n), max(lifted_n), 100 * apart,
              "" if bits_path else " (float mask route)"))


@pytest.mark.parametrize("cell", NONSTATIONARY, ids=PB.r_cell_id)
def test_nonstationary_cell_conditions(cell):
    case, units = PB.r_case(cell), PB.r_oracle(cell)
    assert len(units) == cell["B"] and sum(cell["batches"]) == cell["B"] and len(cell["batches"]) == 3
    per = PB.r_unit_bytes(cell["n_fft"], cell["T"])
    assert PB.r_budget(cell) // per == cell["batches"][0]
    for u in units:
        assert u["raw"].shape[1] == cell["T"]
        assert np.mean(u["raw"] < 0.1) > 0.01 and np.mean(u["raw"] > 0.9) > 0.001      # both ends of the sigmoid
    # rows differ: the final mask of a row is 1000 x further from its neighbour's than the field rule allows (~1e-5)
    # in thousands of cells
    for b in range(1, cell["B"]):
        assert np.sum(np.abs(units[b]["mask"] - units[b - 1]["mask"]) > 0.01) >= 1000


# ---- planted defects -----------------------------------------------------------------------------------------------
# (cell, defect) -> does ``rel_err < 1e-4`` on the whole output see it?  As measured here (the figures are printed).
OLD_BAR = {
    ("split", "thr_prev_row"): True, ("split", "thr_batch_offset"): True, ("split", "thr_prev_batch"): True,
    ("split", "max_next_row"): True, ("split", "stats_Tm1"): True, ("split", "stats_last_slice"): True,
    ("split", "ddof0"): True, ("split", "mask_offset"): True,
    ("split-xnB", "thr_prev_row"): True, ("split-xnB", "thr_batch_offset"): True, ("split-xnB", "thr_prev_batch"): True,
    ("split-xnB", "max_next_row"): True, ("split-xnB", "xn_one_thr"): True, ("split-xnB", "noise_row0"): True,
    ("split-xnB", "stats_Tm1"): True, ("split-xnB", "stats_last_slice"): True, ("split-xnB", "ddof0"): True,
    ("split-xnB", "mask_offset"): True,
}
# defects that touch every row they are planted in by hundreds of cells: every touched row must be named
EVERY_ROW = ("thr_prev_row", "thr_batch_offset", "thr_prev_batch", "xn_one_thr", "noise_row0", "mask_offset")


@pytest.mark.parametrize("name", ["split", "split-xnB"])
def test_control_reproduces_the_oracle(name):
    cell = PB.r_cell(name)
    for u, p in zip(PB.r_oracle(cell), plant(cell, "control")):
        assert np.array_equal(p, u["raw"].astype(bool))


@pytest.mark.parametrize("name,what", sorted(OLD_BAR), ids=["%s-%s" % k for k in sorted(OLD_BAR)])
def test_planted_defect_is_named(name, what):
    cell = PB.r_cell(name)
    touched, named, failed, fewest, err = report(cell, what, plant(cell, what))
    print("%s %-16s: planted in %d rows, bit / mask check names %d (fewest differing cells in one: %d), local_check fails in "
          "%d, output rel_err %.2e (the 1e-4 bar %s it)" % (name, what, touched, named, fewest, failed, err,
                                                           "sees" if err >= TOL else "MISSES"))
    assert touched >= 1 and named >= 1 and failed >= 1
    if what in EVERY_ROW:
        assert named == touched and failed == touched
    assert (err >= TOL) == OLD_BAR[(name, what)], "%s: rel_err %.2e" % (what, err)
