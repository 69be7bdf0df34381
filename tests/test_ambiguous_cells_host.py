"""The near-threshold cells of tests/parity_budget.py (``A_CELLS``) on the CPU: conditions on the oracle alone, so that
the GPU pass of tests/test_gpu_ambiguous_cells.py cannot be an empty one, and planted defects of the exact
re-evaluation, each of which ``bit_diff`` must report on the target cells.

Which cells a kernel flags ambiguous cannot be observed.  What stands in for it: every target lies within delta / 2 of
its threshold, delta = 2^-16 ||x w||_2 computed in float64 from the stored samples; the kernels' float32 error in |X|^2
and in ||x w||^2 is ~delta / 60 RMS, so a cell this close is flagged whatever the rounding does.

The defects are planted in the oracle's own stages: the oracle's bits everywhere, and at the target cells the bit an
exact sum WITH the defect gives.

(a) decisions from the float32 transform alone (``spectrum_f32``);
(b) the exact sum taken at band f + 1 (f - 1 at Nyquist) for the targets on bands 0, n_fft / 4, n_fft / 2;
(c) the exact sum taken at frame t + 1 (t - 1 in the last frame);
(d) the exact sum without the chunk offset: a later chunk's targets read chunk 0's samples;
(e) the float32-rounded window in the exact sum;
(f) only the first target of each frame re-evaluated, the rest left to float32;
(g) control: the oracle's own bits.

For each, whether ``O.rel_err < 1e-4`` on the output sees it is asserted as measured here (``OLD_BAR``).

(e) is below what any float32 input can show, and no flip is asserted for it: a window rounded to float32 moves the
exact sum by 2^-25 ||x|| x 0.6 ~ 1e-3 delta RMS, the size of the float32 rounding of the samples themselves, while the
goals start at 5e-8 T ~ 6e-3 delta.  Its test holds the measured movement (RMS over 1e-4 delta, largest under
delta / 100); measured: no target of any cell flips.  A float32 window in a kernel's exact sum stays undetectable here.
"""
import os
import re

import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB

TOL = 1e-4
FLOAT32_CELLS = [c for c in PB.A_CELLS if c.get("dtype", "float32") == "float32"]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "noisereduce_amd", "csrc")


def _const(file, pattern):
    with open(os.path.join(CSRC, file)) as f:
        m = re.search(pattern, f.read(), re.S)
    assert m, "%s: %s not found" % (file, pattern)
    return int(m.group(1))


def workgroup_frames(cell):
    """Frames per workgroup of every decision kernel a route of the cell can launch, read from the sources: the
    register kernels' frames per wave x 4 waves (k_decide_fast / k_gate_onepass: WAVES quads of 4 frames), and
    WAVES x FPW of launch_decide_lds_n / launch_bits_n / the mixed-radix teams -- the team rules restated from api.hip
    (team_threads, team_count) with SG_TEAM_N and FPW parsed."""
    n_fft = cell["n_fft"]
    if cell["family"] == "torchgate":
        return set()                                   # one row per workgroup, or float64 decisions
    N = n_fft // 2
    team_n = _const("api.hip", r"#define SG_TEAM_N (\d+)")
    fpw_lds = _const("api.hip", r"launch_decide_lds_n\(.*?constexpr int FPW = (\d+);")
    fpw_bits = _const("api.hip", r"launch_bits_n\(.*?constexpr int FPW = (\d+);")
    waves_fast = _const("api.hip", r"SG_STAGE_DECIDE_FAST, st\);\s*constexpr int WAVES = (\d+);")
    out = set()
    if cell["family"] == "mixed_radix":
        # k_decide_mr: teams x fpw (mixed.hip).  mr_fpw gives 1 frame per team to a call of fewer than 1024 workgroups
        # (these cells: 4 units), mr_team one wavefront or less per frame up to N = 1024 (256 threads: at most 16 teams
        # of 16 lanes) and the whole workgroup on one frame beyond
        assert _const("mixed.hip", r"g\.T \+ s\.teams \* 4 - 1\) / \(s\.teams \* 4\)\) < (\d+) \? 1 : 4;") == 1024
        return {16 if N <= 1024 else 1}
    if N & (N - 1) == 0 and N < team_n * 2:
        nt = 16 if N <= 128 else (32 if N == 256 else 64)
        waves = 256 // nt if nt < 64 else (2 if N * 8 > 8192 else 4)
        out.add(waves * fpw_lds)                       # k_decide_lds (the default of the LDS sizes, FORCE_NOFAST of 1024)
    if N >= team_n * 2:
        out.add(1 * fpw_bits)                          # n_fft = 8192: float64, the whole workgroup on one frame
    if cell["family"] == "register" and "W" not in cell:
        out.add({1024: 4 * waves_fast, 512: 4 * _const("fast512.hpp", r"constexpr int F5_FPW = (\d+);"),
                 256: 4 * _const("fast256.hpp", r"constexpr int F25_FPW = (\d+);"), 2048: 2 * 4}[n_fft])
    return out


def _passes(mag, f, u):
    return 20.0 * np.log10(mag + O.EPS64) > u["thresh"][f]


def _plant(case, what):
    """Per unit ``(bits, affected)``: the oracle's bits with the targets' bits retaken under a defect, and the indices
    (into the unit's targets) of the targets the defect touches."""
    units = case["units"]
    out = []
    for ui, u in enumerate(units):
        tf, tt = case["targets"][ui]
        F, T = u["raw"].shape
        bits = u["raw"].astype(bool).copy()
        aff = np.arange(len(tf))
        if what == "control":
            aff = aff[:0]
        elif what == "float32":
            bits[tf, tt] = _passes(np.abs(PB.spectrum_f32(u)[tf, tt]).astype(np.float64), tf, u)
        elif what == "band":
            aff = np.flatnonzero((tf == 0) | (4 * tf == u["cfg"]["n_fft"]) | (tf == F - 1))
            f2 = np.where(tf[aff] == F - 1, tf[aff] - 1, tf[aff] + 1)
            bits[tf[aff], tt[aff]] = _passes(np.abs(u["Z"][f2, tt[aff]]), tf[aff], u)
        elif what == "frame":
            t2 = np.where(tt == T - 1, tt - 1, tt + 1)
            bits[tf, tt] = _passes(np.abs(u["Z"][tf, t2]), tf, u)
        elif what == "chunk_offset":
            if u["chunk"] == 0:
                aff = aff[:0]
            else:
                u0 = next(v for v in units if v["ch"] == u["ch"] and v["chunk"] == 0)
                assert u0["Z"].shape == u["Z"].shape
                bits[tf, tt] = _passes(np.abs(u0["Z"][tf, tt]), tf, u)
        elif what == "window32":
            bits[tf, tt] = _passes(np.abs(_spectrum_window32(u)[tf, tt]), tf, u)
        elif what == "first_only":
            first = np.zeros(len(tf), dtype=bool)
            for t in np.unique(tt):
                i = np.flatnonzero(tt == t)
                first[i[np.argmin(tf[i])]] = True
            aff = np.flatnonzero(~first)
            bits[tf[aff], tt[aff]] = _passes(np.abs(PB.spectrum_f32(u)[tf[aff], tt[aff]]).astype(np.float64), tf[aff], u)
        else:
            raise KeyError(what)
        out.append((bits, aff))
    return out


def _spectrum_window32(u):
    """The unit's float64 transform with the window rounded to float32, (F, T), in the scale of ``u['Z']`` (variant S;
    TorchGate's window table IS float32, so the defect does not exist there)."""
    c = u["cfg"]
    assert c["variant"] == "S"
    w, n_frame = O.hann_periodic(c["W"]), c["W"]
    w32 = w.astype(np.float32).astype(np.float64)
    x = np.asarray(u["x"], dtype=np.float64)
    fr = PB._a_frames(x, -(n_frame // 2), 0, len(x), u["raw"].shape[1], n_frame, c["H"])
    return (np.fft.rfft(fr * w32[None, :], n=c["n_fft"], axis=-1) / np.sum(w)).T


def _report(case, planted):
    """(flipped, affected, rel_err of the output): what ``bit_diff`` names among the targets, and the old bar."""
    flipped = affected = 0
    got, want = [], []
    for ui, (u, (bits, aff)) in enumerate(zip(case["units"], planted)):
        tf, tt = case["targets"][ui]
        cells, left = PB.bit_diff(bits, u)
        assert left == 0.0
        named = {(int(f), int(t)) for f, t in cells}
        assert named <= {(int(f), int(t)) for f, t in zip(tf[aff], tt[aff])}
        flipped += len(named)
        affected += len(aff)
        k0, k1 = u["keep"]
        got.append(PB.regate(u, raw=bits)[k0:k1] if len(named) else u["want"])
        want.append(u["want"])
    return flipped, affected, O.rel_err(np.concatenate(got), np.concatenate(want))


def _assert_separated(cell, case):
    """Targets whose frames share a sample of the recording -- within a unit or across a chunk seam -- lie >= sep bands
    apart: per channel, every pair of targets less than sep bands apart is compared."""
    n_frame = len(PB._a_window(cell, case["W"])[0])
    for ch in {g["ch"] for g in case["geo"]}:
        f = np.concatenate([case["targets"][ui][0] for ui, g in enumerate(case["geo"]) if g["ch"] == ch])
        s0 = np.concatenate([g["g0"] + case["targets"][ui][1] * case["H"] for ui, g in enumerate(case["geo"]) if g["ch"] == ch])
        order = np.argsort(f, kind="stable")
        f, s0 = f[order], s0[order]
        k = 1
        while k < len(f) and np.any(f[k:] - f[:-k] < case["sep"]):
            near = f[k:] - f[:-k] < case["sep"]
            assert not np.any(near & (np.abs(s0[k:] - s0[:-k]) < n_frame)), "channel %d" % ch
            k += 1


@pytest.mark.parametrize("cell", PB.A_CELLS, ids=PB.a_cell_id)
def test_cell_conditions(cell):
    case = PB.near_threshold_case(cell)
    n_fft = cell["n_fft"]
    F = n_fft // 2 + 1
    i16 = case["dtype"] == "int16"
    assert case["residual"] <= PB.A_TOL
    margins = np.concatenate(case["margins"])
    print("%s: %d targets in %d units, %d iterations, |margin| %.4f .. %.3f delta, %.0f %% above" % (
        cell["name"], len(margins), len(case["units"]), case["iterations"], np.abs(margins).min(), np.abs(margins).max(),
        100 * np.mean(margins > 0)))
    if i16:
        assert len(margins) >= 32 and np.any(margins > 0) and np.any(margins < 0)
    if not i16:                                        # (int16 keeps a subset of the targets placed)
        _assert_separated(cell, case)
    for ui, u in enumerate(case["units"]):
        tf, tt = case["targets"][ui]
        T = u["raw"].shape[1]
        m = PB.unit_margin(u)
        assert np.array_equal(m[tf, tt], case["margins"][ui])
        assert np.all(np.abs(m[tf, tt]) <= 0.5), "unit %d: a target is %.3f delta from its threshold" % (ui, np.abs(m[tf, tt]).max())
        # the targets' decisions are the compare of |X| itself (not of a floored dB value), and the sign of the margin
        with np.errstate(divide="ignore"):
            assert np.array_equal(u["db"][tf, tt], 20.0 * np.log10(np.abs(u["Z"][tf, tt]) + O.EPS64))
        assert np.array_equal(u["raw"][tf, tt].astype(bool), m[tf, tt] > 0)
        assert PB.nearest_margin_db(u) > 1e-7
        cells, left = PB.bit_diff(u["raw"], u)
        assert len(cells) == 0 and left == 0.0
        assert 0.01 <= np.mean(u["raw"]) <= 0.99
        if i16:
            continue
        assert min(np.mean(m[tf, tt] > 0), np.mean(m[tf, tt] < 0)) >= 0.2
        assert set(tf.tolist()) == set(range(F)), "unit %d: bands without a target" % ui
        tc = case["crowded"][ui]
        crowd = set(tf[tt == tc].tolist())
        assert crowd == set(range(0, F, case["step"])) and {0, n_fft // 4, n_fft // 2} <= crowd and len(crowd) >= 9
        # every frame position modulo the workgroup's frame count, frame 0 and the last frame; three workgroups
        hit = set(tt.tolist())
        assert {0, T - 1} <= hit
        for P in workgroup_frames(cell):
            assert T >= 3 * P, "unit of %d frames: no interior workgroup of %d frames" % (T, P)
            assert {t % P for t in hit} == set(range(P)), P
        # the edge frames read padding or the neighbour chunk: chunk_size is no multiple of the hop
        if cell["family"] != "torchgate":
            assert case["kw"]["chunk_size"] % case["H"] != 0 and 0 < case["kw"]["padding"] < case["W"] // 2


# does ``rel_err < 1e-4`` on the output see the defect?  As measured on these cells: a flipped near-threshold cell is a
# bin of ~2 x the noise's RMS magnitude, ~1e-3 of the output's peak.
OLD_BAR = {"float32": True, "band": True, "frame": True, "chunk_offset": True, "first_only": True}


@pytest.mark.parametrize("cell", PB.A_CELLS, ids=PB.a_cell_id)
def test_planted_defects(cell):
    case = PB.near_threshold_case(cell)
    rows = cell["family"] == "torchgate"
    f32 = case["dtype"] == "float32"
    n_targets = sum(len(tf) for tf, _ in case["targets"])
    for what in ("control", "float32", "band", "frame", "chunk_offset", "first_only"):
        flipped, affected, err = _report(case, _plant(case, what))
        print("%s %-12s: %4d of %5d affected targets flip (%d targets), output rel_err %.2e" % (
            cell["name"], what, flipped, affected, n_targets, err))
        if what == "control":
            assert flipped == 0 and err == 0.0
            continue
        if what == "chunk_offset" and rows:
            assert affected == 0              # a row has no chunks
            continue
        if case["dtype"] == "int16" and what == "band":
            continue                          # which targets stay within delta / 2 is left to the rounding: no band is promised
        if what in ("float32", "first_only"):
            if f32:
                assert flipped >= 1, what
        else:
            assert affected > 0 and 4 * flipped >= affected, what
        if flipped and f32:
            assert (err >= TOL) == OLD_BAR[what], "%s: rel_err %.2e" % (what, err)


@pytest.mark.parametrize("cell", [c for c in PB.A_CELLS if c["family"] != "torchgate"], ids=PB.a_cell_id)
def test_float32_window_in_the_exact_sum(cell):
    """(e): how far the defect moves the exact sums -- see the module docstring; no flip is asserted either way."""
    case = PB.near_threshold_case(cell)
    moved = []
    for ui, u in enumerate(case["units"]):
        tf, tt = case["targets"][ui]
        s = float(np.sum(O.hann_periodic(u["cfg"]["W"])))
        d = (np.abs(_spectrum_window32(u)[tf, tt]) - np.abs(u["Z"][tf, tt])) * s / PB.unit_delta(u)[tt]
        moved.append(np.abs(d))
    moved = np.concatenate(moved)
    flipped, affected, err = _report(case, _plant(case, "window32"))
    print("%s window32: sums move by %.2e (RMS) .. %.2e delta; %d of %d targets flip, rel_err %.2e" % (
        cell["name"], np.sqrt(np.mean(moved ** 2)), moved.max(), flipped, affected, err))
    assert 1e-4 < np.sqrt(np.mean(moved ** 2)) and moved.max() < 1e-2
