"""The width matrix of tests/parity_budget.py (``W_CELLS``) on the CPU: the conditions tests/test_gpu_smoothing_widths.py
relies on, shown with the oracle alone, and the engine's routing restated.

Stationary cells: the loud block gives a rectangle of ones at least as large as the filter (some cell of the final mask is
exactly 1.0: the full ``ktot`` is summed somewhere), the sparse block holds ones at a density of 0.02 .. 0.3, bits are set
in band 0, band F - 1, the first and the last frame of some unit, and no decision lies within 1e-6 dB of its threshold.
Non-stationary cells: the raw sigmoid has cells below 0.1 and above 0.9.  Every cell: the float32 emulation is a fair
yardstick (the assertion of tests/test_parity_budget_host.py).

Three defects are planted in the oracle's own mask (``PB.regate``) -- the taps at |dt| = nt left out, the taps at
|df| = nf left out, frames beyond the field replicated instead of zero -- and ``mask_diff`` and ``local_check`` must both
name each of them in every stationary cell that smooths."""
import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB

TOL = 1e-4
S_CELLS = [c for c in PB.W_CELLS if c["gate"] == "S"]
NS_CELLS = [c for c in PB.W_CELLS if c["gate"] == "NS"]


def test_separable_sum_is_the_direct_sum():
    rng = np.random.default_rng(5)
    m = (rng.random((37, 29)) < 0.4).astype(np.float64)
    for nf, nt in ((1, 2), (3, 1), (5, 4), (30, 6), (2, 20)):       # (the last two: wider than the field on an axis)
        want = O.conv2_same_direct(m, O.smoothing_filter(nf, nt))
        assert np.max(np.abs(PB.conv2_same_separable(m, nf, nt) - want)) < 1e-14
    ones = np.ones((9, 11))
    assert PB.conv2_same_separable(ones, 2, 3)[4, 5] == 1.0 and PB.conv2_same_separable(ones, 2, 3)[0, 0] < 1.0


@pytest.mark.parametrize("cell", S_CELLS, ids=PB.w_cell_id)
def test_stationary_cell_conditions(cell):
    out, units = PB.w_oracle(cell)
    F = cell["n_fft"] // 2 + 1
    edges = dict(band0=False, bandF=False, first=False, last=False)
    dens = []
    for u in units:
        raw = u["raw"].astype(bool)
        assert raw.shape[0] == F
        if not cell.get("small"):
            assert abs(raw.shape[1] - (2 * cell["nt"] + 70)) <= 2, raw.shape
        assert PB.bit_diff(u["raw"], u)[1] == 0.0 and PB.nearest_margin_db(u) > 1e-6, PB.nearest_margin_db(u)
        loud = PB.w_block_frames(cell, u, "loud")
        assert loud.any() and raw[:, loud].all(), "a decision inside the loud block is 0"
        assert not raw[:, PB.w_block_frames(cell, u, "quiet")].any()
        if cell.get("small"):
            assert u["mask"].max() < 1.0          # the field is smaller than the filter: no cell sums the full ktot
        else:
            assert loud.sum() >= 2 * cell["nt"] + 1 and u["mask"].max() == 1.0
        sp = PB.w_block_frames(cell, u, "sparse")
        dens.append(raw[:, sp].mean())
        edges["band0"] |= raw[0].any()
        edges["bandF"] |= raw[F - 1].any()
        edges["first"] |= raw[:, 0].any()
        edges["last"] |= raw[:, -1].any()
    assert all(edges.values()), edges
    assert all(0.02 <= d <= 0.3 for d in dens), dens


@pytest.mark.parametrize("cell", NS_CELLS, ids=PB.w_cell_id)
def test_nonstationary_cell_conditions(cell):
    out, units = PB.w_oracle(cell)
    for u in units:
        assert (u["raw"] < 0.1).any() and (u["raw"] > 0.9).any()


@pytest.mark.parametrize("cell", [c for c in PB.W_CELLS if c.get("precision") != "float64"], ids=PB.w_cell_id)
def test_emulation_is_a_fair_yardstick(cell):
    out, units = PB.w_oracle(cell)
    assert np.isfinite(out).all() and np.max(np.abs(out)) > 1e-3
    full = np.zeros(np.atleast_2d(out).shape)
    emus = [PB.emulate_f32(u) for u in units]
    for u, e in zip(units, emus):
        (k0, k1), (s0, e0) = u["keep"], u["dst"]
        full[u["ch"], s0:e0] = e[k0:k1]
        assert not len(PB.local_check(e[k0:k1], u, bud=PB.budget(u, e))[0])
    g = O.rel_err(full, np.atleast_2d(out))
    assert PB.FACTOR * g + 4 * PB.EPS32 < TOL / 3, g


DEFECTS = {"dt_taps": dict(drop_t=True), "df_taps": dict(drop_f=True), "replicate": dict(replicate=True)}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
@pytest.mark.parametrize("cell", [c for c in S_CELLS if PB.w_smooth(c)] + [c for c in PB.TW_CELLS if c["gate"] == "T"],
                         ids=PB.w_cell_id)
def test_planted_defect_is_named(cell, defect):
    units = PB.tw_oracle(cell) if cell["gate"] == "T" else PB.w_oracle(cell)[1]
    mask_hit = out_hit = False
    for u in units:
        c = u["cfg"]
        pre = u["raw"] * c["prop"] + (1.0 - c["prop"])          # (variant T's p (raw - 1) + 1 is the same number)
        bad = PB.conv2_same_separable(pre, c["nf"], c["nt"], **DEFECTS[defect])
        if np.array_equal(bad, u["mask"]):
            continue
        mask_hit |= len(PB.mask_diff(bad.astype(np.float32), u)[0]) > 0
        k0, k1 = u["keep"]
        out_hit |= len(PB.local_check(PB.regate(u, mask=bad)[k0:k1], u)[0]) > 0
    assert mask_hit, "mask_diff does not see the defect in any unit"
    assert out_hit, "local_check does not see the defect in any unit"


def test_routes_of_the_matrix():
    """The restated predicates put a cell on each side of every edge (csrc/api.hip; DESIGN.md has the table)."""
    R = {c["name"]: {r: PB.w_route(c, r) for r in c["routes"]} for c in PB.W_CELLS}
    d = lambda name, route="default": R[name][route]      # noqa: E731
    assert d("S-1024-f1-t1-none") == d("S-1024-f1-t1") == ("off", 2, 0)
    assert d("S-1024-f8-t16") == ("k_gate_onepass", 1, 16) and d("S-1024-f8-t17")[0] == d("S-1024-f9-t16")[0] == "k_smooth_bits2"
    assert d("S-512-f8-t24") == ("k_gate_onepass_reg", 1, 32) and d("S-512-f8-t25")[0] == d("S-512-f9-t24")[0] == "k_smooth_bits2"
    assert d("S-256-f8-t27")[0] == "k_gate_onepass_reg" and d("S-256-f8-t28")[0] == "k_smooth_tiled"       # ktot
    assert d("S-256-f5-t40")[0] == "k_gate_onepass_reg" and d("S-256-f5-t41")[0] == "k_smooth_bits2" and \
        d("S-256-f6-t40")[0] == "k_smooth_tiled"
    assert d("S-2048-f24-t8")[0] == "k_gate_onepass_reg" and d("S-2048-f25-t8")[0] == d("S-2048-f24-t9")[0] == "k_smooth_bits2"
    for n, tt in ((128, 256), (400, 128)):
        assert d("S-%d-f14-t3" % n) == ("k_smooth_bits2", 1, tt) and d("S-%d-f15-t3" % n) == ("k_smooth_bits2", 2, tt)
        assert d("S-%d-f30-t6" % n)[0] == "k_smooth_bits2" and d("S-%d-f31-t6" % n)[0] == "k_smooth_f+k_smooth_t"
        assert d("S-%d-f14-t16" % n)[0] == "k_smooth_bits2" and d("S-%d-f15-t15" % n)[0] == "k_smooth_tiled"
        assert d("S-%d-f1-t96-none" % n)[0] == "k_smooth_bits2" and d("S-%d-f1-t97" % n)[0] == "k_smooth_f+k_smooth_t"
    # n_fft = 4096: every tile height of the search, and none
    tiles = {c["nt"]: d(c["name"]) for c in PB.W_CELLS if c["name"].startswith("S-4096-f2-")}
    assert sorted(v[2] for v in tiles.values() if v[0] == "k_smooth_bits2") == [16, 32]
    assert [v[0] for k, v in sorted(tiles.items())][-1] == "k_smooth_tiled"
    un = lambda name: R[name]["force_unfused"][0]        # noqa: E731
    for n, get in ((601, lambda s: d(s)[0]), (1024, lambda s: un(s + "-unfused"))):
        nt_refused = max(c["nt"] for c in PB.W_CELLS if c["n_fft"] == n and c["nf"] == 30 and c["gate"] == "S" and not c.get("precision"))
        assert get("S-%d-f30-t%d" % (n, nt_refused - 1)) == "k_smooth_tiled" and get("S-%d-f30-t%d" % (n, nt_refused)) == "k_smooth_f+k_smooth_t"
        assert get("S-%d-f2-t94" % n) == "k_smooth_tiled" and get("S-%d-f2-t95" % n) == "k_smooth_f+k_smooth_t"
    for n in (1024, 400):
        got = {c["nt"]: d(c["name"])[0] for c in NS_CELLS if c["n_fft"] == n and c["nf"] == 2 and "tc" not in c}
        assert {k for k, v in got.items() if v == "k_iir_mask<nt>"} == {20, 25, 34, 37}, got
        assert d("NS-%d-f24-t9" % n)[0] == "k_iir_mask<nt>" and d("NS-%d-f25-t9" % n)[0] == "k_smooth_tiled"
        tc = next(c for c in NS_CELLS if c["n_fft"] == n and "tc" in c)
        assert d(tc["name"])[0] == "k_smooth_tiled"       # the stability bound refuses an instantiated nt
    for g in ("S", "NS"):
        x = {(c["nf"], c["nt"]): d(c["name"])[0] for c in PB.W_CELLS if c.get("precision") and c["gate"] == g and not c.get("small")}
        assert sorted(v for k, v in x.items() if k[0] == 30) == ["kx_smooth_f+kx_smooth_t", "kx_smooth_tiled"]
        assert x[(3, 95)] == x[(3, 96)] == "kx_smooth_f+kx_smooth_t"
        assert sorted(v for k, v in x.items() if k[0] == 3 and k[1] < 95) == ["kx_smooth_f+kx_smooth_t", "kx_smooth_tiled"]


# ---- TorchGate.forward cells and the moving mean -------------------------------------------------------------------
@pytest.mark.parametrize("cell", PB.TW_CELLS, ids=PB.tw_cell_id)
def test_torchgate_cell_conditions(cell):
    units = PB.tw_oracle(cell)
    case = PB.tw_case(cell)
    edges = dict(band0=False, bandF=False, first=False, last=False)
    assert all(u["raw"].shape == (513, cell["T"]) for u in units)
    for u in units:
        g = O.rel_err(PB.emulate_f32(u), u["want"])
        assert PB.FACTOR * g + 4 * PB.EPS32 < TOL / 3, g
        if cell["gate"] == "TNS":
            assert (u["raw"] < 0.1).any() and (u["raw"] > 0.9).any()
            continue
        raw = u["raw"].astype(bool)
        assert PB.bit_diff(u["raw"], u)[1] == 0.0 and PB.nearest_margin_db(u) > 1e-6, PB.nearest_margin_db(u)
        t = np.arange(cell["T"])
        a, b, _ = case["blocks"][0]
        loud = (256 * t - 512 >= a) & (256 * t + 512 <= b)          # frames whose whole window lies in the first loud block
        assert 0.01 <= raw.mean() < 0.9
        if cell.get("rowgate"):     # steady blocks (own statistics, PB.TW_CELLS): the tones' bins, every fourth
            assert loud.sum() >= 5 and raw[::4][:, loud].all(), "a decision on a tone of the steady block is 0"
        else:
            assert raw[:, loud].all(), "a decision inside the loud block is 0"
            assert loud.sum() >= 2 * cell["nt"] + 1 and u["mask"].max() == 1.0
        edges["band0"] |= raw[0].any()
        edges["bandF"] |= raw[512].any()
        edges["first"] |= raw[:, 0].any()
        edges["last"] |= raw[:, -1].any()
    assert cell["gate"] == "TNS" or all(edges.values()), edges


def test_torchgate_routes_of_the_matrix():
    R = {c["name"]: PB.tw_route(c) for c in PB.TW_CELLS}
    assert R["T-f14-t16-rowgate"] == R["T-f30-t7-rowgate"] == ("k_row_gate", 1, 64)
    assert R["T-f14-t17-rowgate"][0] == R["T-f30-t8-rowgate"][0] == "k_smooth_tiled"      # ktot > 65535: float fields
    assert R["T-f13-t17-rowgate"][0] == "k_smooth_bits2"                                    # nt > 16 alone: the bit route
    assert R["T-f2-t81"] == R["T-f2-t82"] == ("k_smooth_bits2", 1, 32)          # (the launch that once failed: both fit now)
    assert R["T-f2-t74"][2] == 64 and R["T-f2-t75"][2] == 32 and R["T-f1-t90"][1:] == (1, 32) and R["T-f1-t91"][1:] == (1, 16)
    assert R["T-f1-t96-none"][0] == "k_smooth_bits2" and R["T-f1-t97"][0] == "k_smooth_f+k_smooth_t"
    assert R["T-f30-t6"] == ("k_smooth_bits2", 2, 64) and R["T-f31-t6"] == ("k_smooth_bits", 2, 64)
    box = {n for n, r in R.items() if r[0] == "k_box_mask"}
    assert box == {"TNS-f2-t12", "TNS-f24-t9"}, box


@pytest.mark.parametrize("k", sorted({c["kbox"] for c in PB.M_CELLS}))
def test_boxcar_same_is_conv1d_same(k):
    import torch
    rng = np.random.default_rng(k)
    for T in (PB.M_T, 24, 33):
        A = rng.random((3, T))
        want = torch.nn.functional.conv1d(torch.from_numpy(A)[:, None, :], torch.ones(1, 1, k, dtype=torch.float64) / k,
                                          padding="same")[:, 0, :].numpy()
        assert np.max(np.abs(O.boxcar_same(A, k) - want)) < 1e-14


@pytest.mark.parametrize("cell", PB.M_CELLS, ids=PB.m_cell_id)
def test_movemean_cell_conditions(cell):
    units = PB.m_oracle(cell)
    frames = PB.M_LENGTHS if cell["lengths"] else (PB.M_T, PB.M_T)
    assert [u["raw"].shape[1] for u in units] == list(frames)
    for u in units:
        assert u["cfg"]["n_movemean"] == cell["kbox"]
        # A <= k S for a mean over k frames, so (A - S) / S <= k - 1: k = 1 gives the constant sigmoid(-13), k = 2 stays
        # under sigmoid(-3) = 0.047
        assert (u["raw"] < 0.1).any() and ((u["raw"] > 0.9).any() or cell["kbox"] <= 2)
        e = PB.emulate_f32(u)
        assert np.isfinite(e).all() and not len(PB.local_check(e, u, bud=PB.budget(u, e))[0])
        # the yardstick against the global 1e-4 bar, except at k = 1 and k = 3.  The kernels (and the emulation) form the
        # mask in float32 as p (m - 1) + 1, an absolute error of eps32 per cell, which the loud block turns into ~1e-7 of
        # ITS level in the output; at these two lengths the whole gated output is far below that level -- k = 1: the mask
        # is the constant sigmoid(-13) = 2.3e-6, output peak 8.7e-6, 8 g = 1.6e-2; k = 3: mask at most 0.18 in a few
        # cells, output peak 6e-4, 8 g = 6e-5 .. 1.3e-4 -- so a bar relative to the output's peak asks for more than
        # float32 has.  (k = 2: peak 2.2e-2, 8 g = 2 .. 5e-6; every longer mean: peak >= 1, 8 g <= 2e-6.)  Per hop block,
        # FACTOR x the emulation's error stays the GPU test's yardstick for these cells too.
        if cell["kbox"] not in (1, 3):
            g = O.rel_err(e, u["want"])
            assert PB.FACTOR * g + 4 * PB.EPS32 < TOL / 3, g


# ---- the same defects in the non-stationary cells --------------------------------------------------------------------
NS_ALL = NS_CELLS + [c for c in PB.TW_CELLS if c["gate"] == "TNS"]


@pytest.mark.parametrize("defect", sorted(DEFECTS))
@pytest.mark.parametrize("cell", NS_ALL, ids=PB.w_cell_id)
def test_planted_defect_is_named_nonstationary(cell, defect):
    """The final mask of the non-stationary gates is conv(raw sigmoid) (prop_decrease = 1, both variants).  The field is
    judged as the GPU test judges it -- ``_field_rule``: FACTOR x the float32 emulation's largest error over the unit's
    field + 4 eps32 -- and the output by ``local_check`` (float64 cells: ``allowed_f64``, the field by the same float32
    rule, the tighter of the two that could be asked of it)."""
    units = PB.tw_oracle(cell) if cell["gate"] == "TNS" else PB.w_oracle(cell)[1]
    f64 = cell.get("precision") == "float64"
    peak = max(np.max(np.abs(u["want"])) for u in units)
    mask_hit = out_hit = False
    for u in units:
        c = u["cfg"]
        assert c["prop"] == 1.0
        bad = PB.conv2_same_separable(u["raw"], c["nf"], c["nt"], **DEFECTS[defect])
        emu = PB.emulate_stages_f32(u)
        try:
            PB._field_rule(bad, u["mask"], emu[2], "planted")
        except AssertionError:
            mask_hit = True
        k0, k1 = u["keep"]
        y = PB.regate(u, mask=bad)[k0:k1]
        if f64:
            out_hit |= len(PB.local_check(y, u, precision="float64", global_peak=peak)[0]) > 0
        else:
            out_hit |= len(PB.local_check(y, u, bud=PB.budget(u, emu[0]))[0]) > 0
    assert mask_hit, "_field_rule does not see the defect in any unit"
    assert out_hit, "local_check does not see the defect in any unit"
