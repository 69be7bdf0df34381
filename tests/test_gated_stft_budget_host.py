"""The per-frame budget of TorchGate.gated_stft without a GPU (tests/gated_stft_cases.py: ``spectrum_check``,
``spec_adjoint_check``, the E / G / adjoint / R cells): the conditions every input has to meet on the oracle alone, the
defects the metrics must flag when planted in the float32 emulation -- and that they flag nothing on the emulation itself --
the adjoint identity at the new geometries, and the routing restated (``spec_route_label``) against the cells' intent.

One condition is not the one first written down for these cells.  "prop_decrease = 0.5, so the mask is >= 0.5 everywhere"
holds for the field before smoothing only: the reference smooths with zero padding beyond the field (conv2d, padding =
"same"), so a cell whose filter footprint leaves the field keeps only the weight that lies inside -- down to a quarter in
the four corners, 0.15 .. 0.2 of the final mask on these inputs.  What follows from prop_decrease, and is held here, is
mask >= 0.5 x (the filter's weight inside the field) >= 0.125: still no cell anywhere near 0, every bin of every frame is
held."""
import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import gated_stft_cases as C
from tests import parity_budget as PB

F32 = np.float32
DTYPES = ["float32", "float64"]


def test_frames_per_workgroup_are_the_kernels():
    """SPEC_Q is what csrc/spec.hip's spec_nt / spec_teams / SPEC_FPW give, and the source still states them so."""
    import os
    src = open(os.path.join(os.path.dirname(__file__), "..", "noisereduce_amd", "csrc", "spec.hip")).read()
    assert "constexpr int SPEC_FPW = 4;" in src
    assert "return N >= 2048 ? 256 : (N <= 128 ? 16 : (N == 256 ? 32 : 64));" in src
    assert "return N >= 2048 ? 1 : (spec_nt<N>() < 64 ? 256 / spec_nt<N>() : (N * sizeof(cx<float>) > 16384 ? 2 : 4));" in src
    assert C.spec_q_from_source() == C.SPEC_Q == {256: 64, 512: 32, 1024: 16, 2048: 16, 4096: 4}


def test_route_counter_surface():
    """sg_debug_counter 18: declared next to counter 17, its branch numbers named alike in the header and in _ffi."""
    import os
    import re
    from noisereduce_amd import _ffi
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "mi355gate_debug.h")).read()
    assert "which = 18" in hdr
    vals = {k: int(v, 0) for k, v in re.findall(r"#define (SG_SPEC_[A-Z0-9_]+) (0x[0-9a-fA-F]+|\d+)", hdr)}
    assert vals == {"SG_SPEC_ROW_DECIDE": 1, "SG_SPEC_T2_BITS": 2, "SG_SPEC_DECIDE": 3, "SG_SPEC_BOX_MASK": 4,
                    "SG_SPEC_NONSTAT_RAW": 5, "SG_SPEC_BITS_TO_RAW": 0x100, "SG_SPEC_MASK_DIRECT": 0x200}
    assert _ffi.SG_SPEC_NAMES == {0: "none", 1: "k_row_decide", 2: "k_t2_rows+k_decide_bits_t2", 3: "stage_decide",
                                  4: "stage_box_mask", 5: "stage_nonstat_raw"}
    assert callable(getattr(_ffi.Gate, "spectrum_route", None))


def test_cells_cover_the_edges():
    names = [c["name"] for c in C.EG_CELLS]
    assert len(set(names)) == len(names)
    for n_fft, Q in C.SPEC_Q.items():
        Ts = {c["T"] for c in C.E_CELLS if c["n_fft"] == n_fft and c["hop"] is None}
        want = {Q - 1, Q, Q + 1, 2 * Q + 1} if n_fft != 4096 else {9, 12, 13}
        assert Ts == want, (n_fft, Ts)
    assert any(c["n_fft"] == 4096 and c["H"] == 2048 and c["T"] == 5 for c in C.E_CELLS)
    assert {(c["n_fft"], c["W"], c["H"]) for c in C.G_CELLS} == {(256, 200, 37), (512, 400, 100), (1024, 1000, 333),
                                                              (1024, 1024, 512), (2048, 1500, 333), (4096, 3000, 700)}
    for c in C.EG_CELLS:
        r = c["L"] - (c["T"] - 1) * c["H"]
        assert 0 < r < c["H"] and r % 4 and c["L"] >= 2 * c["W"], c["name"]
    for c in C.G_CELLS:
        assert c["T"] == max(c["Q"] + 1, 1 + 2 * c["W"] // c["H"]), c["name"]
    assert {c["n_fft"] for c in C.ADJ_CELLS if c in C.E_CELLS} == set(C.SPEC_Q)
    assert all(c in C.ADJ_CELLS for c in C.G_CELLS)
    for c in C.ADJ_CELLS:
        assert all(0 <= t < c["T"] and 0 <= k <= c["n_fft"] // 2 for t, k in C.adj_impulses(c)), c["name"]
        assert len(set(C.adj_impulses(c))) == 6, c["name"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", C.EG_CELLS, ids=C.eg_cell_id)
def test_input_conditions_of_the_edge_and_geometry_cells(cell, dtype):
    n = cell["n_fft"]
    for b, u in enumerate(C.eg_units(cell, dtype)):
        cfg = u["cfg"]
        assert cfg["stationary"] and cfg["prop"] == C.EG_PROP and cfg["filt"] is not None
        inside = O.conv2_same_direct(np.ones(u["mask"].shape), cfg["filt"])
        assert inside.min() >= 0.25 - 1e-12
        assert np.all(u["mask"] >= C.EG_PROP * inside - 1e-12), (cell["name"], b)
        nf, nt = cfg["nf"], cfg["nt"]
        assert u["mask"][nf:-nf, nt:-nt].min() >= C.EG_PROP - 1e-12
        assert 0.05 <= u["raw"].mean() <= 0.95
        A = np.abs(u["Z"])
        med = np.median(A)
        assert (A[0] > med).sum() >= 3 and (A[n // 2] > med).sum() >= 3, (cell["name"], b)
        # the bursts do carry those bins: each stands 10 x over the median bin in two frames or more (three where the hop
        # is a quarter of the frame; at hop = n / 2 half a frame of burst reaches a third frame by its window's tail only)
        need = 3 if 4 * cell["H"] <= n else 2
        assert (A[0] > CARRY * med).sum() >= need and (A[n // 2] > CARRY * med).sum() >= need, (cell["name"], b)


CARRY = 10.0      # a frame "carries" bin 0 / n/2 where |X| there is over CARRY x the row's median bin magnitude


def _carrying(X, k):
    A = np.abs(X)
    return list(np.flatnonzero(A[k] > CARRY * np.median(A)))


def _spectrum_defects(emu, Q, n, X):
    """name -> (defective copy of the float32 gated spectrum (F, T), frames that must be flagged or None = every frame).  The
    two single-bin defects must be flagged in every frame that carries the bin (``CARRY``)."""
    T = emu.shape[1]
    out = {}
    d = emu.copy()
    d[1::2] *= 1 + 2e-5
    out["odd bins x (1 + 2e-5)"] = (d, None)
    d = emu.copy()
    d[:, -1] *= 1 + 3e-5
    out["last frame x (1 + 3e-5)"] = (d, [T - 1])
    if Q < T:
        d = emu.copy()
        d[:, Q] = d[:, Q - 1]
        out["frame Q holds frame Q - 1"] = (d, [Q])
    d = emu.copy()
    d[0] = d[0].real + 1j * 1e-4 * np.abs(d[0])
    out["Im X[0] = 1e-4 |X[0]|"] = (d, _carrying(X, 0))
    d = emu.copy()
    d[n // 2] *= 1 + 1e-4
    out["bin n/2 x (1 + 1e-4)"] = (d, _carrying(X, n // 2))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", C.EG_CELLS, ids=C.eg_cell_id)
def test_spectrum_check_flags_planted_defects_and_not_the_emulation(cell, dtype):
    n, Q = cell["n_fft"], cell["Q"]
    for b, u in enumerate(C.eg_units(cell, dtype)):
        M = u["mask"].astype(F32)            # the float mask a kernel would hand back
        emu = (u["emu_spec"] * M).astype(np.complex128)
        bad, ratio = C.spectrum_check(emu, u["Z"], M, u["cfg"], emu=u["emu_spec"])
        assert len(bad) == 0 and ratio <= 1.0, (cell["name"], b, bad, ratio)
        again, _ = C.spectrum_check(emu, u["Z"], M, u["cfg"], x=u["x"])         # the emulation from the samples
        assert len(again) == 0
        for name, (d, frames) in _spectrum_defects(emu, Q, n, u["Z"]).items():
            bad, ratio = C.spectrum_check(d, u["Z"], M, u["cfg"], emu=u["emu_spec"])
            must = range(emu.shape[1]) if frames is None else frames
            missing = sorted(set(int(t) for t in must) - set(bad.tolist()))
            assert not missing, "%s row %d %s: %s not flagged in frames %s (flagged %s, largest err / bud %.1f)" % (
                cell["name"], b, dtype, name, missing, bad.tolist(), ratio)
            if frames is not None and len(frames) == 1:
                assert bad.tolist() == list(frames), (cell["name"], name, bad.tolist())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cell", C.ADJ_CELLS, ids=C.eg_cell_id)
def test_spec_adjoint_check_flags_planted_defects_and_not_the_emulation(cell, dtype):
    G, M = C.adj_inputs(cell, dtype)
    n, T, H, L = cell["n_fft"], cell["T"], cell["H"], cell["L"]
    F = n // 2 + 1
    assert np.isnan(M[:, :, F:]).all() and np.isfinite(M[:, :, :F]).all() and M[:, :, :F].min() >= 0.25
    cfg = C.eg_units(cell, "float32")[0]["cfg"]
    for b in range(2):
        Mb = M[b, :, :F].T
        u = C.spec_adjoint_unit(G[b], Mb, cfg, L)
        assert np.isfinite(u["want"]).all() and np.isfinite(u["emu"]).all()
        bad, ratio = C.spec_adjoint_check(u["emu"], G[b], Mb, cfg, L, unit=u)
        assert len(bad) == 0 and ratio <= 1.0, (cell["name"], b, bad, ratio)
        nb = len(u["bud"])
        # a. one hop block x (1 + 3e-5): row 0 in its middle block, row 1 in the block frame 0's two cells peak in
        blk = nb // 2 if b == 0 else 0
        d = u["emu"].astype(np.float64)
        d[blk * H:(blk + 1) * H] *= 1 + 3e-5
        bad, ratio = C.spec_adjoint_check(d, G[b], Mb, cfg, L, unit=u)
        assert bad.tolist() == [blk], "%s row %d: hop block %d x (1 + 3e-5) flagged as %s (%.1f)" % (
            cell["name"], b, blk, bad.tolist(), ratio)
        # b. the last frame left out of the overlap-add of the last hop block
        d = C.emulate_spec_adjoint_f32(G[b], Mb, cfg, L, drop_last=True)
        assert np.array_equal(d[:(nb - 1) * H], u["emu"][:(nb - 1) * H])
        bad, ratio = C.spec_adjoint_check(d, G[b], Mb, cfg, L, unit=u)
        assert bad.tolist() == [nb - 1], "%s row %d: frame T - 1 dropped from the last hop block, flagged %s (%.1f)" % (
            cell["name"], b, bad.tolist(), ratio)
        # c. Im G[n/2] let through at 1e-4 -- held on row 1, whose frames 0 and T - 1 hold 1 + 1j at bin n/2 and little
        # else (in the dense row one bin's 1e-4 is within the rounding of the other 512)
        if b == 1:
            d = C.emulate_spec_adjoint_f32(G[b], Mb, cfg, L, nyquist_imag=1e-4)
            bad, ratio = C.spec_adjoint_check(d, G[b], Mb, cfg, L, unit=u)
            assert 0 in bad.tolist() and nb - 1 in bad.tolist(), "%s: Im G[n/2] at 1e-4 flagged in blocks %s (%.1f)" % (
                cell["name"], bad.tolist(), ratio)
            # ... and with the imaginary parts of bins 0 and n/2 removed the reference does not move at all
            G0 = G[b].copy()
            G0[0] = G0[0].real
            G0[-1] = G0[-1].real
            assert np.array_equal(C.spec_adjoint_unit(G0, Mb, cfg, L)["want"], u["want"])


@pytest.mark.parametrize("cell", C.G_CELLS + [c for c in C.E_CELLS if c["H"] == 2048], ids=C.eg_cell_id)
def test_model_adjoint_identity_at_the_new_geometries(cell):
    """<STFT(x) * m, g> == <x, adjoint(g)> for the real inner product to 1e-12, as tests/test_gated_stft_host.py holds it at
    the first three geometries; and the emulation's merge form is the weight-1 sum."""
    n, W, H, L = cell["n_fft"], cell["W"], cell["H"], cell["L"]
    rng = np.random.default_rng(n + H)
    x = rng.standard_normal((2, L))
    w = C.eg_window64(cell)
    X = O.stft_torch(x, n, W, H, w)
    assert X.shape[2] == cell["T"]
    m = rng.random(X.shape)
    g = rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape)
    Y = X * m
    lhs = np.sum(Y.real * g.real + Y.imag * g.imag)
    rhs = np.sum(x * C.adjoint_np(g, m, n, W, H, L, w))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    cfg = dict(n_fft=n, W=W, H=H, window=w)
    emu = np.stack([C.emulate_spec_adjoint_f32(g[b], m[b], cfg, L) for b in range(2)])
    ref = C.adjoint_np(g, m, n, W, H, L, w)
    assert np.abs(emu - ref).max() <= 1e-5 * np.abs(ref).max()


_STATIONARY_R = [c for c in C.R_CELLS if not C.r_case(c)["nonstationary"]]


@pytest.mark.parametrize("cell", _STATIONARY_R, ids=C.r_cell_id)
def test_input_conditions_of_the_stationary_route_cells(cell):
    """Every row passes 5 - 95 % of its cells and no cell lies within 1e-6 dB of its threshold."""
    for b, u in enumerate(C.r_units(cell)):
        assert u["cfg"]["prop"] == 1.0
        share = float(u["raw"].mean())
        assert 0.05 <= share <= 0.95, (cell["name"], b, share)
        assert PB.nearest_margin_db(u) > 1e-6, (cell["name"], b, PB.nearest_margin_db(u))


def test_route_cells_reach_every_branch():
    """The labels the GPU test asserts, from the predicates restated in ``spec_route_label``: every decide branch, both sides
    of the 128-frame edge with and without noise rows, both smoothing kernels behind each stationary branch, k_box_mask and
    the raw sigmoid on both sides of nt = 12, nf = 24 and n_movemean = 20."""
    labels = {}
    for c in C.R_CELLS:
        case = C.r_case(c)
        u = C.r_units(c)[0]
        T = u["mask"].shape[1]
        labels[c["name"]] = C.spec_route_label(u["cfg"], T, kbox=case["kw"].get("n_movemean_nonstationary", 20))
    spec = {k: v[0][0] for k, v in labels.items()}
    assert spec["R-t128"] == spec["R-t128-xnB"] == "k_row_decide"
    assert spec["R-t129"] == spec["R-t129-xnB"] == "k_t2_rows+k_decide_bits_t2"
    assert spec["R-1024-1024-200"] == spec["R-1024-800-200"] == "stage_decide"
    assert spec["R-tw-T-f1-t96-none"] != "stage_decide" and spec["R-tw-T-f1-t97"] == "stage_decide"
    assert spec["R-tw-T-f30-t6"] == "k_row_decide" and spec["R-tw-T-f31-t6"] == "k_row_decide"
    assert labels["R-tw-T-f30-t6"][1][0] == "k_smooth_tiled" and labels["R-tw-T-f31-t6"][1][0] == "k_smooth_f+k_smooth_t"
    assert spec["R-tw-TNS-f2-t12"] == "stage_box_mask" and spec["R-tw-TNS-f2-t13"] == "stage_nonstat_raw"
    assert spec["R-tw-TNS-f2-t20"] == "stage_nonstat_raw"
    assert spec["R-tw-TNS-f24-t9"] == "stage_box_mask" and spec["R-tw-TNS-f25-t9"] == "stage_nonstat_raw"
    assert spec["R-mm19"] == spec["R-mm21"] == "stage_nonstat_raw"
    assert set(spec.values()) == {"k_row_decide", "k_t2_rows+k_decide_bits_t2", "stage_decide", "stage_box_mask",
                                  "stage_nonstat_raw"}
    assert spec["R-ktot"] == "stage_decide" and labels["R-ktot"][1][0] == "k_smooth_tiled"


def test_no_width_leaves_the_bit_path_for_its_tile():
    """process_batch_impl also leaves the bit path where no tile of k_smooth_bits2 fits (t_sm2_ok).  No cell takes that
    exit because no width can: the bit path exists at n_fft = 1024 only (F = 513), and there the search from 64 frames
    down finds a tile for every (n_grad_freq <= 30, n_grad_time <= 96) whose ktot fits uint16 -- the 16-frame tile of
    (1, 96) takes 149984 of the 153600 bytes."""
    for nf in range(1, 31):
        for nt in range(1, 97):
            if (nf + 1) ** 2 * (nt + 1) ** 2 <= 65535:
                assert PB.sm2_tile(513, nf, nt, tt_max=64) is not None, (nf, nt)
    assert PB.sm2_tile(513, 1, 96, tt_max=64) == 16
