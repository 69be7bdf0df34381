"""Conditions on the ORACLE alone for the tile matrix of tests/parity_budget.py (clips, rows, streams; no GPU), so that a
pass of tests/test_gpu_tile_parity.py cannot be empty: every stationary unit has a mixed mask, decides nothing inside
the ambiguity margin and has room to it; every non-stationary unit has gated and passing cells; the offline oracle is the
truth of every stationary stream (the causal floor is not engaged); and defects of the kinds the tile kernels can have --
planted in the oracle's own stages at the seams of csrc/tile_core.hpp -- are reported by ``local_check``."""
import numpy as np
import pytest

from tests import parity_budget as PB
from tests import stream_model as M

TILE_IDS = [PB.tile_cell_id(c) for c in PB.TILE_CELLS]


def test_tile_matrix_covers_every_column_in_every_path_and_size():
    cells = PB.TILE_CELLS
    assert len(cells) == 60 and len(set(TILE_IDS)) == 60
    cols = set(range(len(PB.TILE_COLUMNS)))
    for path in PB.TILE_PATHS:
        mine = [c for c in cells if c["path"] == path]
        assert {c["n_fft"] for c in mine} == set(PB.TILE_NFFT)
        assert {c["col"] for c in mine} == cols
        for n in PB.TILE_NFFT:      # T0 plus exactly one of T1..T3
            assert sorted(c["col"] for c in mine if c["n_fft"] == n)[0] == 0 and sum(c["n_fft"] == n for c in mine) == 2
    for n in PB.TILE_NFFT:
        assert {c["col"] for c in cells if c["n_fft"] == n} == cols
    T = PB.TILE_COLUMNS
    assert [c["signal"] for c in T] == ["two_level", "dc_nyquist", "bin_centred", "burst_at_seam"]
    assert [c["prop"] for c in T] == [1.0, 0.7, 1.0, 0.7] and [c["smooth"] for c in T] == ["3x2", "3x2", "off", "t9"]
    assert [c.get("dtype", "float32") for c in T] == ["float32", "float32", "float64", "float32"]
    assert [bool(c.get("short_window")) for c in T] == [False, True, False, False]


@pytest.mark.parametrize("cell", PB.TILE_CELLS, ids=TILE_IDS)
def test_tile_shapes_cross_every_seam(cell):
    case = PB.tile_case(cell)
    W, H, n_fft = case["W"], case["H"], cell["n_fft"]
    groups = PB.tile_oracle(cell)
    u0 = groups[0][0]
    c = u0["cfg"]
    assert (c["W"], c["H"]) == (W, H)
    want = {"3x2": (3, 2, True), "off": (1, 1, False), "t9": (1, 9, True)}[cell["smooth"]]
    assert (c["nf"], c["nt"], c["filt"] is not None) == want
    if cell["path"].startswith("clips"):
        cs, pad = case["kw"]["chunk_size"], case["kw"]["padding"]
        assert (cs, pad) == (24 * H + 5, 4 * H + 3)
        lens = [np.shape(y)[-1] for y in case["ys"]]
        assert lens == [2 * cs + cs // 3, cs, cs + 1, W - 3, 24 * H - 1]
        assert {np.ndim(y) for y in case["ys"]} == {1, 2}
        assert [len(g) for g in groups] == [3, 2, 2, 1, 2]
        assert lens[3] < W <= lens[3] + 2 * pad and PB.live_frames(groups[3][0])[0] > 0
        yn = case["y_noise"]
        if cell["stationary"]:
            assert isinstance(yn, np.ndarray) if cell["col"] == 0 else [v is None for v in yn] == [False, True, False, False, False]
        else:
            assert yn is None
        assert groups[0][0]["Z"].shape[1] > 32      # > 4 transform tiles and > 2 smoothing tiles per unit
    elif cell["path"].startswith("rows"):
        lens = [int(n) for n in case["lengths"]]
        L = case["x"].shape[1]
        assert L == 40 * H + 13 and lens[:3] == [L, 2 * W, 2 * W + 1] and [1 + n // H for n in lens[3:]] == [16, 17, 24, 25]
        assert min(lens) >= 2 * W and min(lens) < L
        assert all(np.isnan(case["x"][b, n:]).all() and np.isfinite(case["x"][b, :n]).all() for b, n in enumerate(lens))
        assert (case["xn"] is not None) == (cell["stationary"] and cell["col"] == 0)
        assert [g[0]["Z"].shape[1] for g in groups] == [1 + n // H for n in lens]
    else:
        N = np.shape(case["y"])[-1]
        assert N == W + 40 * H + 13 and case["C"] == len(groups[0]) and set(case["plans"]) == set(PB.STREAM_PLANS)
        assert case["plans"]["whole"] == [] and len(case["plans"]["random"]) == 7
        p = case["plans"]["prime"][0]
        assert abs(p - 1.3 * H) < 0.1 * H + 8 and all(p % d for d in range(2, p))
        assert int(case["lookahead_ms"] / (H / PB.SR * 1000)) >= case["frames"] - 1 == u0["Z"].shape[1] - 1


@pytest.mark.parametrize("cell", PB.TILE_CELLS, ids=TILE_IDS)
def test_tile_input_conditions(cell):
    """The mask of every unit is mixed (an all-pass or all-gate mask hides an error) and no decision is ambiguous."""
    groups = PB.tile_oracle(cell)
    for gi, g in enumerate(groups):
        for ui, u in enumerate(g):
            tag = "%s group %d unit %d" % (PB.tile_cell_id(cell), gi, ui)
            assert np.isfinite(u["want"]).all() and np.max(np.abs(u["want"])) > 0, tag
            raw = u["raw"]
            if u["cfg"]["stationary"]:
                share = float(np.mean(raw))
                assert 0.01 <= share <= 0.99, "%s: share of passing cells %.4f" % (tag, share)
                assert PB.nearest_margin_db(u) > 1e-6, "%s: a decision %.2e dB from its threshold" % (tag, PB.nearest_margin_db(u))
                cells, left = PB.bit_diff(u["raw"], u)
                assert len(cells) == 0 and left == 0.0 <= PB.LEFT_OUT_CAP, tag
            else:
                assert np.any(raw < 0.1) and np.any(raw > 0.9), tag


@pytest.mark.parametrize("cell", [c for c in PB.TILE_CELLS if c["path"] == "stream-S"],
                         ids=[i for i in TILE_IDS if i.startswith("stream-S")])
def test_stationary_streams_do_not_engage_the_causal_floor(cell):
    """``live is False``: no band's running maximum - 80 dB exceeds its threshold, so the streaming model IS the offline
    oracle and the oracle's units are the truth of the stream."""
    case = PB.tile_case(cell)
    units = PB.tile_oracle(cell)[0]
    for ch, u in enumerate(units):
        c = u["cfg"]
        y = np.atleast_2d(case["y"])[ch].astype(np.float64)
        outs, live = M.stream_model([y], u["thresh"], c["n_fft"], c["W"], c["H"], c["prop"], c["nf"], c["nt"], c["filt"] is not None)
        assert live is False
        assert np.max(np.abs(np.concatenate(outs) - u["want"])) <= 1e-12 * np.max(np.abs(u["want"]))


@pytest.mark.parametrize("n_fft", [256, 4096])
def test_causal_floor_cell_is_the_models_and_not_the_offline_one(n_fft):
    cf = PB.causal_floor_case(n_fft)
    u, off = cf["unit"], cf["offline"]
    c = u["cfg"]
    outs, live = M.stream_model([cf["y"].astype(np.float64)], u["thresh"], c["n_fft"], c["W"], c["H"], c["prop"], c["nf"], c["nt"],
                                c["filt"] is not None)
    assert live is True
    model = np.concatenate(outs)
    peak = np.max(np.abs(model))
    assert np.max(np.abs(model - u["want"])) <= 1e-12 * peak          # the unit restates the model
    assert np.max(np.abs(model - off["want"])) > 1e-2 * peak          # and the offline oracle is another signal
    assert 0.01 <= float(np.mean(u["raw"])) <= 0.99 and PB.nearest_margin_db(u) > 1e-6
    bad, _ = PB.local_check(off["want"], u)
    assert len(bad) > 0


# ---- planted defects -----------------------------------------------------------------------------------------------
def _target(n_fft, chunk=1):
    """Clip 0, chunk 1 of the clips-S T0 cell: loud until four hops into the kept range, quiet from there on.  (Chunk 0:
    loud throughout, and its right padding is the recording, not zeros.)"""
    cell = next(c for c in PB.TILE_CELLS if (c["path"], c["n_fft"], c["col"]) == ("clips-S", n_fft, 0))
    u = PB.tile_oracle(cell)[0][chunk]
    assert (u["ch"], u["chunk"]) == (0, chunk)
    return u


@pytest.fixture(scope="module")
def budgets():
    return {}


def _flagged(u, y, budgets):
    """local_check on the kept range of a re-gated unit: (bad blocks, ratio); the budget is computed once per unit."""
    key = u["cfg"]["n_fft"], u["chunk"]
    if key not in budgets:
        budgets[key] = PB.budget(u)
    k0, k1 = u["keep"]
    bad, ratio = PB.local_check(y[k0:k1], u, bud=budgets[key])
    return bad, ratio


def _assert_flagged(what, u, y, budgets):
    bad, ratio = _flagged(u, y, budgets)
    print("%s n_fft=%d: %d bad blocks, local_error / budget %.3g" % (what, u["cfg"]["n_fft"], len(bad), ratio))
    assert len(bad) > 0 and ratio > PB.FACTOR, (what, ratio)


@pytest.mark.parametrize("n_fft", PB.TILE_NFFT)
def test_the_target_unit_passes_as_it_is(n_fft, budgets):
    u = _target(n_fft)
    bad, ratio = _flagged(u, u["y"], budgets)
    assert len(bad) == 0 and ratio == 0.0
    k0, k1 = u["keep"]
    bad, ratio = PB.local_check(PB.emulate_f32(u)[k0:k1], u)
    assert len(bad) == 0 and ratio <= 1.0


@pytest.mark.parametrize("where", ["frame_7", "frame_8", "band_0", "band_F-1", "band_63", "band_64", "first_live_frame",
                                   "last_live_frame"])
@pytest.mark.parametrize("n_fft", PB.TILE_NFFT)
def test_one_flipped_bit_at_a_tile_seam(n_fft, where, budgets):
    """Frames 7 | 8: two transform tiles; bands 63 | 64: two ballot words; band F - 1: the lone Nyquist bit of the last
    word; band 0: its partner in the packed transform; the first / last live frame: the l0 / l1 ends of the unit."""
    u = _target(n_fft)
    F, T = u["raw"].shape
    l0, l1 = PB.live_frames(u)
    assert 0 < l0 < 7 and 8 < l1 < T - 1
    mid = (l0 + l1) // 2
    f, t = {"frame_7": (F // 3, 7), "frame_8": (F // 3, 8), "band_0": (0, mid), "band_F-1": (F - 1, mid), "band_63": (63, mid),
            "band_64": (64, mid), "first_live_frame": (F // 3, l0), "last_live_frame": (F // 3, l1)}[where]
    raw = u["raw"].copy()
    raw[f, t] = ~raw[f, t]
    _assert_flagged("flip (%d, %d)" % (f, t), u, PB.regate(u, raw=raw), budgets)


@pytest.mark.parametrize("end", ["first", "last"])
@pytest.mark.parametrize("n_fft", PB.TILE_NFFT)
def test_time_smoothing_tap_dropped_at_the_end_of_a_unit(n_fft, end, budgets):
    """The live frame at either end of the unit never reads its inner neighbour's row.  (The last frame: of chunk 0 -- in
    the quiet end of chunk 1 the neighbour's row is nearly all gated and a dropped tap drops nearly nothing.)"""
    u = _target(n_fft, 1 if end == "first" else 0)
    c = u["cfg"]
    K = c["filt"]
    ha, hb = K.shape[0] // 2, K.shape[1] // 2
    pre = u["raw"] * c["prop"] + (1.0 - c["prop"])
    l0, l1 = PB.live_frames(u)
    l1 -= 1      # (frame l1 itself reaches 8 kept samples, under a window weight of ~1e-7 at n_fft = 256: nothing to see)
    mask = u["mask"].copy()
    if end == "first":
        mask[:, l0] -= K[ha, hb + 1] * pre[:, l0 + 1]
    else:
        mask[:, l1] -= K[ha, hb - 1] * pre[:, l1 - 1]
    assert np.max(np.abs(mask - u["mask"])) > 0
    _assert_flagged("tap dropped at the %s live frame" % end, u, PB.regate(u, mask=mask), budgets)


@pytest.mark.parametrize("n_fft", PB.TILE_NFFT)
def test_nyquist_mask_taken_from_the_dc_band(n_fft, budgets):
    u = _target(n_fft)
    mask = u["mask"].copy()
    mask[-1, :] = mask[0, :]
    l0, l1 = PB.live_frames(u)
    assert np.max(np.abs(mask - u["mask"])[:, l0:l1 + 1]) > 0.01
    _assert_flagged("Nyquist mask = DC mask", u, PB.regate(u, mask=mask), budgets)


@pytest.mark.parametrize("n_fft", PB.TILE_NFFT)
def test_one_segment_left_out_of_the_overlap_add_at_a_tile_seam(n_fft, budgets):
    """One sample, at a kept position that is a multiple of 256 (the overlap-add tile), misses one frame's segment.  The
    inverse transform is linear in the masked spectrum, so "without frame t" is the unit re-gated with column t at 0."""
    u = _target(n_fft)
    c = u["cfg"]
    k0, k1 = u["keep"]
    for pos in (256, 256 * ((k1 - k0 - 1) // 256)):
        t = (k0 + pos + c["W"] // 2) // c["H"] - 1          # a frame that covers the position with weight
        mask = u["mask"].copy()
        mask[:, t] = 0.0
        y = u["y"].copy()
        y[k0 + pos] = PB.regate(u, mask=mask)[k0 + pos]
        assert np.count_nonzero(y - u["y"]) == 1
        _assert_flagged("segment of frame %d missing at kept position %d" % (t, pos), u, y, budgets)


@pytest.mark.parametrize("n_fft", PB.TILE_NFFT)
def test_last_sample_of_a_hop_divided_by_the_next_hops_envelope(n_fft):
    """Not on the clips cell: the envelope (the sum of the squared windows over the frames that cover a sample) repeats
    from hop to hop wherever every covering frame exists, and a clip's kept range starts win_length + 3 samples into its
    padded window, so in every clips unit this defect changes nothing (at win_length = 3 n_fft / 4 with an odd hop two
    neighbouring samples differ by 8.5e-9 of the envelope at n_fft = 4096: below float32).  It is planted where the
    envelope does change from sample to sample: the last whole hop of a stream (padding 0; the stream-S T0 cell's channel
    0, time-reversed), which the frames after the last one do not cover -- 2 / win_length of the envelope per sample there.  (At the
    START of a stream the missing frame's squared Hann weight at a hop's last sample is ~(pi / win_length)^4: nothing.)"""
    cell = next(c for c in PB.TILE_CELLS if (c["path"], c["n_fft"], c["col"]) == ("stream-S", n_fft, 0))
    case = PB.tile_case(cell)
    # (time-reversed, so that the end of the stream is the loud half: gated to exact zeros, a sample has no error to show)
    u = PB.oracle_units(case["y"][0][::-1].astype(np.float64), PB.SR, y_noise=case["y_noise"].astype(np.float64), **case["kw"])[1][0]
    c = u["cfg"]
    W, H = c["W"], c["H"]
    assert u["keep"][0] == 0
    w = PB.O.hann_periodic(W)
    T = u["raw"].shape[1]
    env = np.zeros(W + (T - 1) * H)
    for t in range(T):
        env[t * H:t * H + W] += w * w
    env = env[W // 2:]
    N = len(u["want"])
    pos = H * (N // H) - 1
    assert abs(env[pos + 1] / env[pos] - 1.0) > 1.0 / W
    out = u["y"].copy()
    out[pos] *= env[pos] / env[pos + 1]
    bad, ratio = PB.local_check(out[:len(u["want"])], u)
    print("envelope of the next hop n_fft=%d: bad blocks %s, local_error / budget %.3g" % (n_fft, bad.tolist(), ratio))
    assert bad.tolist() == [pos // H] and ratio > PB.FACTOR
