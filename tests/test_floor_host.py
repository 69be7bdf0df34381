"""The -80 dB floor cells of tests/parity_budget.py (``F_CELLS``, ``S_CLIPS``) on the CPU: conditions on the oracle alone,
so that the GPU pass of tests/test_gpu_floor.py cannot be an empty one, and planted defects in the oracle's own stages,
each of which the checks of tests/test_gpu_floor.py (``bit_diff`` / ``local_check`` on the gate, the 1e-9 dB bar on the
threshold) must report.

Gate defects (the oracle's bits with the band maxima of the floor taken wrongly):

(a) ``per_unit``     the lift applied per unit: any lifted band lifts every band;
(b) ``kept_range``   the band maximum over the frames that reach a kept sample, not over the padded chunk;
(c) ``band_pm1``     the band maximum of band f + 1 (f - 1 at the last band);
(d) ``prev_unit``    the band maximum of the previous unit (unit 0: the last one's);
(e) ``min_thresh``   the switch against min thresh instead of thresh[f];
(f) ``twin``         the -g build with its switch band lifted all the same;
(g) control: the oracle's own bits.

Statistics defects (the threshold from the oracle's power field):

(h) ``two_only``     per (slice, band) only the two smallest cells floored, a third left at its own dB;
(i) ``pivot``        a floored frame 0 left at its own dB;
(j) ``floor40``      floored at 40 dB under the band's maximum.

For each gate defect, whether ``O.rel_err < 1e-4`` on the output sees it is held as measured here (``OLD_BAR``): on
these band-selective inputs it sees (a), (c), (d), (e), and misses (b) everywhere but in the band-0 cell and (f) in the
band-0 cell.  On the suite's earlier floor inputs, where every band of a unit lifts or none, (a), (c) and (e) change no
bit at all.  For the statistics defects the threshold's distance is held (> 1e-9 dB) and the old bar printed."""
import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB

TOL = 1e-4
GATE_CELLS = [c for c in PB.F_CELLS if not c.get("batch")]


def _raw_db(u):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.abs(u["Z"]) + O.EPS64)


def _bits(u, band_max, thresh_of_switch=None):
    """Decision bits of a unit with the floor taken from ``band_max`` (F,) dB; ``thresh_of_switch``: the threshold the
    lift is switched against (default: thresh[f])."""
    db = _raw_db(u)
    th = u["thresh"]
    bits = db > th[:, None]
    sw = th if thresh_of_switch is None else thresh_of_switch
    return bits | ((band_max - 80.0) > sw)[:, None]


def plant_gate(case, what, twin=None):
    units = case["units"]
    out = []
    for ui, u in enumerate(units):
        db = _raw_db(u)
        mx = db.max(axis=1)
        if what == "control":
            bits = _bits(u, mx)
        elif what == "per_unit":
            bits = _bits(u, mx)
            if np.any(case["margins"][ui] > 0):
                bits[:] = True
        elif what == "kept_range":
            lo, hi = PB.live_frames(u)
            bits = _bits(u, db[:, lo:hi + 1].max(axis=1))
        elif what == "band_pm1":
            bits = _bits(u, np.concatenate([mx[1:], mx[-2:-1]]))
        elif what == "prev_unit":
            bits = _bits(u, _raw_db(units[ui - 1]).max(axis=1))
        elif what == "min_thresh":
            bits = _bits(u, mx, thresh_of_switch=np.full(len(mx), u["thresh"].min()))
        elif what == "twin":
            tu = twin["units"][ui]
            bits = _bits(tu, _raw_db(tu).max(axis=1))
            if ui == twin["switch"][0]:
                bits[twin["switch"][1], :] = True
        else:
            raise KeyError(what)
        out.append(bits)
    return out


def _gate_report(case, planted):
    """(units whose bits bit_diff names, units failing local_check, rel_err of the whole output)."""
    named = failed = 0
    got, want = [], []
    for u, bits in zip(case["units"], planted):
        cells, left = PB.bit_diff(bits, u)
        assert left <= PB.LEFT_OUT_CAP
        k0, k1 = u["keep"]
        g = PB.regate(u, raw=bits)[k0:k1] if len(cells) else u["want"]
        named += len(cells) > 0
        if len(cells):
            failed += len(PB.local_check(g, u)[0]) > 0
        got.append(g)
        want.append(u["want"])
    return named, failed, O.rel_err(np.concatenate(got), np.concatenate(want))


@pytest.mark.parametrize("cell", GATE_CELLS, ids=PB.f_cell_id)
def test_gate_cell_conditions(cell):
    n_fft, W, H, cs, pad, N = PB._f_geometry(cell)
    F = n_fft // 2 + 1
    a, b = PB.floor_gate_case(cell, +1), PB.floor_gate_case(cell, -1)
    su, sb = a["switch"]
    i16 = a["dtype"] == "int16"
    lo, hi = PB.F_GAIN_I16 if i16 else PB.F_GAIN
    assert lo <= a["g"] <= hi and a["g"] == b["g"]
    lifted = [m > 0 for m in a["margins"]]
    print("%s: g %.3e dB, switch (unit %d, band %d) at %+.4e / %+.4e dB after rounding, amplitudes %.8g / %.8g, lifted bands "
          "per unit %s / %s of %d" % (cell["name"], a["g"], su, sb, a["margins"][su][sb], b["margins"][su][sb], a["amplitude"],
                                      b["amplitude"], [int(v.sum()) for v in lifted], [int((m > 0).sum()) for m in b["margins"]], F))
    assert len(a["units"]) == 5 and all(u["raw"].shape[1] <= 60 for u in a["units"])
    # the switch pair: +g / -g after rounding to the dtype, >= 1e-6 dB from the switch, within 10 % of g (int16: 30 %)
    for case, sign in ((a, 1), (b, -1)):
        m = case["margins"][su][sb]
        assert np.sign(m) == sign and abs(m) >= 1e-6 and abs(abs(m) / case["g"] - 1.0) < (0.3 if i16 else 0.1), m
        for ui, mu in enumerate(case["margins"]):
            assert np.all(np.abs(mu) >= 1e-6)
            other = np.delete(mu, sb) if ui == su else mu
            assert np.min(np.abs(other)) >= 1e-3, "unit %d: a band %.3e dB from its switch" % (ui, np.min(np.abs(other)))
    # the pair differs in exactly one (unit, band)
    diff = [(ui, int(f)) for ui in range(5) for f in np.flatnonzero((a["margins"][ui] > 0) != (b["margins"][ui] > 0))]
    assert diff == [(su, sb)], diff
    # coverage: units with no lifted band and with a few; band 0, band F - 1, both sides of the 64-band seam, the last
    # partial 64-band block
    counts = [int(v.sum()) for v in lifted]
    assert 0 in counts and all(c <= 12 for c in counts) and sum(c > 0 for c in counts) >= 3, counts
    anyl = np.any(lifted, axis=0)
    assert anyl[0] and anyl[F - 1]
    if F > 66:
        assert anyl[63] and anyl[64]
    assert anyl[64 * ((F - 1) // 64):].any()
    # a unit whose lifting frames lie wholly in its right padding (unit 0), one in its left padding (unit 3); the loud
    # samples within the last / the first n_fft samples of the padded window
    for ui, side in ((0, "right"), (3, "left")):
        u = a["units"][ui]
        k0, k1 = u["keep"]
        db = _raw_db(u)
        over = (db - 80.0) > u["thresh"][:, None]
        frames = np.flatnonzero(over.any(axis=0))
        assert len(frames) and counts[ui] > 0
        s0 = frames * H - W // 2                          # first sample (of the padded window) of each such frame
        if side == "right":
            assert np.all(s0 >= k1), (ui, frames)
        else:
            assert np.all(s0 + W <= k0), (ui, frames)
        x = np.abs(u["x"])
        loud = np.flatnonzero(x > 0.5 * x.max())
        if side == "right":
            assert loud.min() >= len(x) - n_fft and loud.max() == len(x) - 1
        else:
            assert loud.min() == 0 and loud.max() < n_fft
    for case in (a, b):
        for ui, u in enumerate(case["units"]):
            cells, left = PB.bit_diff(u["raw"], u)
            assert len(cells) == 0 and left <= PB.LEFT_OUT_CAP
            if np.any(case["margins"][ui] > 0):
                assert 0.01 <= np.mean(u["raw"]) <= 0.99, (ui, np.mean(u["raw"]))
            # a lifted band passes whole, and the oracle's dB field says so
            assert np.all(u["raw"][case["margins"][ui] > 0])
    # the recording without the content lifts nothing
    _, plain = PB.floor_plain_oracle(cell)
    assert all(np.all(PB.switch_margin(u) < -1.0) for u in plain)
    assert all(len(PB.bit_diff(u["raw"], u)[0]) == 0 for u in plain)


def test_band0_cell_sits_on_the_in_kernel_bound():
    """The ``switch="dc"`` cell: band 0 holds the minimum threshold, and a constant level spans a whole frame of unit 3,
    so |X_0| = A sum(w): the in-kernel bound max|x| sum|w| itself.  Recorded: the bound's slack over the switch."""
    cells = [c for c in GATE_CELLS if c.get("switch") == "dc"]
    assert len(cells) == 1
    for sign in (1, -1):
        case = PB.floor_gate_case(cells[0], sign)
        su, sb = case["switch"]
        assert (su, sb) == (3, 0)
        u = case["units"][su]
        assert int(np.argmin(u["thresh"])) == 0
        # mag_scale = 1 / sum(w), sum|w| = sum(w): the bound is 20 log10(max|x| + eps) - 80 - min thresh
        slack = 20.0 * np.log10(np.max(np.abs(u["x"])) + O.EPS64) - 80.0 - u["thresh"].min()
        print("%s (%+d): band 0 at %+.4e dB, in-kernel bound %.4f dB over the switch" % (cells[0]["name"], sign,
                                                                                       case["margins"][su][sb], slack))
        assert case["margins"][su][sb] <= slack < 1.0
        assert slack < 0.2          # reached: 0.115 dB (the base noise's peak on top of the level)


# does ``rel_err < 1e-4`` on the whole output see the defect?  As measured on these cells: it MISSES the band maximum
# taken over the kept range (1e-6 .. 6e-6: the bands that only the padding lifts hold the base noise in the kept range,
# 1e-5 against content of 0.4), and in the band-0 cell the lifted -g twin (7e-7: one band of base noise).  There the
# kept-range defect also unlifts band 0 of unit 1, whose second level is louder: seen.
OLD_BAR = {"per_unit": True, "kept_range": False, "band_pm1": True, "prev_unit": True, "min_thresh": True, "twin": True}
OLD_BAR_DC = dict(OLD_BAR, kept_range=True, twin=False)


@pytest.mark.parametrize("cell", GATE_CELLS, ids=PB.f_cell_id)
def test_planted_gate_defects(cell):
    a, b = PB.floor_gate_case(cell, +1), PB.floor_gate_case(cell, -1)
    f64 = a["precision"] == "float64"
    for what in ("control", "per_unit", "kept_range", "band_pm1", "prev_unit", "min_thresh", "twin"):
        case = b if what == "twin" else a
        planted = plant_gate(a, what, twin=b)
        if what == "control":
            assert all(np.array_equal(p, u["raw"].astype(bool)) for p, u in zip(planted, a["units"]))
            continue
        named, failed, err = _gate_report(case, planted)
        print("%s %-10s: bit_diff names %d units, local_check fails in %d, output rel_err %.2e" % (cell["name"], what, named,
                                                                                                failed, err))
        assert named >= 1, what
        assert failed >= 1, what
        if what == "twin":
            assert named == 1
        if not f64:
            bar = OLD_BAR_DC if cell.get("switch") == "dc" else OLD_BAR
            assert (err >= TOL) == bar[what], "%s: rel_err %.2e" % (what, err)


def test_batch_cell_conditions():
    cell = next(c for c in PB.F_CELLS if c.get("batch"))
    case, groups = PB.floor_batch_case(cell), PB.floor_batch_oracle(cell)
    assert len({len(y) for y in case["ys"]}) == 3
    lifted = [sum(int((PB.switch_margin(u) > 0).sum()) for u in grp) for grp in groups]
    print("%s: clips of %s samples, %s units, lifted (unit, band) pairs %s" % (
        cell["name"], [len(y) for y in case["ys"]], [len(g) for g in groups], lifted))
    assert lifted[0] > 0 and lifted[1] == 0 and lifted[2] > 0
    for grp in groups:
        for u in grp:
            assert np.min(np.abs(PB.switch_margin(u))) >= 1e-6


# ---- statistics ----------------------------------------------------------------------------------------------------
def _clip_fields(clip):
    nts, b = PB.stats_clip_slices(clip)
    case = PB.floor_stats_case(clip, nts)
    Z = O.stft_scipy(case["y_noise"].astype(np.float64), clip["n_fft"], case["W"], case["H"])
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(np.abs(Z) + O.EPS64)
    floor = db.max(axis=1, keepdims=True) - 80.0
    return case, nts, b, db, floor, db < floor


def stats_threshold(db, floor_db, what, b):
    """mean + 1.5 std of the floored dB field, with a defect."""
    F, T = db.shape
    mx = db.max(axis=1, keepdims=True)
    if what == "floor40":
        fl = np.maximum(db, mx - 40.0)
    else:
        fl = np.maximum(db, mx - floor_db)
        if what == "pivot":
            fl[:, 0] = db[:, 0]
        elif what == "two_only":
            for s in range(len(b) - 1):
                seg = db[:, b[s]:b[s + 1]]
                order = np.argsort(seg, axis=1)
                rest = np.ones(seg.shape, dtype=bool)
                np.put_along_axis(rest, order[:, :2], False, axis=1)
                fl[:, b[s]:b[s + 1]] = np.where(rest, seg, fl[:, b[s]:b[s + 1]])
        elif what != "control":
            raise KeyError(what)
    return fl.mean(axis=1) + 1.5 * fl.std(axis=1)


@pytest.mark.parametrize("clip", PB.S_CLIPS, ids=PB.s_clip_id)
def test_stats_clip_conditions(clip):
    case, nts, b, db, floor, fl = _clip_fields(clip)
    T = db.shape[1]
    assert T == clip["frames"] and 150 <= T <= 300 and nts >= 4
    fps, smax, maxs, tg = PB.engine_stats_constants()
    assert nts == T // fps and nts <= tg * maxs          # (the single-pass route's own rule decides at these sizes)
    cnt = np.stack([fl[:, b[s]:b[s + 1]].sum(axis=1) for s in range(nts)])          # (slice, band)
    bands = np.flatnonzero(fl.any(axis=1))
    print("%s: %d frames in %d slices %s; %d bands with floored cells; (slice, band) pairs with 1 / 2 / >= 3 floored cells: "
          "%d / %d / %d; frame 0 floored in %d bands, the last frame in %d" % (
              clip["name"], T, nts, b, len(bands), (cnt == 1).sum(), (cnt == 2).sum(), (cnt >= 3).sum(), fl[:, 0].sum(),
              fl[:, -1].sum()))
    thr, _, _ = O.noise_threshold_S(case["y_noise"].astype(np.float64)[None, :], clip["n_fft"], case["W"], case["H"], 1.5,
                                    case["kw"]["chunk_size"], True)
    assert np.max(np.abs(stats_threshold(db, 80.0, "control", b) - thr)) < 1e-12
    if clip["kind"] == "plain":
        assert not fl.any()
        return
    if clip["kind"] == "runs":
        # every band: a slice with exactly one floored frame, one with two, one with >= 3; frame 0 and frame T - 1
        # floored; a floored pair on both sides of a slice boundary
        assert len(bands) == db.shape[0]
        for f in (0, db.shape[0] // 2, db.shape[0] - 1):
            assert 1 in cnt[:, f] and 2 in cnt[:, f] and np.any(cnt[:, f] >= 3)
        assert fl[:, 0].all() and fl[:, -1].all()
        assert any(fl[:, b[s] - 1].all() and fl[:, b[s]].all() for s in range(1, nts))
        assert {m for _, m in case["runs"]} == {1, 2, 3, 5}
        zero = np.flatnonzero(fl.all(axis=0))
        assert len(zero) == sum(m for _, m in case["runs"])
    else:
        # flooring in a few bands of a 64-lane block only: the tone's main-lobe bands, roughly half of their cells
        k = clip["bin"]
        assert len(bands) <= 6 and np.all(np.abs(bands - k) <= 2.5), bands
        assert np.any(cnt >= 3) and 0.25 <= fl[int(k)].mean() <= 0.6
        if k != int(k):
            assert {63, 64} <= set(bands.tolist())       # both sides of the block seam
        else:
            assert bands.min() // 64 == bands.max() // 64 and 8 < k % 64 < 56


@pytest.mark.parametrize("clip", [c for c in PB.S_CLIPS if c["kind"] != "plain"], ids=PB.s_clip_id)
def test_planted_statistics_defects(clip):
    case, nts, b, db, floor, fl = _clip_fields(clip)
    good = stats_threshold(db, 80.0, "control", b)
    # what the old bar makes of it: 60 hops of the clip, 20 dB up, gated with either threshold
    H = case["H"]
    y = case["y_noise"].astype(np.float64)
    y = 10.0 * (y[len(y) // 3 - 30 * H:len(y) // 3 + 30 * H] if clip["kind"] == "tone" else y[:60 * H])
    kw = dict(case["kw"], chunk_size=None)
    _, units = PB.oracle_units(y, PB.SR, y_noise=case["y_noise"].astype(np.float64), **kw)
    u = units[0]
    assert np.max(np.abs(u["thresh"] - good)) < 1e-12
    seen = {}
    for what in ("two_only", "pivot", "floor40"):
        if what == "pivot" and not fl[:, 0].any():
            continue
        if what == "two_only" and not np.any(np.stack([fl[:, b[s]:b[s + 1]].sum(axis=1) for s in range(nts)]) >= 3):
            continue
        bad = stats_threshold(db, 80.0, what, b)
        d = np.max(np.abs(bad - good))
        bits = PB.amp_db_bits(u, bad)
        err = O.rel_err(PB.regate(u, raw=bits)[u["keep"][0]:u["keep"][1]], u["want"]) if np.any(bits != u["raw"]) else 0.0
        print("%s %-8s: threshold off by %.3g dB, gated output rel_err %.2e" % (clip["name"], what, d, err))
        assert d > 1e-9, what
        seen[what] = bool(err >= TOL)
    # the old bar on a gated output (printed above, not held: it depends on the recording that is gated); the statistics
    # already had a 1e-9 dB bar of their own -- what was missing are inputs that reach these branches
    print("%s: rel_err >= 1e-4 on the gated stretch: %s" % (clip["name"], seen))
