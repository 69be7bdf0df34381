"""The -80 dB floor of the stationary gate, band by band, against the float64 oracle: gate and noise statistics.

The inputs are tests/parity_budget.py's ``F_CELLS`` (gate) and ``S_CLIPS`` (statistics); tests/test_floor_host.py holds
on the oracle what they cover: units with no lifted band and with a few, lifted bands 0, F - 1, 63 | 64 and in the last
partial 64-band block, lifts whose only cause lies in a unit's left or right padding, and one band placed +g / -g dB
from its switch (g in [1e-5, 1e-3]).  Per cell and route, for BOTH builds of the switch pair:

* the kernels launched are the ones the route names (the stage-name rules of tests/test_gpu_stagewise.py); where the
  route has a floor pre-pass, ``k_stft_bits<max>`` ran (its stage covers the exact band maxima and the second gate
  launch for the chunks that reported; the two are not told apart by the profile);
* under SG_OPT_FLOOR_TEST 1 / 2, ``debug_counter(2)`` / ``debug_counter(1)`` count the call, and under 2
  ``debug_counter(3)`` moves: a chunk reported;
* decision bits inside ``debug_range()`` equal the oracle's (``bit_diff``); a differing (unit, band) is named with its
  switch margin;
* every unit passes ``local_check`` (float64 cell: the float64 rule; int16: equal to the truncated float64 result);
* the smoothed mask, where a float field exists, is within ``mask_bound``;
* a second run on the same handle gives the same bits and samples;
* the same recording without its content (no band lifts), gated on the same handle straight after, still gives the
  oracle's bits and output: a flag left over from the lifting call would lift there.

Statistics: the engine's threshold of every clip within 1e-9 dB of ``O.noise_threshold_S`` on every band, and a gate
call with it passes ``local_check``.

Lifted counts, switch margins and the largest local_error / budget per cell and route go to the file named by
FLOOR_PARITY_OUT, if set (profiles/floor_parity.json is that file from an MI355X run)."""
import json
import os

import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests.test_gpu_stagewise import _assert_route, _check_bits, _check_stationary_mask, _fetch, _make_sg, _stages

pytestmark = pytest.mark.gpu

_RESULTS = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_results():
    yield
    path = os.environ.get("FLOOR_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "cells": dict(sorted(_RESULTS.items()))}, f, indent=1)


def _route_opts(name):
    from noisereduce_amd import _ffi
    return {"default": [], "force_split": [(_ffi.SG_OPT_FORCE_SPLIT, 1)], "force_nofast": [(_ffi.SG_OPT_FORCE_NOFAST, 1)],
            "force_unfused": [(_ffi.SG_OPT_FORCE_UNFUSED, 1)], "floor_test_1": [(_ffi.SG_OPT_FLOOR_TEST, 1)],
            "floor_test_2": [(_ffi.SG_OPT_FLOOR_TEST, 2)]}[name]


def _bits_of(tag, gate, materialised):
    if materialised:
        raw = _fetch(gate, 0)
        assert raw is not None, "%s: the materialised kernels keep the raw mask" % tag
        return raw > 0.5, (0, raw.shape[2])
    b = _fetch(gate, 3)
    assert b is not None, "%s: the bit-mask stages keep the decision bits" % tag
    return b, gate.debug_range()


def _band_report(tag, case, bits, d0, d1):
    """Differing (unit, band) pairs with their switch margins."""
    lines = []
    for ui, u in enumerate(case["units"]):
        cells, _ = PB.bit_diff(bits[ui], u, frames=(d0, d1))
        for f in sorted({int(c[0]) for c in cells})[:8]:
            n = int(np.sum(cells[:, 0] == f))
            lines.append("unit %d (chunk %d) band %d: %d cells of frames [%d, %d) differ; switch margin %+.4e dB (%s in the "
                         "oracle)" % (ui, u["chunk"], f, n, d0, d1, case["margins"][ui][f],
                                      "lifted" if case["margins"][ui][f] > 0 else "not lifted"))
    return lines


def _check_units(tag, case, units, out, got, bud, f64):
    got = np.atleast_2d(got)
    peak = np.max(np.abs(out))
    worst = 0.0
    for ui, u in enumerate(units):
        s0, e0 = u["dst"]
        if f64:
            bad, ratio = PB.local_check(got[u["ch"], s0:e0], u, precision="float64", global_peak=peak)
        else:
            bad, ratio = PB.local_check(got[u["ch"], s0:e0], u, bud=bud[ui])
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s unit %d (chunk %d): hop blocks %s over their bound, largest error / %s %.2f" % (
            tag, ui, u["chunk"], bad[:10].tolist(), "bound" if f64 else "budget", ratio)
    return worst


GATE_CELLS = [c for c in PB.F_CELLS if not c.get("batch")]


@pytest.mark.parametrize("cell", GATE_CELLS, ids=PB.f_cell_id)
def test_gate_cell(cell):
    from noisereduce_amd import _ffi
    builds = {s: PB.floor_gate_case(cell, s) for s in (+1, -1)}
    a = builds[+1]
    i16, f64 = a["dtype"] == "int16", a["precision"] == "float64"
    plain_out, plain_units = PB.floor_plain_oracle(cell)
    plain_case = dict(a, y=a["y_plain"], units=plain_units, out=plain_out, margins=[PB.switch_margin(u) for u in plain_units])
    sgs = {s: _make_sg(c) for s, c in builds.items()}
    sg_plain = _make_sg(plain_case)
    gate = sgs[+1]._gate
    assert sgs[-1]._gate is gate and sg_plain._gate is gate, "one geometry, one handle"
    # (the stage-name rules of tests/test_gpu_stagewise.py take a cell of its own matrix)
    like = dict(family=cell["family"], n_fft=cell["n_fft"], col=1, short_window="W" in cell)
    buds = {s: None if (i16 or f64) else [PB.budget(u) for u in c["units"]] for s, c in builds.items()}
    bud_plain = None if (i16 or f64) else [PB.budget(u) for u in plain_units]
    gate.profile_enable(True)
    try:
        for route in cell["routes"]:
            for sign, case in builds.items():
                tag = "%s [%s] %+dg" % (cell["name"], route, sign)
                units = case["units"]
                sg = sgs[sign]
                lifted = [int((m > 0).sum()) for m in case["margins"]]
                with gate.lock, gate.with_options(_route_opts(route)):
                    c1, c2, e0 = gate.debug_counter(1), gate.debug_counter(2), gate.debug_counter(3)
                    gate.profile_read(reset=True)
                    got = sg.get_traces()
                    stages = _stages(gate)
                    print("%s: launched %s" % (tag, sorted(stages)))
                    assert got.dtype == np.dtype(case["dtype"])
                    rec = dict(lifted_bands_per_unit=lifted, switch_unit_band=list(case["switch"]),
                               switch_margin_db=float(case["margins"][case["switch"][0]][case["switch"][1]]))
                    _RESULTS["%s/%s/%+dg" % (cell["name"], route, sign)] = rec
                    if f64:
                        worst = _check_units(tag, case, units, case["out"], got, None, True)
                        rec["largest_local_error_over_bound"] = worst
                        assert np.array_equal(got, sg.get_traces()), "%s: a second run gives other samples" % tag
                        continue
                    floor_mode = route.startswith("floor_test")
                    if route == "force_split" and case["kw"]["prop_decrease"] != 1.0 and cell["n_fft"] == 1024:
                        # partial reduction has no lean split form at n_fft = 1024 (api.hip: `fast` needs prop_decrease = 1):
                        # decisions on the LDS transform, the K sums expanded to a float mask, then the fused apply kernel
                        assert {"k_stft_bits<decide>", "k_apply_fast"} <= stages and not (stages & {"k_gate_onepass", "k_decide_fast", "k_decide"}), (tag, sorted(stages))
                    elif a["dtype"] == "float32":
                        _assert_route(like, case, "default" if floor_mode else route, stages)
                    materialised = "k_decide" in stages
                    if not materialised:
                        # every fused route takes the band maxima of the chunks whose floor can be live in the pre-pass
                        assert "k_stft_bits<max>" in stages, (tag, sorted(stages))
                    if route == "floor_test_1":
                        assert gate.debug_counter(2) == c2 + 1 and gate.debug_counter(1) == c1, tag
                        assert "k_unit_absmax+k_prep_thresh" in stages, (tag, sorted(stages))
                    if route == "floor_test_2":
                        assert gate.debug_counter(1) == c1 + 1 and gate.debug_counter(2) == c2, tag
                        assert gate.debug_counter(3) != e0, "%s: no chunk reported, the oracle lifts %s bands" % (tag, lifted)
                    bits, (d0, d1) = _bits_of(tag, gate, materialised)
                    lines = _band_report(tag, case, bits, d0, d1)
                    rec["differing_unit_bands"] = len(lines)
                    assert not lines, "%s: decision bits differ from the oracle:\n%s" % (tag, "\n".join(lines))
                    _check_bits(tag, gate, units, materialised)
                    _check_stationary_mask(tag, gate, units, materialised, must_exist=materialised or "k_apply_istft" in stages)
                    if i16:
                        assert np.array_equal(got, np.trunc(case["out"]).astype(np.int16)), tag
                    else:
                        rec["largest_local_error_over_budget"] = _check_units(tag, case, units, case["out"], got, buds[sign], False)
                    print("%s: lifted %s, largest local_error / budget %s" % (tag, lifted, rec.get("largest_local_error_over_budget")))
                    # once more on the same handle
                    got2 = sg.get_traces()
                    assert np.array_equal(bits, _bits_of(tag, gate, materialised)[0]), "%s: a second run decides differently" % tag
                    assert np.array_equal(got, got2), "%s: a second run gives other samples" % tag
                    # no lift, straight after a lifting call
                    gotp = sg_plain.get_traces()
                    ptag = tag + " then the plain recording"
                    pbits, (p0, p1) = _bits_of(ptag, gate, materialised)
                    plines = _band_report(ptag, plain_case, pbits, p0, p1)
                    assert not plines, "%s: decision bits differ from the oracle:\n%s" % (ptag, "\n".join(plines))
                    if i16:
                        assert np.array_equal(gotp, np.trunc(plain_out).astype(np.int16)), ptag
                    else:
                        _check_units(ptag, plain_case, plain_units, plain_out, gotp, bud_plain, False)
    finally:
        gate.profile_enable(False)


def test_batch_cell():
    """``reduce_noise_batch`` (csrc/ragged.hip): three clips of different length over one noise clip, one lifting bands,
    one lifting none.  The clips kernels keep no decision bits; a band gated whole instead of lifted (or the reverse)
    fails ``local_check`` in its unit (tests/test_floor_host.py: every planted defect does)."""
    import noisereduce_amd as nr
    cell = next(c for c in PB.F_CELLS if c.get("batch"))
    case, groups = PB.floor_batch_case(cell), PB.floor_batch_oracle(cell)
    kw = dict(case["kw"])
    stationary = kw.pop("stationary")
    outs = nr.reduce_noise_batch(case["ys"], PB.SR, stationary=stationary, y_noise=case["y_noise"], **kw)
    worst = 0.0
    for i, (y, o, grp) in enumerate(zip(case["ys"], outs, groups)):
        assert o.shape == y.shape and o.dtype == y.dtype
        for u in grp:
            s0, e0 = u["dst"]
            bad, ratio = PB.local_check(o[s0:e0], u)
            worst = max(worst, ratio)
            assert len(bad) == 0, "%s clip %d chunk %d (%d lifted bands): hop blocks %s over their bound, largest error / " \
                                  "budget %.2f" % (cell["name"], i, u["chunk"], int((PB.switch_margin(u) > 0).sum()),
                                                   bad[:10].tolist(), ratio)
    _RESULTS["%s/default" % cell["name"]] = dict(
        lifted_unit_bands_per_clip=[sum(int((PB.switch_margin(u) > 0).sum()) for u in grp) for grp in groups],
        largest_local_error_over_budget=worst)
    print("%s: largest local_error / budget %.2f" % (cell["name"], worst))


@pytest.mark.parametrize("clip", PB.S_CLIPS, ids=PB.s_clip_id)
def test_statistics_clip(clip):
    nts, _ = PB.stats_clip_slices(clip)
    case = PB.floor_stats_case(clip, nts)
    n_fft, H = clip["n_fft"], case["H"]
    noise = case["y_noise"]
    # the recording that is gated: 40 hops of the clip, 20 dB up, as one chunk (chunk_size also clips the noise clip: it
    # must hold the whole clip)
    y = (10.0 * noise[len(noise) // 3 - 20 * H:len(noise) // 3 + 20 * H]).astype(np.float32)
    kw = case["kw"]
    spec = dict(y=y, y_noise=noise, kw=kw, dtype="float32", precision=None)
    gate = _make_sg(spec)._gate
    gate.profile_enable(True)
    try:
        with gate.lock:
            gate.profile_read(reset=True)
        sg = _make_sg(spec)              # (the same cached handle: its statistics run once more, profiled)
        assert sg._gate is gate
        with gate.lock:
            stages = _stages(gate)
    finally:
        gate.profile_enable(False)
    thr_engine = sg.noise_thresh
    print("%s: statistics launched %s" % (clip["name"], sorted(stages)))
    # sg_noise_stats books its kernels as ONE stage ("noise statistics (all kernels)"); it hands stage_stats one unit (the
    # channel mean), and one unit takes the single-pass k_colstats1 + k_colstats1_final pair, never k_colmax / k_colstats
    assert "noise" in stages and not (stages & {"k_colmax", "k_colstats"}), sorted(stages)
    thr, _, _ = O.noise_threshold_S(noise.astype(np.float64)[None, :], n_fft, n_fft, H, 1.5, kw["chunk_size"], True)
    d = np.abs(thr_engine - thr)
    f = int(np.argmax(d))
    print("%s: threshold within %.3g dB of the oracle's (band %d)" % (clip["name"], d[f], f))
    _RESULTS["stats/%s" % clip["name"]] = dict(slices=nts, threshold_off_db=float(d[f]))
    assert d[f] <= 1e-9, "%s: band %d off by %.3g dB" % (clip["name"], f, d[f])
    out, units = PB.oracle_units(y.astype(np.float64), PB.SR, y_noise=noise.astype(np.float64), **kw)
    assert np.max(np.abs(units[0]["thresh"] - thr)) == 0.0
    got = np.atleast_2d(sg.get_traces())
    worst = 0.0
    for ui, u in enumerate(units):
        s0, e0 = u["dst"]
        bad, ratio = PB.local_check(got[u["ch"], s0:e0], u)
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s unit %d: hop blocks %s over their bound (largest error / budget %.2f)" % (
            clip["name"], ui, bad[:10].tolist(), ratio)
    _RESULTS["stats/%s" % clip["name"]]["largest_local_error_over_budget"] = worst
