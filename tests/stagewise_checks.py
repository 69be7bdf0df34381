"""The checks of one matrix cell on the GPU (plain helper module, imported by tests/test_gpu_stagewise.py and
tests/test_gpu_smoothing_widths.py): run a gate route by route and hold it to the float64 oracle's units

a. decision bits (stationary) inside ``debug_range()`` against the oracle's ``raw``: no differing cell outside the
   ``DELTA_DB`` margin, at most ``LEFT_OUT_CAP`` of a unit's cells inside it;
b. the smoothed mask wherever a float field exists (``mask_bound``); non-stationary: final mask and raw sigmoid under
   ``_field_rule``;
c. the output of every unit per hop block within FACTOR x the float32 emulation's error there (``precision="float64"``:
   ``allowed_f64``).

Bounds and metrics are tests/parity_budget.py's; nothing here defines a tolerance."""
import numpy as np

from tests import parity_budget as PB
from tests.parity_budget import _field_rule

RATIOS = {}


def note(family, route, ratio, ratios=None):
    ratios = RATIOS if ratios is None else ratios
    key = "%s/%s" % (family, route)
    ratios[key] = max(ratios.get(key, 0.0), float(ratio))


def make_sg(case):
    from noisereduce_amd.spectralgate.nonstationary import SpectralGateNonStationary
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    kw = case["kw"]
    y = case["y"].astype(case["dtype"])
    base = dict(y=y, sr=PB.SR, prop_decrease=kw["prop_decrease"], chunk_size=kw["chunk_size"], padding=kw["padding"],
                n_fft=kw["n_fft"], win_length=kw.get("win_length"), hop_length=kw.get("hop_length"),
                time_constant_s=kw.get("time_constant_s", 2.0),
                freq_mask_smooth_hz=kw.get("freq_mask_smooth_hz", 500), time_mask_smooth_ms=kw.get("time_mask_smooth_ms", 50),
                tmp_folder=None, use_tqdm=False, n_jobs=1, precision=case["precision"])
    if kw["stationary"]:
        yn = None if case["y_noise"] is None else case["y_noise"].astype(case["dtype"])
        return SpectralGateStationary(y_noise=yn, n_std_thresh_stationary=1.5, clip_noise_stationary=True, **base)
    return SpectralGateNonStationary(thresh_n_mult_nonstationary=2, sigmoid_slope_nonstationary=10, **base)


# sg_debug_fetch refuses a field the last call's kernels did not keep with one of these messages (api.hip); any other
# error -- a size mismatch, a lost hand-off -- is an error
_NO_SUCH_FIELD = ("fetch field 3", "bit field only exists on the fused path", "lane order",
                  "does not materialise the raw mask")


def fetch(gate, what):
    """A debug field of the last call as (units, F, T), or None where the kernels that ran keep no such field."""
    try:
        return np.swapaxes(gate.debug_field(what), 1, 2)
    except RuntimeError as e:
        if any(m in str(e) for m in _NO_SUCH_FIELD):
            return None
        raise


def stages_of(gate):
    """Kernels the last call launched (first word of each profiled stage name); resets the accumulators."""
    return {k.split(" ")[0] for k in gate.profile_read(reset=True)}


def check_output(tag, family, case, got, out, units, emus, route, ratios=None):
    """c: every unit, every hop block of its kept range."""
    peak = np.max(np.abs(out))
    got = np.atleast_2d(got)
    assert got.shape == np.atleast_2d(out).shape
    f64 = case["precision"] == "float64"
    worst = 0.0
    for ui, u in enumerate(units):
        s0, e0 = u["dst"]
        if f64:
            bad, ratio = PB.local_check(got[u["ch"], s0:e0], u, precision="float64", global_peak=peak)
        else:
            bad, ratio = PB.local_check(got[u["ch"], s0:e0], u, bud=PB.budget(u, emus[ui][0]))
        worst = max(worst, ratio)
        if len(bad):
            err = PB.local_error(got[u["ch"], s0:e0], u["want"], u["cfg"]["H"])
            raise AssertionError("%s unit %d (channel %d, chunk %d): hop blocks %s of %d over their bound: error %s, largest "
                                 "error / budget in the unit %.2f" % (tag, ui, u["ch"], u["chunk"], bad[:10].tolist(), len(err),
                                                                      err[bad[:10]], ratio))
    print("%s: largest local_error / budget %.2f" % (tag, worst))
    note(family + ("_f64" if f64 else ""), route, worst, ratios)


def check_bits(tag, gate, units, materialised):
    """a: decision bits of every unit against the oracle's raw.  The bit-mask stages keep bits (field 3) for the frames
    of debug_range(); the materialised kernels keep the raw mask as floats (field 0) for every frame."""
    if materialised:
        raw = fetch(gate, 0)
        assert raw is not None, "%s: the materialised kernels keep the raw mask" % tag
        bits, (d0, d1) = raw > 0.5, (0, raw.shape[2])
    else:
        bits = fetch(gate, 3)
        assert bits is not None, "%s: the bit-mask stages keep the decision bits" % tag
        d0, d1 = gate.debug_range()
    assert bits.shape[0] == len(units), "%s: %d units in the last batch, %d in the call" % (tag, bits.shape[0], len(units))
    assert 0 <= d0 < d1 <= bits.shape[2], (tag, d0, d1)
    for ui, u in enumerate(units):
        cells, left = PB.bit_diff(bits[ui], u, frames=(d0, d1))
        assert left <= PB.LEFT_OUT_CAP
        assert len(cells) == 0, "%s unit %d: %d decision bits differ from the oracle, first (band, frame) %s of frames " \
                                "[%d, %d)" % (tag, ui, len(cells), cells[:6].tolist(), d0, d1)


def check_stationary_mask(tag, gate, units, materialised, must_exist):
    """b, stationary: the smoothed float mask where one exists.  Returns whether it did."""
    M = fetch(gate, 1)
    if M is None:
        assert not must_exist, "%s: the general apply kernels read a float mask field" % tag
        return False
    assert M.shape[0] == len(units)
    d0, d1 = (0, M.shape[2]) if materialised else gate.debug_range()
    assert 0 <= d0 < d1 <= M.shape[2], (tag, d0, d1)
    for ui, u in enumerate(units):
        # (the materialised kernels smooth a float field with float taps: parity_budget.mask_bound)
        bound = PB.mask_bound(u["cfg"], integer_taps=not materialised)
        cells, w = PB.mask_diff(M[ui], u, frames=(d0, d1), bound=bound)
        assert len(cells) == 0, "%s unit %d: smoothed mask off by up to %.3g (bound %.3g) at %d cells, first (band, frame) " \
                                "%s" % (tag, ui, w, bound, len(cells), cells[:6].tolist())
    return True


def check_nonstationary_fields(tag, gate, units, emus, raw_must_exist):
    """b, non-stationary: final mask (field 1, every route) and raw sigmoid (field 0, materialised kernels)."""
    M = fetch(gate, 1)
    assert M is not None and M.shape[0] == len(units), "%s: the non-stationary gates keep their final mask" % tag
    raw = fetch(gate, 0)
    assert (raw is not None) == raw_must_exist, "%s: raw sigmoid field %s" % (tag, "missing" if raw is None else "unexpected")
    for ui, (u, e) in enumerate(zip(units, emus)):
        _field_rule(M[ui], u["mask"], e[2], "%s unit %d final mask" % (tag, ui))
        if raw is not None:
            _field_rule(raw[ui], u["raw"], e[1], "%s unit %d raw sigmoid" % (tag, ui))


def run_cell(cell_tag, family, case, out, units, sg, routes, assert_route, raw_exists=None, ratios=None):
    """Every route of a cell: the route itself (``assert_route(route name, stages, gate)``), then checks c, a, b.
    ``raw_exists(route name, stages)``: whether a non-stationary route keeps its raw sigmoid field (default: the
    materialised kernels do, k_iir_mask<nt> does not).  Returns {route name: output}."""
    gate = sg._gate
    f64 = case["precision"] == "float64"
    emus = None if f64 else [PB.emulate_stages_f32(u) for u in units]
    stationary = case["kw"]["stationary"]
    outputs = {}
    gate.profile_enable(True)
    try:
        for name, opts in routes:
            tag = "%s [%s]" % (cell_tag, name)
            with gate.lock, gate.with_options(opts):
                gate.profile_read(reset=True)
                got = sg.get_traces()
                stages = stages_of(gate)
                assert got.dtype == np.dtype(case["dtype"])
                assert_route(name, stages, gate)
                outputs[name] = got
                check_output(tag, family, case, got, out, units, emus, name, ratios)
                if f64:
                    continue                               # the float64 pipeline keeps no debug fields
                materialised = "k_decide" in stages        # float64 transform + float raw / smoothed fields
                if stationary:
                    check_bits(tag, gate, units, materialised)
                    check_stationary_mask(tag, gate, units, materialised,
                                          must_exist=materialised or "k_apply_istft" in stages)
                else:
                    keeps_raw = "k_box_mask" in stages if raw_exists is None else raw_exists(name, stages)
                    check_nonstationary_fields(tag, gate, units, emus, raw_must_exist=keeps_raw)
    finally:
        gate.profile_enable(False)
    return outputs
