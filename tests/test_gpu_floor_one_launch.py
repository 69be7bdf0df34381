"""The floor fix-up of the n_fft = 1024 one-pass gate as ONE launch (noisereduce_amd/csrc/onepass.hpp: k_floor_fix -- the
float64 band maxima of the chunks whose in-kernel floor test fired and their second gate pass, with a per-chunk arrival word
between the two roles) against the two launches it replaces (SG_OPT_FLOOR_TWO_LAUNCH: k_stft_bits<max>, then the gate's REDO
instantiation) and against the float64 oracle.

Shapes: n_fft 1024, hop 256, SG_OPT_FLOOR_TEST 2, chunk_size 4096 and 8192 at padding 512 -- 2 and 3 tiles per unit plus the two
halo tiles, as in tests/test_gpu_onepass_plan.py -- over 5 units per channel (four whole chunks and a remainder).  The recordings
follow the lifting recordings of tests/parity_budget.py (``floor_gate_case``, whose own geometry is fixed at chunk_size
37 H + 11): white noise 10 dB under a white noise clip, and in the units that are to report a tone 84 dB over the clip's level in
the middle of the chunk, where no other unit's padded window holds it: its bands are lifted whole by the -80 dB floor (the
oracle's decision bits say so), and the in-kernel floor test fires in exactly that unit.  ``floor_gate_case``'s own
register-1024 recording runs too.

Per case: output samples and decision bits (field 3 inside ``debug_range()``) of the one launch are bit-equal to the two
launches on the same handle; ``debug_counter(20)`` names the form; decision bits equal the oracle's and every unit passes
``PB.local_check``.  The lose hook (SG_OPT_INJECT_HANDOFF_FAULT bit 6: the wait for a chunk's maxima gives up at once) makes the
call report SG_E_HANDOFF, and the next call on the handle is right.

n_fft = 256 / 512 / 2048 keep the two launches (their REDO bodies take another argument struct): the counter says so."""
import functools

import numpy as np
import pytest
import torch

from tests import parity_budget as PB
from tests import stagewise_checks as SC

pytestmark = pytest.mark.gpu

PAD, REM = 512, 700
ONE, TWO = 1, 2   # SG_FLOOR_ONE_LAUNCH, SG_FLOOR_TWO_LAUNCH (include/mi355gate_debug.h)

# case -> per channel, the units that hold a tone ("t") or a NaN sample ("n")
CASES = {
    "none": [{}],
    "one-interior": [{2: "t"}],
    "first-and-last": [{0: "t", 4: "t"}],
    "every-unit": [{k: "t" for k in range(5)}],
    "two-channels": [{1: "t"}, {3: "t", 4: "t"}],
    "nonfinite-next-to-reported": [{1: "n", 2: "t"}],
}


def _kw(cs, n_fft=1024):
    return dict(stationary=True, n_fft=n_fft, chunk_size=cs, padding=PAD, prop_decrease=1.0)


@functools.lru_cache(maxsize=None)
def _recording(name, cs):
    """(y, y_noise) float32: y (N,) or (C, N)."""
    plan = CASES[name]
    N = 4 * cs + REM
    rng = np.random.default_rng(7300 + 13 * sorted(CASES).index(name) + cs)
    noise = (3e-5 * np.random.default_rng(7299).standard_normal(40 * 256)).astype(np.float32)   # (one clip: the handle keeps one threshold)
    y = 1e-5 * rng.standard_normal((len(plan), N))
    i = np.arange(N, dtype=np.float64)
    for c, units in enumerate(plan):
        for k, what in units.items():
            # the middle of chunk k; the remainder chunk's content lies past unit 3's right padding
            a, b = (k * cs + cs // 2 - 512, k * cs + cs // 2 + 512) if k < 4 else (4 * cs + PAD + 8, 4 * cs + REM - 10)
            if what == "t":
                y[c, a:b] += 0.5 * np.sin(2 * np.pi * (128 + 7 * c) * (i[a:b] - a) / 1024.0)
            else:
                y[c, (a + b) // 2] = np.nan
    y = y.astype(np.float32)
    return (y[0] if len(plan) == 1 else y), noise


@functools.lru_cache(maxsize=None)
def _oracle(name, cs):
    """(out, units) of the recording with a NaN sample read as 0: only the unit that holds it differs (no other unit's padded
    window reaches it), and that unit is not compared."""
    y, noise = _recording(name, cs)
    return PB.oracle_units(np.nan_to_num(y.astype(np.float64)), PB.SR, y_noise=noise.astype(np.float64), **_kw(cs))


def _case(y, noise, kw):
    return dict(y=y, y_noise=noise, kw=kw, dtype="float32", precision=None)


def _gate_call(sg, two):
    """One get_traces on SG_OPT_FLOOR_TEST 2: (samples, decision bits, debug_range, floor_route, reported?)."""
    from noisereduce_amd import _ffi
    g = sg._gate
    with g.lock, g.with_options([(_ffi.SG_OPT_FLOOR_TEST, 2), (_ffi.SG_OPT_FLOOR_TWO_LAUNCH, int(two))]):
        e0 = g.debug_counter(3)
        got = np.array(sg.get_traces())
        route = g.debug_counter(20)
        bits = SC.fetch(g, 3)
        d0, d1 = g.debug_range()
        reported = g.debug_counter(3) != e0
    assert bits is not None
    bits = bits.copy()
    bits[:, :, :d0] = 0   # (frames outside debug_range were not decided)
    bits[:, :, d1:] = 0
    return got, bits, (d0, d1), route, reported


def _same(a, b):
    """Bit-equal (a NaN equals the same NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_oracle(tag, got, bits, rng, units, skip=()):
    got = np.atleast_2d(got)
    for ui, u in enumerate(units):
        if ui in skip:   # (a unit with a NaN sample: no float64 result to bound)
            continue
        cells, _ = PB.bit_diff(bits[ui], u, frames=rng)
        assert len(cells) == 0, "%s unit %d: %d decision bits differ from the oracle, bands %s" % (
            tag, ui, len(cells), sorted({int(c[0]) for c in cells})[:8])
        s0, e0 = u["dst"]
        bad, ratio = PB.local_check(got[u["ch"], s0:e0], u)
        assert len(bad) == 0, "%s unit %d: hop blocks %s over their bound, largest error / budget %.2f" % (tag, ui, bad[:10].tolist(), ratio)


@pytest.mark.parametrize("cs", [4096, 8192])
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_launch_equals_two_launches_and_the_oracle(name, cs):
    y, noise = _recording(name, cs)
    sg = SC.make_sg(_case(y, noise, _kw(cs)))
    one = _gate_call(sg, False)
    two = _gate_call(sg, True)
    tag = "%s cs %d" % (name, cs)
    print("%s: reported %s / %s, form %d / %d" % (tag, one[4], two[4], one[3], two[3]))
    assert one[3] == ONE and two[3] == TWO, (tag, one[3], two[3])
    assert one[4] == two[4] == (name != "none"), "%s: the floor test fired in %s / %s" % (tag, one[4], two[4])
    assert one[2] == two[2]
    assert _same(one[1], two[1]), "%s: decision bits of one launch differ from two launches" % tag
    assert _same(one[0], two[0]), "%s: samples of one launch differ from two launches" % tag
    sg._gate.check_errors()
    _, units = _oracle(name, cs)
    plan = [units_c.get(k) for units_c in CASES[name] for k in range(5)]
    nan_units = [ui for ui, w in enumerate(plan) if w == "n"]
    if nan_units:   # no cell of such a unit passes: its kept samples are gated to zero or NaN, never let through
        s0, e0 = units[nan_units[0]]["dst"]
        kept = one[0][s0:e0]
        assert np.all(np.isnan(kept) | (kept == 0)), tag
    lifted = [int((PB.switch_margin(u) > 0).sum()) if ui not in nan_units else -1 for ui, u in enumerate(units)]
    print("%s: lifted bands per unit %s" % (tag, lifted))
    assert [n > 0 for n in lifted] == [w == "t" for w in plan], (tag, lifted)
    _check_oracle(tag, one[0], one[1], one[2], units, skip=nan_units)
    # a second run on the handle gives the same
    again = _gate_call(sg, False)
    assert _same(again[0], one[0]) and _same(again[1], one[1]), "%s: a second run differs" % tag


@pytest.mark.parametrize("cs", [4096, 8192])
def test_plain_call_straight_after_a_lifting_one(cs):
    """A flag, an arrival word or band maxima left over from the lifting call would lift here."""
    y, noise = _recording("every-unit", cs)
    yp, _ = _recording("none", cs)
    lifting, plain = SC.make_sg(_case(y, noise, _kw(cs))), SC.make_sg(_case(yp, noise, _kw(cs)))
    assert lifting._gate is plain._gate, "one geometry, one handle"
    a = _gate_call(lifting, False)
    assert a[4] and a[3] == ONE
    b = _gate_call(plain, False)
    assert not b[4] and b[3] == ONE
    _, units = _oracle("none", cs)
    _check_oracle("plain after every-unit, cs %d" % cs, b[0], b[1], b[2], units)
    assert _same(_gate_call(plain, True)[0], b[0])


def test_the_register_1024_floor_cell():
    """``floor_gate_case``'s own lifting recording (chunk_size 37 H + 11, padding 9 H + 5: lifts whose only cause lies in a unit's
    left or right padding, a band a hair over its switch)."""
    cell = PB.f_cell("register-1024")
    for sign in (+1, -1):
        case = PB.floor_gate_case(cell, sign)
        sg = SC.make_sg(case)
        one, two = _gate_call(sg, False), _gate_call(sg, True)
        assert one[3] == ONE and two[3] == TWO and one[4] and two[4]
        assert _same(one[1], two[1]) and _same(one[0], two[0]), sign
        _check_oracle("register-1024 %+dg" % sign, one[0], one[1], one[2], case["units"])


def test_a_wait_that_gives_up_is_reported_and_the_next_call_is_right():
    from noisereduce_amd import _ffi
    cs = 4096
    y, noise = _recording("one-interior", cs)
    sg = SC.make_sg(_case(y, noise, _kw(cs)))
    good = _gate_call(sg, False)
    yd = torch.from_numpy(y).to("cuda:0")
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    dev = SpectralGateStationary(y=yd, sr=PB.SR, y_noise=torch.from_numpy(noise).to("cuda:0"), n_std_thresh_stationary=1.5,
                                 clip_noise_stationary=True, prop_decrease=1.0, chunk_size=cs, padding=PAD, n_fft=1024,
                                 win_length=None, hop_length=None, time_constant_s=2.0, freq_mask_smooth_hz=500,
                                 time_mask_smooth_ms=50, tmp_folder=None, use_tqdm=False, n_jobs=1)
    g = dev._gate
    assert g is sg._gate, "one geometry, one handle"
    with g.lock, g.with_options([(_ffi.SG_OPT_FLOOR_TEST, 2)]):
        assert _same(dev.get_traces().cpu().numpy(), good[0])
        g.check_errors()
        g.set_option(_ffi.SG_OPT_INJECT_HANDOFF_FAULT, 64)
        bad = dev.get_traces().clone()
        torch.cuda.synchronize()
        assert g.debug_counter(20) == ONE
        with pytest.raises(_ffi.HandoffTimeout):
            g.check_errors()
        g.check_errors()
        # the reported unit's tiles could not know its maxima: NaN, never a plausible value; the other units are untouched
        bad = bad.cpu().numpy()
        assert np.isnan(bad[2 * cs:3 * cs]).any()
        keep = np.ones(len(bad), bool)
        keep[2 * cs - 1024:3 * cs + 1024] = False
        assert _same(bad[keep], good[0][keep])
        assert _same(dev.get_traces().cpu().numpy(), good[0])
        g.check_errors()


@pytest.mark.parametrize("n_fft", [256, 512, 2048])
def test_the_other_geometries_keep_two_launches(n_fft):
    cs = 16 * n_fft
    rng = np.random.default_rng(n_fft)
    noise = (3e-5 * rng.standard_normal(40 * n_fft // 4)).astype(np.float32)
    y = (1e-5 * rng.standard_normal(4 * cs + REM)).astype(np.float32)
    y[2 * cs + cs // 2:2 * cs + cs // 2 + n_fft] += 0.5
    sg = SC.make_sg(_case(y, noise, dict(_kw(cs, n_fft), padding=2 * n_fft)))
    got, _, _, route, reported = _gate_call(sg, False)
    assert route == TWO and reported
    assert _same(got, _gate_call(sg, True)[0])
