"""The shared 1024-term exact re-evaluation (noisereduce_amd/csrc/exact1024.hpp) through every n_fft = 1024 gate form.

Inputs: tests/parity_budget.py's near-threshold recordings ``register-1024`` (float32), ``register-1024-f64`` and
``register-1024-i16`` -- 48 hops per chunk, the smallest case that still holds three workgroups -- whose target cells lie
within delta / 2 of their thresholds on both sides, including the frames cut short by zero padding and the bins 0, 256 and
512 together in one frame.

Across gate forms: the persistent one-pass gate (SG_OPT_TILE_ORDER 0), one ticket-drawn tile per workgroup (2) and the
three-kernel route (SG_OPT_FORCE_SPLIT: k_decide_fast) call the same helper.  Their decision bits equal the oracle's on
every cell inside ``debug_range()`` and are identical across the three; a second run on the same handle repeats bits and
samples (the order in which the pending loop retires cells must not matter).

Window: the helper takes its float64 window values from the handle's table whoever supplied them.  A handle created with
the same Hann values passed explicitly decides the same bits and gives the same samples as the default handle."""
import math

import numpy as np
import pytest

from tests import parity_budget as PB
from tests.test_gpu_ambiguous_cells import _target_report
from tests.test_gpu_stagewise import _check_bits, _fetch, _make_sg, _stages

pytestmark = pytest.mark.gpu

CELLS = ["register-1024", "register-1024-f64", "register-1024-i16"]


def _forms():
    from noisereduce_amd import _ffi
    return [("tile_order_0", [(_ffi.SG_OPT_TILE_ORDER, 0)]), ("tile_order_2", [(_ffi.SG_OPT_TILE_ORDER, 2)]),
            ("force_split", [(_ffi.SG_OPT_FORCE_SPLIT, 1)])]


def _bits(gate, tag):
    b = _fetch(gate, 3)
    assert b is not None, "%s: the bit-mask stages keep the decision bits" % tag
    return b, gate.debug_range()


@pytest.mark.parametrize("name", CELLS)
def test_gate_forms_agree(name):
    case = PB.near_threshold_case(PB.a_cell(name))
    units = case["units"]
    sg = _make_sg(case)
    gate = sg._gate
    seen = {}
    gate.profile_enable(True)
    try:
        for form, opts in _forms():
            tag = "%s [%s]" % (name, form)
            with gate.lock, gate.with_options(opts):
                gate.profile_read(reset=True)
                got = sg.get_traces()
                stages = _stages(gate)
                print("%s: launched %s" % (tag, sorted(stages)))
                if form == "force_split" or case["dtype"] == "int16":
                    assert "k_decide_fast" in stages and "k_gate_onepass" not in stages, (tag, sorted(stages))
                else:
                    assert "k_gate_onepass" in stages and "k_decide_fast" not in stages, (tag, sorted(stages))
                bits, (d0, d1) = _bits(gate, tag)
                n, lines = _target_report(tag, case, bits, d0, d1)
                assert n > 0, tag
                assert not lines, "%s: target cells decided against the oracle in frames [%d, %d):\n%s" % (
                    tag, d0, d1, "\n".join(lines))
                _check_bits(tag, gate, units, False)
                got2 = sg.get_traces()
                bits2 = _bits(gate, tag)[0]
                assert np.array_equal(bits, bits2), "%s: a second run decides differently" % tag
                assert np.array_equal(got, got2), "%s: a second run gives other samples" % tag
                seen[form] = (bits, (d0, d1))
                print("%s: %d target cells in frames [%d, %d) agree with the oracle" % (tag, n, d0, d1))
    finally:
        gate.profile_enable(False)
    ref_bits, ref_range = seen["tile_order_0"]
    for form, (bits, rng) in seen.items():
        lo, hi = max(rng[0], ref_range[0]), min(rng[1], ref_range[1])
        assert lo < hi, (name, form, rng, ref_range)
        assert np.array_equal(bits[:, :, lo:hi], ref_bits[:, :, lo:hi]), \
            "%s: %s decides other bits than tile_order_0 in frames [%d, %d)" % (name, form, lo, hi)


@pytest.mark.parametrize("name", CELLS)
def test_explicit_hann_window_same_bits_and_samples(name, monkeypatch):
    """The library's own window, handed in by the caller: same table values, same decisions, same output."""
    from noisereduce_amd import _ffi
    case = PB.near_threshold_case(PB.a_cell(name))
    sg = _make_sg(case)
    with sg._gate.lock:
        want = sg.get_traces()
        want_bits, want_range = _bits(sg._gate, name)
    # the values sg_create computes for itself, through the same libm: 0.5 - 0.5 cos(2 pi k / W) in float64
    hann = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * float(k) / 1024.0) for k in range(1024)], dtype=np.float64)
    real = _ffi.cached_gate
    monkeypatch.setattr(_ffi, "cached_gate", lambda device, slot=0, **kw: real(device, slot=slot, window=hann, **kw))
    twin = _make_sg(case)
    assert twin._gate is not sg._gate, "the explicit window must get a handle of its own"
    with twin._gate.lock:
        got = twin.get_traces()
        got_bits, got_range = _bits(twin._gate, name + " [explicit window]")
    assert got_range == want_range
    assert np.array_equal(got_bits, want_bits), "%s: an explicit Hann window decides other bits" % name
    assert np.array_equal(got, want), "%s: an explicit Hann window gives other samples" % name
