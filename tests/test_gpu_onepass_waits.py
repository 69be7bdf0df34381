"""The persistent n_fft = 1024 gate after its compiler-inserted vmcnt(0) waits left the per-tile chain (onepass.hpp: the
mid-tile ticket draw as a global returning atomic waited for at the hand-over, the tile_fast epilogue's global stores and
partial wait for 1 / envelope, the smoothing stage's MFMA operands from LDS, the next tile's samples loaded without a branch).

What runs here is the hand-over of a ticket that arrives late and the open seam's loads waited for at seam_finish, not the
benchmark's shape: recordings long enough that every workgroup loops over several tickets, crosses units and halo tiles and
closes an open seam when it leaves.  Every call is held to the one-tile form (SG_OPT_TILE_ORDER 2: immediate hand-off, the
ticket drawn at the start) bit for bit and to the oracle within the bound of tests/test_gpu_onepass_chain.py; the error word
must be clean; every call runs twice (the second pass closes its seams over warm buffers)."""
import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests.test_gpu_onepass_chain import HEAD, TOL, _oracle_head, _signal

pytestmark = pytest.mark.gpu

KW = dict(sr=48000, n_std_thresh_stationary=1.5, clip_noise_stationary=True, n_fft=1024, win_length=None, hop_length=None,
          time_constant_s=2.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50, tmp_folder=None, use_tqdm=False, n_jobs=1)


def _both_forms(sg, opts=()):
    """(persistent, persistent again, one tile per workgroup) of one object; the error word read after every call."""
    from noisereduce_amd import _ffi
    gate = sg._gate
    assert gate.get_option(_ffi.SG_OPT_TILE_ORDER) == 0
    with gate.lock, gate.with_options(list(opts)):
        with gate.with_options([(_ffi.SG_OPT_TILE_ORDER, 2)]):
            b = sg.get_traces()
            gate.check_errors()
        a = sg.get_traces()
        gate.check_errors()
        a2 = sg.get_traces()
        gate.check_errors()
    diff = np.flatnonzero((np.atleast_2d(a) != np.atleast_2d(b)).any(axis=0))
    assert np.array_equal(a, b, equal_nan=True), "persistent and one-tile outputs differ at %d samples, first %s" % (len(diff), diff[:8])
    assert np.array_equal(a, a2, equal_nan=True), "a second persistent run gives other samples"
    return a


# (channels, samples, chunk_size, padding, prop_decrease): the first is 2 880 tickets on 768 workgroups -- 9.6 M samples, 15
# tickets per unit, two of them halo tiles; the second runs the PROP instantiation over rows that mix both epilogues
@pytest.mark.parametrize("C,n,cs,pad,prop", [(2, 4800000, 50000, 6000, 1.0), (3, 2880123, 100000, 5000, 0.8)],
                         ids=["float32-2880-tickets", "prop-0.8"])
def test_float32_persistent_equals_one_tile_and_oracle(C, n, cs, pad, prop):
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    y = _signal(C, n)
    sg = SpectralGateStationary(y=y, y_noise=None, prop_decrease=prop, chunk_size=cs, padding=pad, **KW)
    a = _both_forms(sg)
    assert np.isfinite(a).all()
    err = O.rel_err(a[:, :HEAD], _oracle_head(y, cs, pad, prop))
    print("C %d n %d prop %.1f: rel err of the first %d samples %.3e" % (C, n, prop, HEAD, err))
    assert err < TOL, err


def test_int16_recording_of_a_few_chunks():
    """An integer recording: the exact re-evaluation reads the caller's samples in their own type."""
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    n, cs, pad = 700001, 200000, 10000
    y = np.round(O.synth_signal(n, seed=311, tone_hz=750.0).astype(np.float64) * 20000).astype(np.int16)
    sg = SpectralGateStationary(y=y, y_noise=None, prop_decrease=1.0, chunk_size=cs, padding=pad, **KW)
    a = np.asarray(_both_forms(sg))
    want = O.reduce_noise_S(y.astype(np.float64)[None, :], 48000, stationary=True, chunk_size=cs, padding=pad, prop_decrease=1.0)
    got = a.reshape(want.shape)
    if np.issubdtype(got.dtype, np.integer):
        # the truncated float64 oracle, as tests/test_gpu_fuzz.py holds integer recordings: equal wherever the float64 value
        # is not within 1e-9 of an integer, within one count there
        diff = got.astype(np.int64) - want.astype(np.int16).astype(np.int64)
        decided = np.abs(want - np.round(want)) > 1e-9
        print("int16: %d samples differ, %d of them decided ones" % (np.count_nonzero(diff), np.count_nonzero(diff[decided])))
        assert np.max(np.abs(diff)) <= 1 and np.count_nonzero(diff[decided]) == 0
    else:
        err = O.rel_err(got.astype(np.float64), want)
        print("int16: rel err %.3e" % err)
        assert err < TOL, err


@pytest.mark.parametrize("prop", [1.0, 0.8])
def test_a_unit_that_reports_its_floor_test_runs_the_redo_launch(prop):
    """SG_OPT_FLOOR_TEST 2: the first launch tests the floor itself, the chunks that report are gated again (REDO)."""
    from noisereduce_amd import _ffi
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    from tests.test_gpu_onepass import _floor_inputs
    y, y_noise, cs, pad = _floor_inputs("live")
    sg = SpectralGateStationary(y=y, y_noise=y_noise, prop_decrease=prop, chunk_size=cs, padding=pad, **KW)
    gate = sg._gate
    e0 = gate.debug_counter(3)
    a = _both_forms(sg, [(_ffi.SG_OPT_FLOOR_TEST, 2)])
    assert gate.debug_counter(3) != e0, "no chunk reported its floor test: the REDO launch had nothing to do"
    want = O.reduce_noise_S(y.astype(np.float64), 48000, stationary=True, y_noise=y_noise.astype(np.float64),
                            prop_decrease=prop, chunk_size=cs, padding=pad)
    err = O.rel_err(a, want)
    print("floor live, prop %.1f: rel err %.3e" % (prop, err))
    assert err < TOL, err
