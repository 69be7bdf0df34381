"""The per-tile chain of the persistent n_fft = 1024 gate (k_gate_onepass<..., PERSIST>): the seam between abutting tiles
finished one tile late, and the exact re-evaluation of near-threshold cells.

Deferred seam.  An interior tile of the persistent kernel leaves its three leading partial hops open and finishes them in
the workgroup's next iteration (onepass.hpp, "DEFERRED SEAM"); an open seam is closed on the spot before the workgroup
leaves, in a halo tile and before a tile that takes the general epilogue.  The one-tile kernel (SG_OPT_TILE_ORDER 2) keeps
the immediate hand-off, and the sums are the same in the same order: the outputs must be equal bit for bit.  The shapes
make every workgroup loop over several tickets (more than 2 x 768), cross units and halo tiles, mix rows that take the
general epilogue with rows that do not, and end workgroups on their first tile.

Exact cells.  tests/parity_budget.py's near-threshold recording for the register path at n_fft = 1024 (built as
tests/test_gpu_ambiguous_cells.py builds it): the mask bits of the persistent kernel equal the oracle's and its output
equals the one-tile kernel's."""
import functools
import math

import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests.test_gpu_stagewise import _check_bits, _make_sg

pytestmark = pytest.mark.gpu

TOL = 1e-4          # BASELINE.json north_star: output within 1e-4 (relative to peak) of the CPU reference
HEAD = 300000       # samples compared with the oracle

# (channels, samples, chunk_size, padding)
SHAPES = [
    (2, 4800000, 50000, 6000),       # 2 880 tickets: 15 per unit, two of them halo tiles
    (1, 8640000, 600000, 30000),     # long interior runs
    (3, 2880123, 100000, 5000),      # odd row length: two of the three rows unaligned -> general epilogue; tickets that
                                     # cross a row boundary mix deferred and immediate tiles in one workgroup
    (1, 20000, 600000, 30000),       # fewer tiles than the grid: a workgroup's first tile is its last
]


@functools.lru_cache(maxsize=None)
def _signal(C, n):
    y = np.stack([O.synth_signal(n, seed=211 + c, tone_hz=600.0 + 350 * c) for c in range(C)]).astype(np.float32)
    return y


def _oracle_head(y, cs, pad, prop):
    """The oracle's first HEAD samples.  The threshold reads the first chunk_size samples of the channel mean and a chunk
    reads its own window: a prefix that holds every chunk window that reaches into the head gives the same samples."""
    n = y.shape[1]
    k = math.ceil(min(HEAD, n) / cs)
    n_pref = min(n, max(k * cs + pad, cs))
    want = O.reduce_noise_S(y[:, :n_pref].astype(np.float64), 48000, stationary=True, chunk_size=cs, padding=pad,
                            prop_decrease=prop)
    return want[:, :HEAD]


@pytest.mark.parametrize("prop", [1.0, 0.8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d-n%d-cs%d-pad%d" % s)
def test_deferred_seam_equals_immediate_handoff(shape, prop):
    from noisereduce_amd import _ffi
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    C, n, cs, pad = shape
    y = _signal(C, n)
    sg = SpectralGateStationary(y=y, sr=48000, y_noise=None, prop_decrease=prop, n_std_thresh_stationary=1.5,
                                chunk_size=cs, clip_noise_stationary=True, padding=pad, n_fft=1024, win_length=None,
                                hop_length=None, time_constant_s=2.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50,
                                tmp_folder=None, use_tqdm=False, n_jobs=1)
    gate = sg._gate
    assert gate.get_option(_ffi.SG_OPT_TILE_ORDER) == 0
    try:
        gate.set_option(_ffi.SG_OPT_TILE_ORDER, 2)
        b = sg.get_traces()                 # one ticket-drawn tile per workgroup: immediate hand-off
    finally:
        gate.set_option(_ffi.SG_OPT_TILE_ORDER, 0)
    a = sg.get_traces()                     # persistent workgroups: deferred seam
    a2 = sg.get_traces()
    gate.check_errors()
    assert np.isfinite(a).all()
    diff = np.flatnonzero((a != b).any(axis=0))
    assert np.array_equal(a, b), "persistent and one-tile outputs differ at %d samples, first %s" % (len(diff), diff[:8])
    assert np.array_equal(a, a2), "a second persistent run gives other samples"
    err = O.rel_err(a[:, :HEAD], _oracle_head(y, cs, pad, prop))
    print("shape %s prop %.1f: rel err of the first %d samples %.3e" % (shape, prop, HEAD, err))
    assert err < TOL, err


def test_exact_cells_persistent_equals_oracle_bits_and_one_tile_output():
    from noisereduce_amd import _ffi
    case = PB.near_threshold_case(PB.a_cell("register-1024"))
    units = case["units"]
    T = units[0]["raw"].shape[1]
    # what the recording must hold for this test to mean anything
    many = two_frames = nyquist = first = last = False
    for tf, tt in case["targets"]:
        cnt = np.bincount(tt, minlength=T)
        many |= bool(cnt.max() >= 3)                                       # several cells in one frame
        hit = cnt > 0
        # (a wave holds four consecutive frames of a 16-frame tile; any window of four frames with two hit frames will do)
        two_frames |= bool((np.convolve(hit.astype(int), np.ones(4, int), "valid") >= 2).any())
        nyquist |= bool((tf == 512).any())
        first |= bool(hit[0])
        last |= bool(hit[T - 1])
    assert many and two_frames and nyquist and first and last, (many, two_frames, nyquist, first, last)
    sg = _make_sg(case)
    gate = sg._gate
    gate.profile_enable(True)
    try:
        with gate.lock:
            gate.profile_read(reset=True)
            a = sg.get_traces()
            stages = {k.split(" ")[0] for k in gate.profile_read(reset=True)}
            assert "k_gate_onepass" in stages, sorted(stages)
            _check_bits("register-1024 [persistent]", gate, units, False)
            a2 = sg.get_traces()
            _check_bits("register-1024 [persistent, second run]", gate, units, False)
            with gate.with_options([(_ffi.SG_OPT_TILE_ORDER, 2)]):
                b = sg.get_traces()
                _check_bits("register-1024 [one tile per workgroup]", gate, units, False)
        gate.check_errors()
    finally:
        gate.profile_enable(False)
    assert np.array_equal(a, b) and np.array_equal(a, a2)
