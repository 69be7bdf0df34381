"""k_gate_onepass with the launch plan (noisereduce_amd/csrc/onepass_plan.hpp: quotients by multiply-high, interior units'
flags by range, folded addresses) against the three-kernel path, bit for bit, at the smallest shapes at which a tile's
coordinates can go wrong: 2 and 3 tiles per unit plus the two halo tiles (chunk_size 4096 and 8192 at padding 2048: 16 and 32
hops, n_tiles = (hops + 3 + 15) // 16; a unit of 2 tiles has no tile_fast tile, so its interior units are known to the plan by
blk_vec alone), rows of 1, 3 and 7 chunks with a ragged remainder -- so every edge unit sits next to an interior one --, 1 and
3 channels, a float32 view one sample into its buffer (no unit is interior: rows lose their alignment), int16 input, partial
reduction, a get_traces sub-range, and both ticket-drawn tile orders (0: persistent workgroups, the plan's user; 2: one tile per
workgroup, which shares the source).
Compared as tests/test_gpu_onepass.py::test_onepass_equals_three_kernel_path compares."""
import numpy as np
import pytest
import torch

from oracle import spectralgate_oracle as O

pytestmark = pytest.mark.gpu

SG_KW = dict(sr=48000, y_noise=None, prop_decrease=1.0, n_std_thresh_stationary=1.5, chunk_size=8192,
             clip_noise_stationary=True, padding=2048, n_fft=1024, win_length=None, hop_length=None,
             time_constant_s=2.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50, tmp_folder=None,
             use_tqdm=False, n_jobs=1)
RAGGED = 1234   # samples behind the last whole chunk


def _sg(y, cs, **over):
    from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
    kw = dict(SG_KW, chunk_size=cs)
    kw.update(over)
    return SpectralGateStationary(y=y, **kw)


def _signal(n, C):
    y = np.stack([O.synth_signal(n, sr=48000, seed=170 + c, tone_hz=400.0 * (c + 1)) for c in range(C)]).astype(np.float32)
    return y[0] if C == 1 else y


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _onepass_vs_split(sg, exact=True, **rng):
    """One-pass gate at SG_OPT_TILE_ORDER 0 and 2 against the decide / smooth / apply kernels on the same handle."""
    from noisereduce_amd import _ffi
    g = sg._gate
    got = {}
    try:
        for order in (0, 2):
            g.set_option(_ffi.SG_OPT_TILE_ORDER, order)
            got[order] = _host(sg.get_traces(**rng))
            assert np.array_equal(got[order], _host(sg.get_traces(**rng))), "not deterministic run to run (tile order %d)" % order
        g.set_option(_ffi.SG_OPT_TILE_ORDER, 0)
        g.set_option(_ffi.SG_OPT_FORCE_SPLIT, 1)
        want = _host(sg.get_traces(**rng))
    finally:
        g.set_option(_ffi.SG_OPT_FORCE_SPLIT, 0)
        g.set_option(_ffi.SG_OPT_TILE_ORDER, 0)
    g.check_errors()
    assert np.isfinite(want.astype(np.float64)).all() and want.any()
    for order, a in got.items():
        if exact:
            assert np.array_equal(a, want), "one-pass gate (tile order %d) differs from the three-kernel path" % order
        else:   # partial reduction: the split path expands a float mask field first (test_onepass_equals_three_kernel_path)
            assert O.rel_err(a, want) < 2e-6, order
    return want


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("chunks", [1, 3, 7])
@pytest.mark.parametrize("cs", [4096, 8192])
def test_plan_gate_equals_three_kernel_path(cs, chunks, C):
    _onepass_vs_split(_sg(_signal(chunks * cs + RAGGED, C), cs))


@pytest.mark.parametrize("cs", [4096, 8192])
@pytest.mark.parametrize("C", [1, 3])
def test_float32_view_one_sample_into_its_buffer(C, cs):
    n = 7 * cs + RAGGED
    buf = torch.from_numpy(np.atleast_2d(_signal(n + 1, C))).to("cuda:0")
    y = buf[:, 1:] if C > 1 else buf[0, 1:]
    assert y.data_ptr() % 16 == 4
    got = _onepass_vs_split(_sg(y, cs))
    # ... and it is the gate of the same samples in an aligned buffer
    assert np.array_equal(got, _onepass_vs_split(_sg(y.clone(), cs)))


@pytest.mark.parametrize("cs", [4096, 8192])
def test_int16_input(cs):
    y = np.round(_signal(7 * cs + RAGGED, 1) * 12000.0).astype(np.int16)
    _onepass_vs_split(_sg(y, cs))


@pytest.mark.parametrize("cs", [4096, 8192])
def test_partial_reduction(cs):
    _onepass_vs_split(_sg(_signal(7 * cs + RAGGED, 3), cs, prop_decrease=0.8), exact=False)


@pytest.mark.parametrize("cs", [4096, 8192])
@pytest.mark.parametrize("a, b", [(1 + 100 / 8192, 5 + 17 / 8192), (2, 6), (3 + 4 / 8192, 4.25)])
def test_get_traces_sub_range(a, b, cs):
    """[start, end) in chunks: inside chunks 1 and 5, on chunk boundaries, and a little over one chunk from an offset of 4."""
    start, end = int(round(a * cs)), int(round(b * cs))
    y = _signal(7 * cs + RAGGED, 3)
    sg = _sg(y, cs)
    part = _onepass_vs_split(sg, start_frame=start, end_frame=end)
    assert part.shape[-1] == end - start
