"""The routes of the planner (csrc/route.hpp: plan_S, plan_T) on the GPU, one cell per pipeline of plan_S -- and the row gate's
160-row edge of plan_T -- that the other route tests (test_gpu_torchgate_routes.py, test_gpu_reg_epilogue.py) do not pin by
launch counts.  tests/test_route_plan_host.py holds the table itself; here each cell shows that the engine runs what the plan
says:

* the profiled stage launch counts of the call equal the cell's table (a stage = one profiling scope; the noise statistics of
  the constructor are not part of the call);
* sg_debug_dims, sg_debug_range and sg_debug_counter 17 (the smoothing route) report the plan's facts: the units of the batch,
  or 0 where the route keeps no fields; all frames, a window of them, or the frames the one-pass tiles reach; the smoothing kernel;
* every hop block of every unit within FACTOR x the float32 budget of the float64 oracle (tests/parity_budget.py: local_check);
  integer outputs at most 1 LSB from the truncated float64 result.

Variant S shapes: two channels of 30 000 samples in chunks of 12 000 + 2 x 3 000 (the last chunk holds 6 000), float32; the
fallback cells gate two channels of 2 600 samples as one unit each (11 hops: fewer than two one-pass tiles).  The stationary
cells set SG_OPT_FLOOR_TEST 2 (the floor test in the gate kernel), so that the launch counts do not depend on the prediction.
Geometries: n_fft 1024 / 512 / 256 / 2048 (register transforms), 4096 (LDS transform) and 1000 (mixed radix)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import parity_budget as PB

pytestmark = pytest.mark.gpu

N, CS, PAD, N_SHORT = 30000, 12000, 3000, 2600
PREP, MAX, BITS, MASK = "k_unit_absmax+k_prep_thresh", "k_stft_bits<max>", "k_stft_bits<decide>", "mask"
ONEPASS_REG = {"k_gate_onepass": 1, MAX: 1, "k_apply_fast": 1}            # (k_apply_fast: the seam kernel's scope)
BITS3 = {PREP: 1, MAX: 1, "k_decide_fast": 1, MASK: 1, "k_apply_fast": 1}
FUSED_LDS = {PREP: 1, MAX: 1, BITS: 1, MASK: 1, "k_apply_istft": 1, "k_ola": 1}
SMOOTH = {"none": 0, "off": 1, "tiled": 2, "separate": 3, "bits2": 4, "bits": 5, "onepass": 6, "onepass_reg": 7, "row_gate": 8,
          "iir_mask": 9, "box_mask": 10, "x_tiled": 11, "x_separate": 12}


def _c(name, n_fft, stages, smooth, rng, opts=(), stationary=True, prop=1.0, short=False, dtype="float32", units=None, **kw):
    return dict(name=name, n_fft=n_fft, stages=stages, smooth=smooth, range=rng, opts=opts, stationary=stationary, prop=prop,
                short=short, dtype=dtype, units=units, kw=kw)


# range: "tiles" (the frames the one-pass tiles reach), "window" (k_decide_fast decides the frames the kept hops need), "all",
# None (the route decides no bits: sg_debug_range is not its business)
CELLS = [
    _c("onepass-1024", 1024, {"k_gate_onepass": 1, MAX: 1}, "onepass", "tiles"),
    _c("onepass-1024-prop", 1024, {"k_gate_onepass": 1, MAX: 1}, "onepass", "tiles", prop=0.8),
    _c("onepass-512", 512, ONEPASS_REG, "onepass_reg", "tiles"),
    _c("onepass-256", 256, ONEPASS_REG, "onepass_reg", "tiles"),
    _c("onepass-2048", 2048, ONEPASS_REG, "onepass_reg", "tiles"),
    _c("fallback-bits3", 1024, BITS3, "bits2", "window", short=True),
    _c("fallback-fused-prop", 1024, {PREP: 1, MAX: 1, BITS: 1, MASK: 1, "k_apply_fast": 1}, "bits2", "all", prop=0.8, short=True),
    _c("split-1024", 1024, BITS3, "bits2", "window", opts=("SG_OPT_FORCE_SPLIT",)),
    _c("split-512", 512, {"k_decide_fast": 1, MAX: 2, MASK: 1, "k_apply_fast": 1}, "bits2", "all", opts=("SG_OPT_FORCE_SPLIT",)),
    _c("f64-decide", 1024, {PREP: 1, MAX: 1, BITS: 1, MASK: 1, "k_apply_fast": 1}, "bits2", "all", opts=("SG_OPT_FORCE_F64_DECIDE",)),
    _c("lds-4096", 4096, FUSED_LDS, "bits2", "all", freq_mask_smooth_hz=200),      # (nf = 17: 500 Hz are 42 bins, beyond the bit path)
    _c("mixed-1000", 1000, FUSED_LDS, "bits2", "all"),
    _c("unfused", 1024, {"k_stft<double>": 1, "k_colmax": 1, "k_decide": 1, MASK: 1, "k_apply_fast": 1}, "tiled", None,
       opts=("SG_OPT_FORCE_UNFUSED",)),
    _c("nofast-unfused", 1024, {"k_stft<double>": 1, "k_colmax": 1, "k_decide": 1, MASK: 1, "k_apply_istft": 1, "k_ola": 1}, "tiled", None,
       opts=("SG_OPT_FORCE_UNFUSED", "SG_OPT_FORCE_NOFAST")),
    _c("exact-fused", 1024, BITS3, "bits2", "window", dtype="int16"),
    _c("exact-apply64", 1024, {"k_stft<double>": 1, "k_decide": 1, MASK: 1, "k_apply_fast": 1}, "x_tiled", None, dtype="int16",
       opts=("SG_OPT_FORCE_F64_DECIDE",), units=0),
    _c("exact-materialised", 1024, {"k_stft<double>": 1, "k_decide": 1, MASK: 1, "k_apply_istft": 1, "k_ola": 1}, "x_separate", None,
       dtype="int16", opts=("SG_OPT_EXACT_MATERIALISED",), units=0),
    _c("ns-smoothed", 1024, {"k_mag_fast*": 1, "k_iir_chain_par": 1, "k_iir_mask<nt>": 1, "k_apply_fast": 1}, "iir_mask", None,
       stationary=False),
    _c("ns-chain", 1024, {"k_mag_fast*": 1, "k_iir_chain_par": 1, "k_iir_mask<nt>": 1, MASK: 1, "k_apply_fast": 1}, "tiled", None,
       stationary=False, time_mask_smooth_ms=120),      # nt = 22: no k_iir_mask<22>
    _c("ns-raw", 1024, {"k_mag_fast*": 1, "k_box_mask": 1, MASK: 1, "k_apply_fast": 1}, "tiled", None, stationary=False,
       opts=("SG_OPT_FORCE_UNFUSED",)),
]


def _signal(cell):
    n = N_SHORT if cell["short"] else N
    y = np.stack([PB.signals.dc_nyquist(n, PB.SR, 31 + ch) for ch in range(2)])
    return np.round(y * 20000.0).astype(np.int16) if cell["dtype"] == "int16" else y.astype(np.float32)


def _kw(cell):
    n = N_SHORT if cell["short"] else N
    return dict(stationary=cell["stationary"], n_fft=cell["n_fft"], chunk_size=n if cell["short"] else CS,
                padding=0 if cell["short"] else PAD, prop_decrease=cell["prop"], **cell["kw"])


@functools.lru_cache(maxsize=None)
def _oracle(n_fft, stationary, prop, short, dtype, kw):
    """The float64 oracle's output and units of a shape (computed once, shared by the cells of the shape; nobody writes to them)."""
    cell = dict(n_fft=n_fft, stationary=stationary, prop=prop, short=short, dtype=dtype, kw=dict(kw))
    return PB.oracle_units(_signal(cell).astype(np.float64), PB.SR, **_kw(cell))


def _make_sg(y, kw):
    common = dict(y=y, sr=PB.SR, chunk_size=kw["chunk_size"], padding=kw["padding"], n_fft=kw["n_fft"], win_length=None, hop_length=None,
                  time_constant_s=2.0, freq_mask_smooth_hz=kw.get("freq_mask_smooth_hz", 500), time_mask_smooth_ms=kw.get("time_mask_smooth_ms", 50), tmp_folder=None,
                  prop_decrease=kw["prop_decrease"], use_tqdm=False, n_jobs=1)
    if kw["stationary"]:
        from noisereduce_amd.spectralgate.stationary import SpectralGateStationary
        return SpectralGateStationary(y_noise=None, n_std_thresh_stationary=1.5, clip_noise_stationary=True, **common)
    from noisereduce_amd.spectralgate.nonstationary import SpectralGateNonStationary
    return SpectralGateNonStationary(thresh_n_mult_nonstationary=2, sigmoid_slope_nonstationary=10, **common)


def _dims(gate):
    d = (ctypes.c_int64 * 3)()
    gate._check(gate.lib.sg_debug_dims(gate._h, d))
    return int(d[0]), int(d[1])


def _profiled(gate, call):
    gate.profile_enable(True)
    try:
        gate.profile_read(reset=True)
        out = call()
        stages = {k.split(" ")[0]: v[1] for k, v in gate.profile_read(reset=True).items() if v[1] > 0}
    finally:
        gate.profile_enable(False)
    stages.pop("noise", None)      # (the noise statistics, where the call repeats them)
    stages.pop("k_channel_mean", None)
    return out, stages


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: c["name"])
def test_variant_s_cell(cell):
    from noisereduce_amd import _ffi
    tag = cell["name"]
    y, kw = _signal(cell), _kw(cell)
    out, units = _oracle(cell["n_fft"], cell["stationary"], cell["prop"], cell["short"], cell["dtype"], tuple(sorted(cell["kw"].items())))
    sg = _make_sg(y, kw)
    gate = sg._gate
    opts = [(getattr(_ffi, o), 1) for o in cell["opts"]] + ([(_ffi.SG_OPT_FLOOR_TEST, 2)] if cell["stationary"] else [])
    with gate.lock, gate.with_options(opts):
        est = gate.workspace_bytes(2, y.shape[1], chunked=True)
        got, stages = _profiled(gate, sg.get_traces)
        n_units, T = _dims(gate)
        d0, d1 = gate.debug_range()
        smooth = gate.debug_counter(17) & 0xff
    print("%s: stages %s, dims (%d, %d), range (%d, %d), smoothing route %d, workspace figure %d" % (tag, stages, n_units, T, d0, d1, smooth, est))
    assert stages == cell["stages"], "%s: launched %s, the plan's route launches %s" % (tag, stages, cell["stages"])
    assert smooth == SMOOTH[cell["smooth"]], (tag, smooth)
    frames = units[0]["raw"].shape[1]
    assert n_units == (len(units) if cell["units"] is None else cell["units"]), (tag, n_units, len(units))
    if n_units:
        assert T == frames, (tag, T, frames)
    if cell["range"] == "all":
        assert (d0, d1) == (0, frames), (tag, d0, d1)
    elif cell["range"] == "window":
        assert 0 <= d0 < d1 <= frames, (tag, d0, d1)
    elif cell["range"] == "tiles":
        H, padL = units[0]["cfg"]["H"], cell["n_fft"] // 2
        k0, k1 = units[0]["keep"]
        assert 0 <= d0 <= max(0, (k0 + padL) // H - 3) and (k1 - 1 + padL) // H < d1 <= frames, (tag, d0, d1)
    assert got.shape == y.shape and got.dtype == y.dtype, (tag, got.shape, got.dtype)
    if cell["dtype"] == "int16":
        d = np.abs(got.astype(np.int32) - out.astype(np.int16).astype(np.int32))     # (the reference truncates its float64 result)
        assert d.max() <= 1, "%s: %d samples more than 1 LSB from the truncated float64 result" % (tag, int(np.sum(d > 1)))
        return
    worst = 0.0
    for u in units:
        s0, e0 = u["dst"]
        bad, ratio = PB.local_check(got[u["ch"], s0:e0], u)
        worst = max(worst, ratio)
        assert len(bad) == 0, "%s channel %d chunk %d: hop blocks %s over their bound, largest error / budget %.2f" % (
            tag, u["ch"], u["chunk"], bad[:10].tolist(), ratio)
    print("%s: largest local_error / budget %.2f" % (tag, worst))


# ---- variant T: the row gate's edge, 160 rows of 64 frames (RG_MIN_ROWS) against 159 ----
RG_ROWS, RG_L = 160, 63 * 256 + 100


@functools.lru_cache(maxsize=None)
def _rows_oracle():
    x = PB.route_rows(RG_ROWS, RG_L, 77)
    _, units = PB.torchgate_units(x, PB.R_SR, window=PB.tile_window(1024))
    return x, units


@pytest.mark.parametrize("rows, stages, smooth", [(160, {"k_row_gate": 1}, "row_gate"),
                                                   (159, {"k_stft<double>": 1, "k_decide": 1, MASK: 1, "k_apply_fast": 1}, "bits2")])
def test_the_row_gate_edge(rows, stages, smooth):
    import torch
    from noisereduce_amd import _ffi
    from noisereduce_amd.torchgate import TorchGate
    x, units = _rows_oracle()
    assert units[0]["raw"].shape[1] == 64
    tg = TorchGate(sr=PB.R_SR)
    gate = _ffi.Gate("cuda", **PB.torchgate_gate_kwargs(tg))
    try:
        xd = torch.from_numpy(x[:rows]).float().cuda()
        y, got_stages = _profiled(gate, lambda: gate.process_batch(xd, None))
        n_units, T = _dims(gate)
        assert got_stages == stages, (rows, got_stages)
        assert (n_units, T) == (rows, 64) and tuple(gate.debug_range()) == (0, 64)
        assert gate.debug_counter(17) & 0xff == SMOOTH[smooth]
        got = y.cpu().numpy()
        worst = 0.0
        for b in range(0, rows, 7):      # (every seventh row: the kernels treat rows alike, the emulation costs more than the call)
            bad, ratio = PB.local_check(got[b], units[b])
            worst = max(worst, ratio)
            assert len(bad) == 0, "%d rows, row %d: hop blocks %s over their bound (%.2f)" % (rows, b, bad[:10].tolist(), ratio)
        print("%d rows: largest local_error / budget %.2f" % (rows, worst))
    finally:
        gate.close()
