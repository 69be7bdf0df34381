"""The three table-driven paths -- reduce_noise_batch (csrc/ragged.hip), TorchGate.forward(lengths=) (csrc/rows.hip) and
StreamBank (csrc/stream.hip) -- against the float64 oracle per hop block, on the tile matrix of tests/parity_budget.py
(TILE_CELLS: path-gate x n_fft x column).  All three run the frame code of csrc/tile_core.hpp; a slip there moves a few
samples per hop or one band, far below 1e-4 of the loudest sample, which is all the paths' own suites ask for.

Per cell: the call really ran the tile kernels (route, one sub-batch, the RG stages / the step's launch count); the
stationary thresholds lie within 1e-9 dB of the oracle's; every unit of every clip, row and stream channel passes
``PB.local_check`` with the float32 budget (the tile paths keep frame segments as float32, whatever the sample type);
rows also hand back their final mask, which is held to the oracle's (stationary) or to the emulation's error
(non-stationary); the four block plans of a stream are bit-identical before any of them is compared with the oracle.
tests/test_tile_parity_host.py holds the conditions on the oracle that keep these checks from being empty.

The largest local_error / budget per path-gate and n_fft goes to the file named by TILE_PARITY_OUT, if set
(profiles/tile_parity.json is that file from an MI355X run)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import parity_budget as PB

pytestmark = pytest.mark.gpu

_RATIOS = {}
_IDS = [PB.tile_cell_id(c) for c in PB.TILE_CELLS]
_S_STAGES = {"k_rg_noise_power", "k_rg_noise_final", "k_rg_decide", "k_rg_fsmooth", "k_rg_apply", "k_rg_ola"}
_NS_STAGES = {"k_rg_decide", "k_rg_iir", "k_rg_fsmooth", "k_rg_apply", "k_rg_ola"}
_STREAM_STAGES = {"k_rg_decide", "k_rg_fsmooth", "k_rg_apply", "k_rg_ola"}


def _note(cell, ratio):
    key = "%s/%d" % (cell["path"], cell["n_fft"])
    _RATIOS[key] = max(_RATIOS.get(key, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _dump_ratios():
    yield
    path = os.environ.get("TILE_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"factor_allowed": PB.FACTOR, "largest_local_error_over_budget": dict(sorted(_RATIOS.items()))},
                      f, indent=1)


def _launches(gate):
    """{kernel: launches} of the profiled stages since the last read (first word of each stage name)."""
    return {k.split(" ")[0]: v[1] for k, v in gate.profile_read(reset=True).items() if v[1] > 0}


def _check_unit(tag, cell, u, got):
    """One unit's kept samples per hop block; returns the float32 emulation's stages for the mask checks."""
    emu = PB.emulate_stages_f32(u)
    bud = PB.budget(u, emu[0])
    got = np.asarray(got)
    assert got.shape == u["want"].shape, (tag, got.shape, u["want"].shape)
    bad, ratio = PB.local_check(got, u, bud=bud)
    print("%s: largest local_error / budget %.3f" % (tag, ratio))
    if len(bad):
        err = PB.local_error(got, u["want"], u["cfg"]["H"])
        raise AssertionError("%s: hop blocks %s of %d over their bound: error %s, budget %s, largest error / budget in the unit "
                             "%.2f" % (tag, bad[:10].tolist(), len(err), err[bad[:10]], bud[bad[:10]], ratio))
    _note(cell, ratio)
    return emu


# ---- reduce_noise_batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [c for c in PB.TILE_CELLS if c["path"].startswith("clips")],
                         ids=[i for i in _IDS if i.startswith("clips")])
def test_clips_cell(cell):
    import noisereduce_amd as nr
    from noisereduce_amd import batch
    case, groups = PB.tile_case(cell), PB.tile_oracle(cell)
    tag = PB.tile_cell_id(cell)
    kw = dict(case["kw"])
    stationary = kw.pop("stationary")
    dt = np.dtype(case["dtype"])
    ys = [y.astype(dt) for y in case["ys"]]
    yn = case["y_noise"]
    p = batch.plan(ys, PB.SR, stationary=stationary, y_noise=yn, **kw)
    assert p.routes == [batch.BATCHED] * len(ys) and len(p.units) == sum(len(g) for g in groups)
    g = batch._gate_for(PB.SR, stationary, p, dict(kw, n_std_thresh_stationary=1.5, time_constant_s=2.0,
                                                   thresh_n_mult_nonstationary=2, sigmoid_slope_nonstationary=10), "cuda")
    g.profile_enable(True)
    try:
        g.profile_read(reset=True)
        outs = nr.reduce_noise_batch(ys, PB.SR, stationary=stationary, y_noise=yn, **kw)
        launched = _launches(g)
    finally:
        g.profile_enable(False)
    assert g.clip_batches() == 1
    want_stages = _S_STAGES if stationary else _NS_STAGES
    assert launched == {k: 1 for k in want_stages}, (tag, launched)
    if stationary:
        n_noise = len(ys) if isinstance(yn, list) else 1
        thr = g.clip_thresholds(n_noise)
        for i, grp in enumerate(groups):
            d = np.max(np.abs(thr[i if n_noise > 1 else 0] - grp[0]["thresh"]))
            assert d <= 1e-9, "%s clip %d: threshold %.3g dB from the oracle's" % (tag, i, d)
    for i, (y, o, grp) in enumerate(zip(ys, outs, groups)):
        assert o.shape == y.shape and o.dtype == dt, (tag, i)
        o2 = np.atleast_2d(o)
        covered = np.zeros(o2.shape, dtype=bool)
        for u in grp:
            s0, e0 = u["dst"]
            _check_unit("%s clip %d channel %d chunk %d" % (tag, i, u["ch"], u["chunk"]), cell, u, o2[u["ch"], s0:e0])
            covered[u["ch"], s0:e0] = True
        assert covered.all()


# ---- TorchGate.forward(lengths=) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [c for c in PB.TILE_CELLS if c["path"].startswith("rows")],
                         ids=[i for i in _IDS if i.startswith("rows")])
def test_rows_cell(cell):
    from noisereduce_amd.torchgate import TorchGate
    case, groups = PB.tile_case(cell), PB.tile_oracle(cell)
    tag = PB.tile_cell_id(cell)
    kw, H, n_fft = case["kw"], case["H"], cell["n_fft"]
    F = n_fft // 2 + 1
    tdt = torch.float64 if case["dtype"] == "float64" else torch.float32
    x = torch.from_numpy(case["x"]).to(tdt).cuda()
    xn = None if case["xn"] is None else torch.from_numpy(case["xn"]).to(tdt).cuda()
    lengths = case["lengths"]
    tg = TorchGate(sr=PB.SR, **kw).cuda()
    gate = tg._gate_for(x.device)
    gate.profile_enable(True)
    try:
        gate.profile_read(reset=True)
        y = tg(x, xn, lengths=lengths)
        launched = _launches(gate)
    finally:
        gate.profile_enable(False)
    assert gate.rows_batches() == 1
    assert launched == {k: 1 for k in (_S_STAGES if cell["stationary"] else _NS_STAGES)}, (tag, launched)
    assert y.dtype == tdt and tuple(y.shape) == (x.shape[0], H * (x.shape[1] // H))
    with gate.lock:
        y2, mask = gate.process_rows(x, lengths, xn, None, save_mask=True)
    assert gate.rows_batches() == 1 and torch.equal(y2, y)
    got, mask = y.cpu().numpy(), mask.cpu().numpy()
    worst_field = 0.0
    for b, grp in enumerate(groups):
        u = grp[0]
        n = len(u["want"])
        assert n == H * (int(lengths[b]) // H)
        emu = _check_unit("%s row %d" % (tag, b), cell, u, got[b, :n])
        assert np.all(got[b, n:] == 0), "%s row %d: samples written beyond the row's own output" % (tag, b)
        T = u["mask"].shape[1]
        M = mask[b, :T, :F].T
        assert np.all(mask[b, T:, :F] == 0), "%s row %d: mask rows written beyond the row's own frames" % (tag, b)
        if cell["stationary"]:
            cells, w = PB.mask_diff(M, u, bound=PB.mask_bound(u["cfg"]))
            assert len(cells) == 0, "%s row %d: final mask off by up to %.3g (bound %.3g) at %d cells, first (band, frame) %s" % (
                tag, b, w, PB.mask_bound(u["cfg"]), len(cells), cells[:6].tolist())
            if u["cfg"]["filt"] is None and u["cfg"]["prop"] == 1.0:      # the mask is the bits
                assert set(np.unique(M).tolist()) <= {0.0, 1.0}
                cells, left = PB.bit_diff(M > 0.5, u)
                assert left <= PB.LEFT_OUT_CAP
                assert len(cells) == 0, "%s row %d: %d decision bits differ from the oracle, first (band, frame) %s" % (
                    tag, b, len(cells), cells[:6].tolist())
        else:
            worst_field = max(worst_field, PB._field_rule(M, u["mask"], emu[2], "%s row %d final mask" % (tag, b)))
    if not cell["stationary"]:
        print("%s: largest mask error / the emulation's %.3f" % (tag, worst_field))


# ---- StreamBank ----------------------------------------------------------------------------------------------------
def _run_streams(bank, plans):
    """plans: {slot: (signal (N,) or (C, N), cuts)}.  Step i pushes every stream's i-th block; then all are flushed.
    Returns ({slot: output}, number of steps)."""
    blocks = {s: np.split(np.asarray(y), c, axis=-1) for s, (y, c) in plans.items()}
    outs = {s: [] for s in plans}
    steps = max(len(b) for b in blocks.values())
    for i in range(steps):
        for s, o in bank.push({s: b[i] for s, b in blocks.items() if i < len(b)}).items():
            outs[s].append(o)
    for s, o in bank.flush(list(plans)).items():
        outs[s].append(o)
    return {s: np.concatenate(v, axis=-1) for s, v in outs.items()}, steps + 1


def _bank_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("stationary", "chunk_size", "padding")}


@pytest.mark.parametrize("cell", [c for c in PB.TILE_CELLS if c["path"].startswith("stream")],
                         ids=[i for i in _IDS if i.startswith("stream")])
def test_stream_cell(cell):
    from noisereduce_amd import stream
    case, units = PB.tile_case(cell), PB.tile_oracle(cell)[0]
    tag = PB.tile_cell_id(cell)
    dt = np.dtype(case["dtype"])
    y = case["y"].astype(dt)
    N, C = y.shape[-1], case["C"]
    if cell["stationary"]:
        bank = stream.StreamBank(PB.SR, 4, channels=C, y_noise=case["y_noise"], max_block=N, **_bank_kw(case["kw"]))
        d = np.max(np.abs(bank.thresholds() - units[0]["thresh"]))
        assert d <= 1e-9, "%s: threshold %.3g dB from the oracle's" % (tag, d)
    else:
        bank = stream.StreamBank(PB.SR, 4, channels=C, stationary=False, lookahead_ms=case["lookahead_ms"], max_block=N,
                                 **_bank_kw(case["kw"]))
        assert bank.lookahead_frames >= case["frames"] - 1
    g = bank.gate
    g.profile_enable(True)
    try:
        g.profile_read(reset=True)
        got, steps = _run_streams(bank, {s: (y, case["plans"][k]) for s, k in enumerate(PB.STREAM_PLANS)})
        launched = _launches(g)
    finally:
        g.profile_enable(False)
    assert launched == {k: steps for k in _STREAM_STAGES}, (tag, steps, launched)
    for s, k in enumerate(PB.STREAM_PLANS):
        assert got[s].shape == y.shape and got[s].dtype == dt, (tag, k)
        if s:
            same = np.array_equal(got[s], got[0], equal_nan=True)
            where = [] if same else np.flatnonzero(np.any(np.atleast_2d(got[s] != got[0]), axis=0))[:6].tolist()
            assert same, "%s: block plan %r differs from the whole stream, first at samples %s" % (tag, k, where)
    g2 = np.atleast_2d(got[0])
    for ch, u in enumerate(units):
        _check_unit("%s channel %d" % (tag, ch), cell, u, g2[ch])
    bank.close()


@pytest.mark.parametrize("n_fft", [256, 4096])
def test_stream_under_the_causal_floor(n_fft):
    """The input of tests/test_gpu_stream.py's causal-floor test at the two outer sizes: the truth is the streaming model
    (tests/stream_model.py, restated as a unit by PB.causal_floor_case), per hop block."""
    from noisereduce_amd import stream
    cf = PB.causal_floor_case(n_fft)
    u, y = cf["unit"], cf["y"]
    N = len(y)
    bank = stream.StreamBank(PB.SR, 1, y_noise=cf["noise"], max_block=N, **_bank_kw(cf["kw"]))
    assert np.max(np.abs(bank.thresholds() - u["thresh"])) <= 1e-9
    rng = np.random.default_rng(n_fft)
    got, _ = _run_streams(bank, {0: (y, PB.stream_cuts("random", N, u["cfg"]["W"], u["cfg"]["H"], rng))})
    cell = dict(path="stream-S-causal", n_fft=n_fft)
    _check_unit("stream-S-causal-%d" % n_fft, cell, u, got[0])
    bad, _ = PB.local_check(got[0], dict(cf["offline"]))
    assert len(bad) > 0      # and it is not the offline gate
    bank.close()
