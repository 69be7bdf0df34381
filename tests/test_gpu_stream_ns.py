"""The non-stationary StreamBank on the GPU: every stream's concatenated output against the float64 streaming model; with
a lookahead that covers the stream against the float64 oracle run offline and reduce_noise on the same device; per hop
block against tests/parity_budget.py; bitwise invariance; NaN / Inf / digital silence; buffer discipline; launch counts;
a stationary and a non-stationary bank side by side."""
import numpy as np
import pytest
import torch

import noisereduce_amd as nr
from noisereduce_amd import stream
from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests import stream_ns_model as M

pytestmark = pytest.mark.gpu

# (sr, n_fft, win_length, hop_length): tests/test_gpu_stream.py's
GEOMS = [(48000, 1024, None, None), (16000, 512, 400, 160), (8000, 256, None, 50), (44100, 2048, 1500, 333),
         (48000, 4096, None, None)]
SMOOTH = {"on": (500, 50), "time_off": (500, None), "off": (None, None)}
ORACLE_TOL = 1e-4      # of peak: the project's bar
DEVICE_TOL = 2.5e-6    # of peak, against reduce_noise(stationary=False) on the same device: see the test that uses it
LOOKAHEADS_MS = (0.0, 30.0, 100.0)
TIME_CONSTANTS = (0.1, 2.0)


def _kw(n_fft, W, H, fhz=500, tms=50, p=1.0, tc=2.0):
    return dict(n_fft=n_fft, win_length=W, hop_length=H, freq_mask_smooth_hz=fhz, time_mask_smooth_ms=tms, prop_decrease=p,
                time_constant_s=tc)


def _cuts(kind, N, W, H, rng):
    if kind == "whole":
        return []
    if kind == "random":
        return sorted(int(c) for c in rng.integers(0, N + 1, 7))
    if kind == "edge":       # 1-sample blocks around the sample that completes a frame, and a few 0-sample blocks
        e = 3 * H - W // 2 + W
        return sorted(min(c, N) for c in (e - 3, e - 2, e - 1, e, e, e, e + 1, e + 2, N // 2, N // 2))
    if kind == "small":
        return list(range(131, N, 131))
    raise KeyError(kind)


def _run(bank, plans, as_tensor=False):
    """plans: {slot: (signal (N,) or (C, N), cuts)}.  Step i pushes every stream's i-th block; then all are flushed."""
    blocks = {s: np.split(np.asarray(y), c, axis=-1) for s, (y, c) in plans.items()}
    outs = {s: [] for s in plans}
    for i in range(max(len(b) for b in blocks.values())):
        step = {s: b[i] for s, b in blocks.items() if i < len(b)}
        if as_tensor:
            step = {s: torch.from_numpy(np.ascontiguousarray(v)).cuda() for s, v in step.items()}
        for s, o in bank.push(step).items():
            outs[s].append(o.cpu().numpy() if as_tensor else o)
    for s, o in bank.flush(list(plans)).items():
        outs[s].append(o.cpu().numpy() if as_tensor else o)
    return {s: np.concatenate(v, axis=-1) for s, v in outs.items()}


def _model(y, sr, n_fft, W, H, fhz, tms, p, tc, L, direct=False):
    n_fft_, W_, H_, nf, nt, smooth, _ = M.geometry(sr, n_fft, W, H, fhz, tms)
    b = O.iir_coefficient(tc, sr, H_)
    return np.concatenate(M.stream_ns_model([np.asarray(y, dtype=np.float64)], n_fft_, W_, H_, p, nf, nt, smooth, b, L,
                                            direct=direct))


def _frames(N, W, H):
    return (N + 2 * (W // 2) - W) // H + 1


@pytest.mark.parametrize("p", [1.0, 0.7])
@pytest.mark.parametrize("smooth", list(SMOOTH))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%d-%d" % (g[0], g[1]))
def test_streams_equal_the_model(geom, dtype, smooth, p):
    sr, n_fft, W, H = geom
    fhz, tms = SMOOTH[smooth]
    n_fft_, W_, H_ = O.resolve_stft_params(n_fft, W, H)
    case = GEOMS.index(geom) * 12 + (dtype == np.float64) * 6 + list(SMOOTH).index(smooth) * 2 + (p != 1.0)
    rng = np.random.default_rng(case)
    C = 1 + case % 2
    ms, tc = LOOKAHEADS_MS[case % 3], TIME_CONSTANTS[(case // 3) % 2]
    kw = _kw(n_fft, W, H, fhz, tms, p, tc)
    lens = [int(n) for n in rng.integers(W_ + 5, 6 * W_ + 20 * H_, 4)]
    bank = stream.StreamBank(sr, 5, channels=C, stationary=False, lookahead_ms=ms, max_block=max(lens), **kw)
    L = bank.lookahead_frames
    assert L == int(ms / (H_ / sr * 1000))
    plans = {}
    for s, (N, kind) in enumerate(zip(lens, ("whole", "random", "edge", "small"))):
        y = np.stack([O.synth_signal(N, sr=sr, seed=100 * case + 10 * s + c, dtype=dtype) for c in range(C)])
        plans[s + 1] = (y if C > 1 else y[0], _cuts(kind, N, W_, H_, rng))
    got = _run(bank, plans, as_tensor=bool(case % 3 == 0))
    for s, (y, cuts) in plans.items():
        g = got[s]
        assert g.shape == np.shape(y) and g.dtype == dtype
        y2, g2 = np.atleast_2d(y), np.atleast_2d(g)
        for c in range(C):
            model = _model(y2[c], sr, n_fft, W, H, fhz, tms, p, tc, L)
            e_mod = np.max(np.abs(g2[c] - model)) / np.max(np.abs(model))
            print(f"[stream-ns] {geom} {np.dtype(dtype).name} {smooth} p={p} L={L} tc={tc} slot {s} ch {c}: model {e_mod:.2e}")
            assert e_mod <= ORACLE_TOL, (s, c, e_mod)


@pytest.mark.parametrize("tc", TIME_CONSTANTS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%d-%d" % (g[0], g[1]))
def test_a_lookahead_that_covers_the_stream_gives_the_offline_gate(geom, tc):
    """L >= T - 1.  Against reduce_noise on the same device the bound is taken from the distance d of the two OFFLINE paths
    (reduce_noise on the device against the float64 oracle), measured on the MI355X over these ten cases: at most 1.03e-6 of
    peak.  The stream transforms, smooths the level and sums the mask in float64 and rounds to float32
    only at the sigmoid and the segments; the offline device path is float32 throughout.  So the stream is expected no
    farther from the oracle than that path is, and by the triangle inequality no farther than 2 d = 2.06e-6 from it:
    DEVICE_TOL = 2.5e-6.  d itself is printed and held to the project's bar."""
    sr, n_fft, W, H = geom
    n_fft_, W_, H_ = O.resolve_stft_params(n_fft, W, H)
    rng = np.random.default_rng(GEOMS.index(geom))
    N = int(5 * W_ + 31 * H_ + 7)
    T = _frames(N, W_, H_)
    kw = _kw(n_fft, W, H, tc=tc)
    y = O.synth_signal(N, sr=sr, seed=17 + GEOMS.index(geom), dtype=np.float32)
    want = O.reduce_noise_S(y.astype(np.float64), sr, stationary=False, chunk_size=None, padding=0, **kw)
    dev = nr.reduce_noise(y=y, sr=sr, stationary=False, chunk_size=None, padding=0, device="cuda", **kw)
    peak = np.max(np.abs(want))
    d_off = np.max(np.abs(dev - want)) / peak
    ms = (T + 2) * H_ / sr * 1000.0
    bank = stream.StreamBank(sr, 3, stationary=False, lookahead_ms=ms, max_block=N, **kw)
    assert bank.lookahead_frames >= T - 1
    got = _run(bank, {0: (y, []), 1: (y, _cuts("random", N, W_, H_, rng)), 2: (y, _cuts("small", N, W_, H_, rng))})
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])
    e_or = np.max(np.abs(got[0] - want)) / peak
    e_dev = np.max(np.abs(got[0] - dev)) / peak
    print(f"[stream-ns] {geom} tc={tc} L>=T-1: oracle {e_or:.2e}  device {e_dev:.2e}  (offline device vs oracle {d_off:.2e}, "
          f"allowed {DEVICE_TOL:.2e})")
    assert d_off <= ORACLE_TOL, d_off
    assert e_or <= ORACLE_TOL, e_or
    assert e_dev <= DEVICE_TOL, e_dev


def test_quiet_part_is_held_per_hop_block():
    """With L >= T - 1 the stream is the offline gate, so the oracle's units and the float32 budget of
    tests/parity_budget.py apply as they stand."""
    worst = 0.0
    for sr, n_fft, W, H in ((48000, 1024, None, None), (16000, 512, 400, 160)):
        y = PB.signals.two_level(40000, sr=sr)
        n_fft_, W_, H_ = O.resolve_stft_params(n_fft, W, H)
        kw = dict(n_fft=n_fft, win_length=W, hop_length=H)
        _, units = PB.oracle_units(y, sr, stationary=False, chunk_size=None, padding=0, **kw)
        assert len(units) == 1
        ms = (_frames(len(y), W_, H_) + 2) * H_ / sr * 1000.0
        bank = stream.StreamBank(sr, 1, stationary=False, lookahead_ms=ms, max_block=len(y), **kw)
        got = _run(bank, {0: (y, list(range(997, len(y), 997)))})[0]
        bad, ratio = PB.local_check(got, units[0])
        print(f"[stream-ns] local parity n_fft={n_fft}: largest local_error / budget {ratio:.3f} (allowed {PB.FACTOR})")
        assert len(bad) == 0, (n_fft, bad[:8], ratio)
        worst = max(worst, ratio)
    assert worst <= PB.FACTOR


def _mono_bank(S, sr=16000, n_fft=512, W=400, H=160, max_block=16000, ms=50.0, tc=0.1, **kw):
    return stream.StreamBank(sr, S, stationary=False, n_fft=n_fft, win_length=W, hop_length=H, max_block=max_block,
                             lookahead_ms=ms, time_constant_s=tc, **kw)


def test_300_streams_of_different_lengths_and_plans_and_bitwise_invariance():
    sr, n_fft, W, H = 16000, 512, 400, 160
    rng = np.random.default_rng(300)
    kinds = ("whole", "random", "edge", "small")
    plans = {}
    for s in range(300):
        N = int(rng.integers(W, 5000))
        plans[s] = (O.synth_signal(N, sr=sr, seed=s, dtype=np.float32), _cuts(kinds[s % 4], N, W, H, rng))
    bank = _mono_bank(300)
    L = bank.lookahead_frames
    assert L == 5
    got = _run(bank, plans)
    worst = 0.0
    for s, (y, _) in plans.items():
        model = _model(y, sr, n_fft, W, H, 500, 50, 1.0, 0.1, L)
        worst = max(worst, np.max(np.abs(got[s] - model)) / np.max(np.abs(model)))
    print(f"[stream-ns] 300 streams: worst {worst:.2e} of peak against the model")
    assert worst <= ORACLE_TOL
    # the same stream under another block plan, alone in another bank, in another slot, in another order: bit for bit
    y7 = plans[7][0]
    alone = _mono_bank(1)
    assert np.array_equal(_run(alone, {0: (y7, [])})[0], got[7])
    assert np.array_equal(_run(alone, {0: (y7, list(range(1, len(y7), 997)))})[0], got[7])
    again = _run(bank, {250: (y7, _cuts("small", len(y7), W, H, rng)), 3: (plans[9][0], [17]), 0: plans[0]},
                 as_tensor=True)
    assert np.array_equal(again[250], got[7]) and np.array_equal(again[0], got[0]) and np.array_equal(again[3], got[9])


def test_slot_is_clean_after_a_nan_stream():
    bank = _mono_bank(2)
    y = O.synth_signal(6000, sr=16000, seed=5, dtype=np.float32)
    clean = _run(bank, {1: (y, [1000, 1001, 4000])})[1]
    assert np.all(np.isfinite(clean))
    bad = y.copy()
    bad[2500] = np.nan
    dirty = _run(bank, {1: (bad, [3000])})[1]
    assert np.isnan(dirty).any()
    assert np.array_equal(_run(bank, {1: (y, [77])})[1], clean)
    bank.push({1: bad[:3000]})
    bank.reset([1])
    assert np.array_equal(_run(bank, {1: (y, [])})[1], clean)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_samples_mid_stream(bad):
    sr, n_fft, W, H = 16000, 512, 400, 160
    y = O.synth_signal(8000, sr=sr, seed=3, dtype=np.float32)
    y[3777] = bad
    ym = y.astype(np.float64)
    ym[3777] = np.nan           # an Inf sample is treated like a NaN
    bank = _mono_bank(1)
    model = _model(ym, sr, n_fft, W, H, 500, 50, 1.0, 0.1, bank.lookahead_frames, direct=True)
    got = _run(bank, {0: (y, [1000, 3777, 3778, 6000])})[0]
    assert np.array_equal(np.isfinite(got), np.isfinite(model))
    ok = np.isfinite(model)
    assert ok.sum() >= 1000 and (~ok).sum() >= 4000
    assert np.max(np.abs(got[ok] - model[ok])) <= ORACLE_TOL * np.max(np.abs(model[ok]))
    # the forward state stays NaN: nothing finite comes out after the sample
    assert not np.isfinite(got[3777:]).any()


def test_digital_silence_gives_what_the_oracles_arithmetic_gives():
    sr, n_fft, W, H = 16000, 512, 400, 160
    bank = _mono_bank(2)
    L = bank.lookahead_frames
    y = O.synth_signal(9000, sr=sr, seed=4, dtype=np.float32)
    y[:4000] = 0.0              # leading digital silence: S = 0 where the lookahead window is silent too
    model = _model(y, sr, n_fft, W, H, 500, 50, 1.0, 0.1, L, direct=True)
    zeros = np.zeros(3000, dtype=np.float32)
    got = _run(bank, {0: (y, [500, 3999, 4001, 7000]), 1: (zeros, [1000])})
    assert np.array_equal(np.isfinite(got[0]), np.isfinite(model))
    ok = np.isfinite(model)
    assert ok.sum() >= 3000 and (~ok).sum() >= 1000
    assert np.max(np.abs(got[0][ok] - model[ok])) <= ORACLE_TOL * np.max(np.abs(model[ok]))
    with np.errstate(invalid="ignore"):
        offline = O.reduce_noise_S(zeros.astype(np.float64), sr, stationary=False, chunk_size=None, padding=0, n_fft=n_fft,
                                   win_length=W, hop_length=H, time_constant_s=0.1)
    # (NaN up to the inverse transform's length, the zero tail after it)
    assert np.isnan(offline[:2800]).all() and np.array_equal(got[1], offline.astype(np.float32), equal_nan=True)
    # the slot is clean afterwards
    fresh = _run(_mono_bank(1), {0: (y, [])})[0]
    assert np.array_equal(_run(bank, {1: (y, [123])})[1], fresh, equal_nan=True)


def test_buffers_are_read_and_written_within_their_bounds():
    sr, W, H = 16000, 400, 160
    from noisereduce_amd import _ffi
    bank = _mono_bank(3)
    bank._ensure()
    g, b = bank.gate, bank._bank
    lag = bank.nt + bank.lookahead_frames
    y = O.synth_signal(5000, sr=sr, seed=8, dtype=np.float32)
    ref = _run(_mono_bank(1), {0: (y, [])})[0]
    x = torch.full((3100,), float("nan"), device="cuda")
    out = torch.full((6000,), -77.0, device="cuda")
    pos, done, chunks = 0, 0, []
    for n in (700, 0, 1, 1299, 3000):
        x.fill_(float("nan"))
        x[5:5 + n] = torch.from_numpy(y[pos:pos + n]).cuda()
        flush = pos + n == len(y)
        k = (len(y) if flush else stream.emitted(pos + n, W, H, lag)) - done
        if not flush:
            assert g.stream_bank_emitted(b, pos + n) == stream.emitted(pos + n, W, H, lag)
        out.fill_(-77.0)
        g.stream_push(b, x, out, [_ffi.SgStreamRec(slot=2, flush=int(flush), n_samples=n, in_offset=5, in_stride=n,
                                                   out_offset=11, out_stride=k)])
        o = out.cpu().numpy()
        assert np.all(o[:11] == -77.0) and np.all(o[11 + k:] == -77.0)
        chunks.append(o[11:11 + k].copy())
        pos, done = pos + n, done + k
        if not flush:
            assert g.stream_counters(b, 2) == (pos, done)
    assert np.array_equal(np.concatenate(chunks), ref)
    assert g.stream_state_bytes(3, 1, bank.max_block, bank.lookahead_frames) == bank.state_bytes
    with pytest.raises(ValueError):
        g.stream_set_threshold(b, [0], np.zeros(257))      # a non-stationary bank takes no threshold


def test_launches_per_step_do_not_depend_on_the_step():
    counts = []
    for S, n in ((3, 1), (300, 1), (3, 16000), (300, 16000)):
        bank = _mono_bank(S)
        x = {s: torch.from_numpy(O.synth_signal(n, sr=16000, seed=s, dtype=np.float32)).cuda() for s in range(S)}
        bank.push(x)
        g = bank.gate
        g.profile_enable(True)
        g.profile_read(reset=True)
        bank.push(x)
        counts.append({k: v[1] for k, v in g.profile_read(reset=True).items()})
        g.profile_enable(False)
    assert all(c == counts[0] for c in counts), counts
    assert sum(counts[0].values()) == 4


def test_push_of_device_tensors_returns_shapes_from_host_arithmetic():
    S, n = 64, 16000
    bank = _mono_bank(S)
    x = {s: torch.from_numpy(O.synth_signal(n, sr=16000, seed=s, dtype=np.float32)).cuda() for s in range(S)}
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    outs = bank.push(x)
    done.record()
    pending = not done.query()          # the step was only enqueued: its kernels have not finished yet
    k = stream.emitted(n, 400, 160, bank.nt + bank.lookahead_frames)
    assert all(o.is_cuda and o.shape == (k,) for o in outs.values())
    torch.cuda.synchronize()
    assert pending
    gate = nr.StreamGate(16000, stationary=False, n_fft=512, win_length=400, hop_length=160, max_block=n, lookahead_ms=50.0,
                         time_constant_s=0.1)
    y = O.synth_signal(n, sr=16000, seed=0, dtype=np.float32)
    one = np.concatenate([gate.push(y), gate.flush()])
    assert np.array_equal(one[:k], outs[0].cpu().numpy())


def test_a_stationary_and_a_non_stationary_bank_side_by_side():
    sr = 16000
    geo = dict(n_fft=512, win_length=400, hop_length=160, max_block=16000)
    noise = 0.1 * np.random.default_rng(7).standard_normal(3 * sr // 4)
    y = O.synth_signal(7000, sr=sr, seed=12, dtype=np.float32)
    cuts = list(range(800, 7000, 800))
    alone_s = _run(stream.StreamBank(sr, 2, y_noise=noise, **geo), {1: (y, cuts)})[1]
    alone_n = _run(_mono_bank(2), {1: (y, cuts)})[1]
    bs, bn = stream.StreamBank(sr, 2, y_noise=noise, **geo), _mono_bank(2)
    outs_s, outs_n = [], []
    for blk in np.split(y, cuts):
        outs_n.append(bn.push({1: blk})[1])
        outs_s.append(bs.push({1: blk})[1])
    outs_s.append(bs.flush([1])[1])
    outs_n.append(bn.flush([1])[1])
    assert np.array_equal(np.concatenate(outs_s), alone_s)
    assert np.array_equal(np.concatenate(outs_n), alone_n)
    assert not np.array_equal(alone_s, alone_n)
