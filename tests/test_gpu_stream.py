"""StreamBank on the GPU: every stream's concatenated output against the float64 oracle run offline, against
reduce_noise on the same device, and against the float64 streaming model; bitwise invariance; the causal floor; buffer
discipline; launch counts."""
import numpy as np
import pytest
import torch

import noisereduce_amd as nr
from noisereduce_amd import stream
from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests import stream_model as M

pytestmark = pytest.mark.gpu

# (sr, n_fft, win_length, hop_length)
GEOMS = [(48000, 1024, None, None), (16000, 512, 400, 160), (8000, 256, None, 50), (44100, 2048, 1500, 333),
         (48000, 4096, None, None)]
SMOOTH = {"on": (500, 50), "time_off": (500, None), "off": (None, None)}
ORACLE_TOL = 1e-4      # of peak: the project's bar
DEVICE_TOL = 2e-6      # of peak, against reduce_noise on the same device (tests/test_gpu_batch_fuzz.py's bound)


def _noise(sr, seed=7):
    return 0.1 * np.random.default_rng(seed).standard_normal(3 * sr // 4)


def _kw(sr, n_fft, W, H, fhz=500, tms=50, p=1.0):
    return dict(n_fft=n_fft, win_length=W, hop_length=H, freq_mask_smooth_hz=fhz, time_mask_smooth_ms=tms, prop_decrease=p)


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


def _model(y, thresh, sr, n_fft, W, H, fhz, tms, p):
    n_fft_, W_, H_, nf, nt, smooth, _ = M.geometry(sr, n_fft, W, H, fhz, tms)
    outs, live = M.stream_model([np.asarray(y, dtype=np.float64)], thresh, n_fft_, W_, H_, p, nf, nt, smooth)
    return np.concatenate(outs), live


def _thresh(noise, sr, n_fft, W, H):
    n_fft_, W_, H_ = O.resolve_stft_params(n_fft, W, H)
    return O.noise_threshold_S(np.atleast_2d(noise), n_fft_, W_, H_, 1.5, None, True)[0]


@pytest.mark.parametrize("p", [1.0, 0.7])
@pytest.mark.parametrize("smooth", list(SMOOTH))
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%d-%d" % (g[0], g[1]))
def test_streams_equal_the_offline_gate(geom, dtype, smooth, p):
    sr, n_fft, W, H = geom
    fhz, tms = SMOOTH[smooth]
    n_fft_, W_, H_ = O.resolve_stft_params(n_fft, W, H)
    case = GEOMS.index(geom) * 12 + (dtype == np.float64) * 6 + list(SMOOTH).index(smooth) * 2 + (p != 1.0)
    rng = np.random.default_rng(case)
    C = 1 + case % 2
    noise = _noise(sr)
    thresh = _thresh(noise, sr, n_fft, W, H)
    kw = _kw(sr, n_fft, W, H, fhz, tms, p)
    lens = [int(n) for n in rng.integers(W_ + 5, 6 * W_ + 20 * H_, 4)]
    bank = stream.StreamBank(sr, 5, channels=C, y_noise=noise, max_block=max(lens), **kw)
    assert np.max(np.abs(bank.thresholds() - thresh)) <= 1e-9
    plans = {}
    for s, (N, kind) in enumerate(zip(lens, ("whole", "random", "edge", "small"))):
        y = np.stack([O.synth_signal(N, sr=sr, seed=100 * case + 10 * s + c, dtype=dtype) for c in range(C)])
        plans[s + 1] = (y if C > 1 else y[0], _cuts(kind, N, W_, H_, rng))
    got = _run(bank, plans, as_tensor=bool(case % 3 == 0))
    for s, (y, cuts) in plans.items():
        g = got[s]
        assert g.shape == np.shape(y) and g.dtype == dtype
        y2, g2 = np.atleast_2d(y), np.atleast_2d(g)
        want = np.atleast_2d(O.reduce_noise_S(y2.astype(np.float64), sr, stationary=True, y_noise=noise, chunk_size=None,
                                              padding=0, **kw))
        dev = np.atleast_2d(nr.reduce_noise(y=y2, sr=sr, y_noise=noise, stationary=True, chunk_size=None, padding=0,
                                            device="cuda", **kw))
        for c in range(C):
            model, live = _model(y2[c], thresh, sr, n_fft, W, H, fhz, tms, p)
            assert live is False
            peak = np.max(np.abs(want[c]))
            e_or = np.max(np.abs(g2[c] - want[c])) / peak
            e_dev = np.max(np.abs(g2[c] - dev[c])) / peak
            e_mod = np.max(np.abs(g2[c] - model)) / peak
            print(f"[stream] {geom} {np.dtype(dtype).name} {smooth} p={p} slot {s} ch {c}: oracle {e_or:.2e} "
                  f"device {e_dev:.2e} model {e_mod:.2e}")
            assert e_or <= ORACLE_TOL and e_mod <= ORACLE_TOL, (s, c, e_or, e_mod)
            assert e_dev <= DEVICE_TOL, (s, c, e_dev)


def _mono_bank(S, sr=16000, n_fft=512, W=400, H=160, max_block=16000, noise=None, **kw):
    noise = _noise(sr) if noise is None else noise
    return stream.StreamBank(sr, S, y_noise=noise, n_fft=n_fft, win_length=W, hop_length=H, max_block=max_block, **kw)


def test_300_streams_of_different_lengths_and_plans_and_bitwise_invariance():
    sr, n_fft, W, H = 16000, 512, 400, 160
    rng = np.random.default_rng(300)
    noise = _noise(sr)
    thresh = _thresh(noise, sr, n_fft, W, H)
    kinds = ("whole", "random", "edge", "small")
    plans = {}
    for s in range(300):
        N = int(rng.integers(W, 5000))
        plans[s] = (O.synth_signal(N, sr=sr, seed=s, dtype=np.float32), _cuts(kinds[s % 4], N, W, H, rng))
    bank = _mono_bank(300, noise=noise)
    got = _run(bank, plans)
    worst = 0.0
    for s, (y, _) in plans.items():
        model, live = _model(y, thresh, sr, n_fft, W, H, 500, 50, 1.0)
        assert live is False
        worst = max(worst, np.max(np.abs(got[s] - model)) / np.max(np.abs(model)))
    print(f"[stream] 300 streams: worst {worst:.2e} of peak against the model")
    assert worst <= ORACLE_TOL
    # the same stream under another block plan, alone in another bank, and in another slot: bit for bit
    y7 = plans[7][0]
    alone = _mono_bank(1, noise=noise)
    assert np.array_equal(_run(alone, {0: (y7, [])})[0], got[7])
    assert np.array_equal(_run(alone, {0: (y7, list(range(1, len(y7), 997)))})[0], got[7])
    again = _run(bank, {250: (y7, _cuts("small", len(y7), W, H, rng)), 0: plans[0], 3: (plans[9][0], [17])},
                 as_tensor=True)
    assert np.array_equal(again[250], got[7]) and np.array_equal(again[0], got[0]) and np.array_equal(again[3], got[9])


def test_slot_is_clean_after_a_nan_stream():
    bank = _mono_bank(2)
    y = O.synth_signal(6000, sr=16000, seed=5, dtype=np.float32)
    clean = _run(bank, {1: (y, [1000, 1001, 4000])})[1]
    bad = y.copy()
    bad[2500] = np.nan
    dirty = _run(bank, {1: (bad, [3000])})[1]
    assert np.isnan(dirty).any()
    assert np.array_equal(_run(bank, {1: (y, [77])})[1], clean)
    bank.push({1: bad[:3000]})
    bank.reset([1])
    assert np.array_equal(_run(bank, {1: (y, [])})[1], clean)


def test_causal_floor_is_the_models_and_not_the_offline_one():
    sr, n_fft, W, H = 48000, 1024, None, None
    rng = np.random.default_rng(11)
    N = 40000
    y = 1e-5 * rng.standard_normal(N)
    y[N // 2:] += 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(N - N // 2) / sr)
    y = y.astype(np.float32)
    noise = 1e-5 * rng.standard_normal(3 * sr // 4)
    thresh = _thresh(noise, sr, n_fft, W, H)
    model, live = _model(y, thresh, sr, n_fft, W, H, 500, 50, 1.0)
    assert live is True
    offline = O.reduce_noise_S(y.astype(np.float64), sr, stationary=True, y_noise=noise, chunk_size=None, padding=0)
    bank = stream.StreamBank(sr, 1, y_noise=noise, max_block=N)
    got = _run(bank, {0: (y, [5000, 20003, 20004, 31000])})[0]
    peak = np.max(np.abs(model))
    e_mod, e_off = np.max(np.abs(got - model)) / peak, np.max(np.abs(got - offline)) / peak
    print(f"[stream] causal floor: {e_mod:.2e} of peak from the model, {e_off:.2e} from the offline oracle")
    assert e_mod <= ORACLE_TOL
    assert e_off > 1e-2


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_samples_mid_stream(bad):
    sr, n_fft, W, H = 16000, 512, 400, 160
    noise = _noise(sr)
    thresh = _thresh(noise, sr, n_fft, W, H)
    y = O.synth_signal(8000, sr=sr, seed=3, dtype=np.float32)
    y[3777] = bad
    ym = y.astype(np.float64)
    ym[3777] = np.nan           # an Inf sample is treated like a NaN
    model, _ = _model(ym, thresh, sr, n_fft, W, H, 500, 50, 1.0)
    got = _run(_mono_bank(1, noise=noise), {0: (y, [1000, 3777, 3778, 6000])})[0]
    assert np.array_equal(np.isfinite(got), np.isfinite(model))
    ok = np.isfinite(model)
    assert (~ok).sum() >= 400
    assert np.max(np.abs(got[ok] - model[ok])) <= ORACLE_TOL * np.max(np.abs(model[ok]))
    # every band is gated from the first frame that saw it: the finite output after it is the (1 - p) = 0 part
    assert np.max(np.abs(got[5000:])) == 0.0


def test_quiet_part_is_held_per_hop_block():
    worst = 0.0
    for sr, n_fft, W, H in ((48000, 1024, None, None), (16000, 512, 400, 160)):
        y = PB.signals.two_level(40000, sr=sr)
        noise = _noise(sr)
        kw = dict(n_fft=n_fft, win_length=W, hop_length=H)
        _, units = PB.oracle_units(y, sr, stationary=True, y_noise=noise, chunk_size=None, padding=0, **kw)
        assert len(units) == 1
        thresh = _thresh(noise, sr, n_fft, W, H)
        assert _model(y, thresh, sr, n_fft, W, H, 500, 50, 1.0)[1] is False
        bank = stream.StreamBank(sr, 1, y_noise=noise, max_block=len(y), **kw)
        got = _run(bank, {0: (y, list(range(997, len(y), 997)))})[0]
        bad, ratio = PB.local_check(got, units[0])
        print(f"[stream] local parity n_fft={n_fft}: largest local_error / budget {ratio:.3f} (allowed {PB.FACTOR})")
        assert len(bad) == 0, (n_fft, bad[:8], ratio)
        worst = max(worst, ratio)
    assert worst <= PB.FACTOR


def test_buffers_are_read_and_written_within_their_bounds():
    sr, W, H = 16000, 400, 160
    from noisereduce_amd import _ffi
    bank = _mono_bank(3)
    bank._ensure()
    g, b = bank.gate, bank._bank
    y = O.synth_signal(5000, sr=sr, seed=8, dtype=np.float32)
    ref = _run(_mono_bank(1), {0: (y, [])})[0]
    x = torch.full((3100,), float("nan"), device="cuda")
    out = torch.full((6000,), -77.0, device="cuda")
    pos, done, chunks = 0, 0, []
    for n in (700, 0, 1, 1299, 3000):
        x.fill_(float("nan"))
        x[5:5 + n] = torch.from_numpy(y[pos:pos + n]).cuda()
        flush = pos + n == len(y)
        k = (len(y) if flush else stream.emitted(pos + n, W, H, bank.nt)) - done
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
    k = stream.emitted(n, 400, 160, bank.nt)
    assert all(o.is_cuda and o.shape == (k,) for o in outs.values())
    torch.cuda.synchronize()
    assert pending
    gate = nr.StreamGate(16000, y_noise=_noise(16000), n_fft=512, win_length=400, hop_length=160, max_block=n)
    y = O.synth_signal(n, sr=16000, seed=0, dtype=np.float32)
    one = np.concatenate([gate.push(y), gate.flush()])
    assert np.array_equal(one[:k], outs[0].cpu().numpy())
