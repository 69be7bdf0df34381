"""StreamBank(noise_from_stream=True) on the GPU: every stream against the float64 model of the running noise statistics
(tests/stream_adaptive_model.py), per hop block on a two-level signal, the learnt profile itself, bitwise invariance, state
hygiene, non-finite samples and silence, launch counts and buffer discipline, and a fixed-profile bank next to it."""
import functools

import numpy as np
import pytest
import torch

import noisereduce_amd as nr
from noisereduce_amd import stream
from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests import stream_adaptive_model as AM
from tests import stream_model as M

pytestmark = pytest.mark.gpu

ORACLE_TOL = 1e-4      # of peak: the project's bar (tests/test_gpu_stream.py)
DEVICE_TOL = 2e-6
PROFILE_TOL = 1e-9     # dB: the bar tests/test_gpu_tile_parity.py holds thresholds to

# (block dtype, device tensors, smoothing, prop_decrease, channels)
MIXES = {"f32-numpy-smooth-p1-mono": (np.float32, False, (500, 50), 1.0, 1),
         "f64-tensor-nosmooth-p07-stereo": (np.float64, True, (None, None), 0.7, 2),
         "f64-numpy-smooth-p07-stereo": (np.float64, False, (500, 50), 0.7, 2),
         "f32-tensor-nosmooth-p1-mono": (np.float32, True, (None, None), 1.0, 1)}
PLANS = ("whole", "20ms", "random", "long_then_short")


def _cuts(plan, N, sr, H, learn, rng):
    if plan == "whole":
        return []
    if plan == "20ms":
        return list(range(sr // 50, N, sr // 50))
    if plan == "random":        # 0- and 1-sample blocks among them
        c = sorted(int(v) for v in rng.integers(1, N, 6))
        return sorted(c + [c[1], c[1] + 1, c[3], c[3], c[4] + 1])
    if plan == "long_then_short":   # the first block ends beyond the learn window: the boundary falls inside a launch
        first = N // 2 if learn is None else max(N // 2, (learn + 8) * H)
        return [first] + list(range(first + 97, N, 1499))
    raise KeyError(plan)


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


def _kw(n_fft, W, H, fhz=500, tms=50, p=1.0):
    return dict(n_fft=n_fft, win_length=W, hop_length=H, freq_mask_smooth_hz=fhz, time_mask_smooth_ms=tms, prop_decrease=p)


@functools.lru_cache(maxsize=None)
def _model(sig_key, sr, n_fft, W, H, fhz, tms, p, mem, learn_s):
    """The model of one channel, computed once per (signal, parameters) and shared: (output, thr, raw), read-only."""
    y = _SIGNALS[sig_key]()
    n_fft_, W_, H_, nf, nt, smooth, _ = AM.geometry(sr, n_fft, W, H, fhz, tms)
    outs, thr, raw = AM.adaptive_model([np.asarray(y, dtype=np.float64)], n_fft_, W_, H_, p, nf, nt, smooth,
                                       lam=AM.forget_factor(mem, sr, H_), learn=AM.learn_frames(learn_s, sr, H_))
    out = np.concatenate(outs)
    for a in (out, thr, raw):
        a.setflags(write=False)
    return out, thr, raw


_SIGNALS = {}


def _signal(key, make):
    _SIGNALS.setdefault(key, make)
    return _SIGNALS[key]()


def _parity(geom, mem, learn_s, mix):
    sr, n_fft, W, H = geom
    dtype, as_tensor, (fhz, tms), p, C = MIXES[mix]
    N = AM.parity_length(geom)
    learn = AM.learn_frames(learn_s, sr, H)
    rng = np.random.default_rng(AM.GEOMS.index(geom) * 100 + list(MIXES).index(mix))
    keys = [("swell", geom, c) for c in range(C)]
    chans = [_signal(k, functools.partial(AM.swell, N, sr, AM.parity_seed(geom, c))) for c, k in enumerate(keys)]
    y = np.stack(chans).astype(dtype)
    bank = stream.StreamBank(sr, len(PLANS) + 1, channels=C, noise_from_stream=True, noise_memory_s=mem,
                             noise_learn_s=learn_s, max_block=N, **_kw(n_fft, W, H, fhz, tms, p))
    plans = {s + 1: (y if C > 1 else y[0], _cuts(pl, N, sr, H, learn, rng)) for s, pl in enumerate(PLANS)}
    if learn is not None:      # one block straddles the end of the learn window
        first = plans[4][1][0]
        assert M.t_dec(first, W, H) >= learn > 0
    got = _run(bank, plans, as_tensor=as_tensor)
    bank.close()
    worst = 0.0
    for s in plans:
        g = np.atleast_2d(got[s])
        assert g.shape == (C, N) and got[s].dtype == dtype
        assert np.array_equal(got[s], got[1]), (s, "the block split changed the output")
        for c in range(C):
            want, _, _ = _model(keys[c], sr, n_fft, W, H, fhz, tms, p, mem, learn_s)
            worst = max(worst, np.max(np.abs(g[c] - want)) / np.max(np.abs(want)))
    print(f"[adaptive] {geom} memory {mem} learn {learn_s} {mix}: worst {worst:.2e} of peak against the model")
    assert worst <= ORACLE_TOL


@pytest.mark.parametrize("mix", list(MIXES))
@pytest.mark.parametrize("learn_s", AM.LEARN_S)
@pytest.mark.parametrize("mem", AM.MEMORY_S)
@pytest.mark.parametrize("geom", AM.GEOMS[:3], ids=lambda g: "%d-%d" % g[:2])
def test_streams_equal_the_model(geom, mem, learn_s, mix):
    _parity(geom, mem, learn_s, mix)


def test_streams_equal_the_model_at_n_fft_4096():
    _parity(AM.GEOMS[3], 0.25, 0.3, "f64-tensor-nosmooth-p07-stereo")


def test_quiet_part_is_held_per_hop_block():
    worst = 0.0
    for sr, n_fft, W, H in ((48000, 1024, None, None), (16000, 512, 400, 160)):
        for quiet_first, p in AM.TWO_LEVEL:
            y = AM.two_level(sr, sr, quiet_first=quiet_first)
            unit = AM.unit(y, sr, n_fft, W, H, p=p)
            bank = stream.StreamBank(sr, 1, noise_from_stream=True, max_block=len(y), prop_decrease=p,
                                     n_fft=n_fft, win_length=W, hop_length=H)
            got = _run(bank, {0: (y, list(range(997, len(y), 997)))})[0]
            bank.close()
            bad, ratio = PB.local_check(got, unit)
            print(f"[adaptive] local parity n_fft={n_fft} quiet first {quiet_first} p={p}: largest local_error / budget "
                  f"{ratio:.3f} (allowed {PB.FACTOR})")
            assert len(bad) == 0, (n_fft, quiet_first, bad[:8], ratio)
            worst = max(worst, ratio)
    assert worst <= PB.FACTOR


def _mono(S, sr=16000, n_fft=512, W=400, H=160, max_block=24000, **kw):
    return stream.StreamBank(sr, S, noise_from_stream=True, n_fft=n_fft, win_length=W, hop_length=H, max_block=max_block, **kw)


def test_noise_profile_is_the_models_threshold():
    sr, n_fft, W, H = 16000, 512, 400, 160
    N = int(1.2 * sr)
    ys = np.stack([AM.swell(N, sr, 40 + c) for c in range(2)])
    for mem, learn_s in ((None, None), (0.25, 0.3)):
        lam, learn = AM.forget_factor(mem, sr, H), AM.learn_frames(learn_s, sr, H)
        bank = _mono(2, channels=2, noise_memory_s=mem, noise_learn_s=learn_s)
        assert np.isnan(bank.noise_profile(1)).all() and bank.noise_profile(1).shape == (2, n_fft // 2 + 1)
        thr = []
        for c in range(2):
            T = (N + 2 * (W // 2) - W) // H + 1
            _, db = AM.spectrum(ys[c].astype(np.float64), T, n_fft, W, H)
            thr.append(AM.recurrence(db, lam=lam, learn=learn)[1])
        n, held = 0, None
        for cut in (100, 3000, 7001, 7002, 12000, N):      # 100 samples: no frame yet
            bank.push({1: ys[:, n:cut]})
            n = cut
            prof = bank.noise_profile(1)
            assert prof.dtype == np.float64 and np.isnan(bank.noise_profile(0)).all()
            t = M.t_dec(n, W, H)
            if t < 0:
                assert np.isnan(prof).all()
                continue
            err = max(np.max(np.abs(prof[c] - thr[c][:, t])) for c in range(2))
            print(f"[adaptive] noise_profile memory {mem} learn {learn_s} after frame {t}: {err:.2e} dB from the model")
            assert err <= PROFILE_TOL
            if learn is not None and t >= learn - 1:
                assert held is None or np.array_equal(prof, held)     # bitwise constant once the window has passed
                held = prof
        assert (held is not None) == (learn is not None)
        bank.flush([1])
        assert np.isnan(bank.noise_profile(1)).all()
        bank.close()
    # the anchor: cumulative statistics, both floors idle -> the reference's threshold of the whole signal
    y = O.synth_signal(N, sr=sr, seed=21, dtype=np.float32)
    gate = nr.StreamGate(sr, noise_from_stream=True, n_fft=n_fft, win_length=W, hop_length=H, max_block=N)
    gate.push(y)
    want = O.noise_threshold_S(y[None].astype(np.float64), n_fft, W, H, 1.5, chunk_size=N)[0]
    T = (N + 2 * (W // 2) - W) // H + 1
    _, db = AM.spectrum(y.astype(np.float64), T, n_fft, W, H)
    # (the last frames of the whole signal see the zeros after it: the bank has them only at the flush, so compare on
    # the frames it has decided)
    t = M.t_dec(N, W, H)
    err = np.max(np.abs(gate.noise_profile()[0] - AM.recurrence(db[:, :t + 1])[1][:, -1]))
    assert err <= PROFILE_TOL
    assert np.max(np.abs(AM.recurrence(db)[1][:, -1] - want)) <= PROFILE_TOL
    gate.close()


def test_64_streams_and_bitwise_invariance():
    sr, n_fft, W, H = 16000, 512, 400, 160
    rng = np.random.default_rng(64)
    plans = {}
    for s in range(64):
        N = int(rng.integers(W + 10, 6000))
        cuts = [[], sorted(int(c) for c in rng.integers(0, N + 1, 5)), list(range(131, N, 131)), [N // 2, N // 2]][s % 4]
        plans[s] = (AM.swell(N, sr, 500 + s), cuts)
    kw = dict(noise_memory_s=0.25, noise_learn_s=0.1)
    bank = _mono(64, **kw)
    got = _run(bank, plans)
    y7 = plans[7][0]
    alone = _mono(1, **kw)
    a = _run(alone, {0: (y7, [])})[0]
    assert np.array_equal(a, got[7])
    again = _run(bank, {50: (y7, list(range(1, len(y7), 997))), 0: plans[3], 9: (plans[12][0], [17])}, as_tensor=True)
    assert np.array_equal(again[50], a) and np.array_equal(again[0], got[3]) and np.array_equal(again[9], got[12])
    # per-unit statistics: channel 0 of a stereo stream is the mono stream of that channel
    other = AM.swell(len(y7), sr, 777) * 3.0
    stereo = _mono(3, channels=2, **kw)
    st = _run(stereo, {2: (np.stack([y7, other]), [1000, 1001, 2500])})[2]
    assert np.array_equal(st[0], a)
    assert np.array_equal(st[1], _run(alone, {0: (other, [333])})[0])
    for b in (bank, alone, stereo):
        b.close()


def test_slot_is_clean_after_flush_reset_and_a_nan_stream():
    y = AM.swell(6000, 16000, 5)
    z = AM.swell(5000, 16000, 6) * 4.0
    fresh = _run(_mono(2, noise_memory_s=0.25), {1: (y, [])})[1]
    bank = _mono(2, noise_memory_s=0.25)
    _run(bank, {1: (z, [1000, 4000])})                       # another stream first: the flush clears the statistics
    assert np.array_equal(_run(bank, {1: (y, [1000, 1001, 4000])})[1], fresh)
    bad = z.copy()
    bad[2500] = np.nan
    dirty = _run(bank, {1: (bad, [3000])})[1]
    assert np.isnan(dirty).any()
    assert np.array_equal(_run(bank, {1: (y, [77])})[1], fresh)
    bank.push({1: bad[:3000]})
    bank.reset([1])
    assert np.isnan(bank.noise_profile(1)).all()
    assert np.array_equal(_run(bank, {1: (y, [])})[1], fresh)
    bank.push({1: z[:3000]})                                  # a finite stream, reset mid-way
    bank.reset([1])
    assert np.array_equal(_run(bank, {1: (y, [2999])})[1], fresh)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nonfinite_samples_mid_stream(bad):
    sr, n_fft, W, H = 16000, 512, 400, 160
    y = AM.swell(16000, sr, 3)
    y[7777] = bad
    ym = y.astype(np.float64)
    ym[7777] = np.nan           # an Inf sample is treated like a NaN
    n_fft_, W_, H_, nf, nt, smooth, _ = AM.geometry(sr, n_fft, W, H)
    for mem in (None, 0.25):
        model = np.concatenate(AM.adaptive_model([ym], n_fft_, W_, H_, 1.0, nf, nt, smooth,
                                                 lam=AM.forget_factor(mem, sr, H))[0])
        got = _run(_mono(1, noise_memory_s=mem), {0: (y, [1000, 7777, 7778, 12000])})[0]
        assert np.array_equal(np.isfinite(got), np.isfinite(model))
        ok = np.isfinite(model)
        assert (~ok).sum() >= 400
        assert np.max(np.abs(got[ok] - model[ok])) <= ORACLE_TOL * np.max(np.abs(model[ok]))
        # every band is gated from the first frame that saw it, forgetting or not
        assert np.max(np.abs(got[9000:])) == 0.0


def test_leading_digital_silence():
    sr, n_fft, W, H = 16000, 512, 400, 160
    n0 = sr // 5
    y = np.concatenate([np.zeros(n0, dtype=np.float32), AM.swell(sr, sr, 8)])
    n_fft_, W_, H_, nf, nt, smooth, _ = AM.geometry(sr, n_fft, W, H)
    model = np.concatenate(AM.adaptive_model([y.astype(np.float64)], n_fft_, W_, H_, 1.0, nf, nt, smooth)[0])
    got = _run(_mono(1), {0: (y, [1000, n0, n0 + 1, 9000])})[0]
    err = np.max(np.abs(got - model)) / np.max(np.abs(model))
    print(f"[adaptive] leading silence: {err:.2e} of peak against the model")
    assert err <= ORACLE_TOL
    assert np.all(got[:n0 - W] == 0.0)        # every sample whose frames lie wholly in the silence
    # (a zero spectrum gives zeros whatever the mask: what the gate made of the silence is in the profile.)  While every
    # decided frame is silent each band is constant: d = 0, M2 = 0, thr = mu = x = 20 log10(eps), the same bits in every
    # band; and cumulative or forgetting, held or not, it is the same number
    floor_db = 20 * np.log10(O.EPS64)
    for kw in (dict(), dict(noise_memory_s=0.25, noise_learn_s=0.05)):
        bank = _mono(1, **kw)
        for n in (1000, n0 - W):                  # two steps: the state is carried, every decided frame is silent
            bank.push({0: y[bank.received(0):n]})
            prof = bank.noise_profile(0)[0]
            assert np.all(prof == prof[0]) and abs(prof[0] - floor_db) <= PROFILE_TOL, (n, prof[:4], floor_db)
        bank.close()


def test_launches_per_step_do_not_depend_on_the_step():
    counts = []
    for S, n in ((3, 1), (64, 1), (3, 16000), (64, 16000)):
        bank = _mono(S, max_block=16000)
        x = {s: torch.from_numpy(O.synth_signal(n, sr=16000, seed=s, dtype=np.float32)).cuda() for s in range(S)}
        bank.push(x)
        g = bank.gate
        g.profile_enable(True)
        g.profile_read(reset=True)
        bank.push(x)
        counts.append({k: v[1] for k, v in g.profile_read(reset=True).items()})
        g.profile_enable(False)
        bank.close()
    assert all(c == counts[0] for c in counts), counts
    assert sum(counts[0].values()) == 4


def test_buffers_are_read_and_written_within_their_bounds():
    sr, W, H = 16000, 400, 160
    from noisereduce_amd import _ffi
    bank = _mono(3)
    bank._ensure()
    g, b = bank.gate, bank._bank
    y = O.synth_signal(5000, sr=sr, seed=8, dtype=np.float32)
    ref = _run(_mono(1), {0: (y, [])})[0]
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
    assert np.isfinite(ref).all()                      # the NaN guard bands around the blocks were never read
    with pytest.raises(ValueError, match="adaptive"):
        g.stream_set_threshold(b, [0], np.zeros(257))
    for forget, learn in ((0.0, -1), (1.5, -1), (float("nan"), -1), (0.5, 0)):
        with pytest.raises(ValueError, match="forget|learn_frames"):
            g.stream_create_adaptive(1, 1, 100, forget, learn)
    assert g.stream_state_bytes(3, 1, bank.max_block, adaptive=True) == bank.state_bytes


def test_a_fixed_profile_bank_next_to_an_adaptive_one():
    sr, n_fft, W, H = 16000, 512, 400, 160
    N = 9000
    y = O.synth_signal(N, sr=sr, seed=31, dtype=np.float32)
    noise = 0.1 * np.random.default_rng(7).standard_normal(3 * sr // 4)
    adaptive = _mono(2)
    adaptive.push({0: y[:4000]})
    kw = _kw(n_fft, W, H)
    fixed = stream.StreamBank(sr, 2, y_noise=noise, max_block=N, **kw)
    blocks = np.split(y, [1000, 4000, 4001])
    outs = []
    for i, blk in enumerate(blocks):                    # the two banks step in turn
        outs.append(fixed.push({1: blk})[1])
        adaptive.push({0: y[4000 + 100 * i:4100 + 100 * i]})
    outs.append(fixed.flush([1])[1])
    got = np.concatenate(outs)
    thresh = O.noise_threshold_S(noise[None], n_fft, W, H, 1.5, None, True)[0]
    assert np.max(np.abs(fixed.thresholds() - thresh)) <= 1e-9
    n_fft_, W_, H_, nf, nt, smooth, _ = M.geometry(sr, n_fft, W, H)
    model = np.concatenate(M.stream_model([y.astype(np.float64)], thresh, n_fft_, W_, H_, 1.0, nf, nt, smooth)[0])
    want = O.reduce_noise_S(y.astype(np.float64), sr, stationary=True, y_noise=noise, chunk_size=None, padding=0, **kw)
    dev = nr.reduce_noise(y=y, sr=sr, y_noise=noise, stationary=True, chunk_size=None, padding=0, device="cuda", **kw)
    peak = np.max(np.abs(want))
    e_or, e_mod, e_dev = (np.max(np.abs(got - r)) / peak for r in (want, model, dev))
    print(f"[adaptive] fixed-profile bank beside an adaptive one: oracle {e_or:.2e} device {e_dev:.2e} model {e_mod:.2e}")
    assert e_or <= ORACLE_TOL and e_mod <= ORACLE_TOL and e_dev <= DEVICE_TOL
    with pytest.raises(ValueError):
        fixed.noise_profile(1)
