"""The non-stationary StreamBank without a GPU: the float64 model against the offline oracle and against the contract's
recursion, the emission arithmetic with a lookahead, the C ABI surface, and argument checks (all before any device work)."""
import os
import re

import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import stream_ns_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (sr, n_fft, win_length, hop_length, prop_decrease, samples, time_constant_s)
GEOMS = [(48000, 1024, None, None, 1.0, 30000, 2.0), (16000, 512, 400, 160, 0.8, 12001, 0.1),
         (8000, 256, None, 50, 1.0, 4000, 0.5), (44100, 2048, 1500, 333, 0.6, 30000, 2.0)]


def _model(y, cuts, sr, n_fft, W, H, p, tc, L, **kw):
    n_fft_, W_, H_, nf, nt, smooth, _ = M.geometry(sr, n_fft, W, H)
    b = O.iir_coefficient(tc, sr, H_)
    return np.concatenate(M.stream_ns_model(np.split(y, cuts), n_fft_, W_, H_, p, nf, nt, smooth, b, L, **kw))


@pytest.mark.parametrize("sr,n_fft,W,H,p,N,tc", GEOMS)
def test_model_is_the_offline_gate_when_the_lookahead_covers_the_stream(sr, n_fft, W, H, p, N, tc):
    rng = np.random.default_rng(N)
    y = O.synth_signal(N, sr=sr, seed=N).astype(np.float64)
    n_fft_, W_, H_ = O.resolve_stft_params(n_fft, W, H)
    T = (N + 2 * (W_ // 2) - W_) // H_ + 1
    want = O.reduce_noise_S(y, sr, stationary=False, prop_decrease=p, time_constant_s=tc, chunk_size=None, padding=0,
                            n_fft=n_fft, win_length=W, hop_length=H)
    peak = np.max(np.abs(want))
    e = W_ + 2 * H_ - W_ // 2          # the sample that completes frame 2: one-sample and empty blocks around it
    plans = {"whole": [], "cuts": sorted(int(c) for c in rng.integers(0, N, 5)), "strided": list(range(997, N, 997)),
             "edge": [e - 2, e - 1, e, e, e, e + 1, N // 2, N // 2, N - 1]}
    for name, cuts in plans.items():
        for L in (T - 1, T + 40):
            got = _model(y, cuts, sr, n_fft, W, H, p, tc, L)
            assert got.shape == y.shape
            err = np.max(np.abs(got - want)) / peak
            print(f"[stream-ns model] {sr} {n_fft} {name} L={L}: {err:.2e} of peak")
            assert err <= 1e-12, (name, L, err)


def test_recursion_is_the_oracles_smoother_of_the_signal_known_L_frames_later():
    rng = np.random.default_rng(3)
    A = np.abs(rng.standard_normal((5, 60)))
    b = O.iir_coefficient(0.1, 16000, 160)
    fwd = M.forward_pass(b, A)
    full = O.filtfilt_onepole(b, A)
    for L in (59, 60, 1000):                 # unbounded lookahead: bit for bit the offline smoother
        assert np.array_equal(M.smoothed_level(b, fwd, L), full)
    for L in (0, 1, 7, 30):
        S = M.smoothed_level(b, fwd, L)
        for t in range(60):
            e = min(t + L, 59)
            assert np.array_equal(S[:, t], O.filtfilt_onepole(b, A[:, :e + 1])[:, t]), (L, t)


@pytest.mark.parametrize("L", [0, 3, 8])
def test_model_does_not_depend_on_the_block_split(L):
    sr, n_fft, W, H, N = 16000, 512, 400, 160, 9000
    y = O.synth_signal(N, sr=sr, seed=21).astype(np.float64)
    whole = _model(y, [], sr, n_fft, W, H, 1.0, 0.1, L, direct=True)
    rng = np.random.default_rng(L)
    e = W + 3 * H - W // 2
    for cuts in (list(range(131, N, 131)), sorted(int(c) for c in rng.integers(0, N, 9)), [e - 1, e, e, e + 1, N - 1, N]):
        got = _model(y, cuts, sr, n_fft, W, H, 1.0, 0.1, L, direct=True)
        assert np.max(np.abs(got - whole)) <= 1e-13 * np.max(np.abs(whole)), cuts[:4]


def test_error_against_offline_does_not_increase_with_the_lookahead():
    sr, n_fft, W, H = 16000, 512, 400, 160
    y = O.synth_signal(2 * sr, sr=sr).astype(np.float64)
    assert (len(y) + 2 * (W // 2) - W) // H + 1 == 201
    want = O.reduce_noise_S(y, sr, stationary=False, time_constant_s=0.1, chunk_size=None, padding=0, n_fft=n_fft,
                            win_length=W, hop_length=H)
    peak = np.max(np.abs(want))
    errs = []
    for L in (0, 8, 32, 128, 200):
        errs.append(np.max(np.abs(_model(y, [5000, 20000], sr, n_fft, W, H, 1.0, 0.1, L) - want)) / peak)
        print(f"[stream-ns model] L={L}: {errs[-1]:.2e} of the offline output's peak")
    assert all(a >= b for a, b in zip(errs, errs[1:])), errs
    assert errs[0] > 1e-2 and errs[3] < 1e-5 and errs[4] <= 1e-12, errs


def test_latency_and_emitted_add_the_lookahead_to_nt():
    from noisereduce_amd import stream
    for sr, n_fft, W, H, ms in ((16000, 512, 400, 160, 100.0), (48000, 1024, None, None, 100.0), (48000, 1024, None, None, 0.0),
                                (8000, 256, None, 50, 33.0)):
        n_fft_, W_, H_, nf, nt, smooth, ntl = M.geometry(sr, n_fft, W, H)
        L = int(ms / (H_ / sr * 1000))
        bank = stream.StreamBank(sr, 3, stationary=False, n_fft=n_fft, win_length=W, hop_length=H, lookahead_ms=ms)
        assert bank._bank is None
        assert bank.lookahead_frames == L and bank.nt == ntl
        assert bank.latency_samples == W_ + (ntl + L + 1) * H_
        prev = 0
        for n in range(0, 3 * W_ + (40 + L) * H_ + 1, 7):
            e = stream.emitted(n, W_, H_, ntl + L)
            assert e == M.emitted(n, W_, H_, ntl + L) and prev <= e <= n
            assert n - e < bank.latency_samples
            prev = e
    off = stream.StreamBank(16000, 1, stationary=False, n_fft=512, freq_mask_smooth_hz=None, time_mask_smooth_ms=None,
                            lookahead_ms=25.0, hop_length=160, win_length=400)
    assert off.nt == 0 and off.lookahead_frames == 2 and off.latency_samples == 400 + 3 * 160


def test_a_non_stationary_bank_is_constructed_without_a_noise_profile():
    import noisereduce_amd as nr
    from noisereduce_amd import stream
    bank = stream.StreamBank(48000, 4, stationary=False)
    assert bank.stationary is False and bank.lookahead_frames == 0 and bank._bank is None
    assert bank.latency_samples == 1024 + (bank.nt + 1) * 256
    gate = nr.StreamGate(16000, stationary=False, n_fft=512, lookahead_ms=100.0, time_constant_s=0.1)
    assert gate.bank.lookahead_frames == 12 and gate.latency_samples == gate.bank.latency_samples
    assert stream.StreamBank(48000, 1).stationary is True          # the default stays the stationary gate


def test_arguments_are_checked_before_any_device_work():
    from noisereduce_amd import stream
    thr = np.zeros(513)
    bad_ctor = [dict(thresholds_db=thr), dict(y_noise=np.zeros(48000)), dict(lookahead_ms=-1.0), dict(n_fft=400),
                dict(lookahead_ms=float("nan")), dict(lookahead_ms=float("inf")), dict(time_constant_s=0.0), dict(max_block=0),
                dict(lookahead_ms=4097 * 256 / 48.0, max_state_bytes=1 << 50)]     # more frames than the library takes
    for kw in bad_ctor:
        with pytest.raises(ValueError):
            stream.StreamBank(48000, 2, stationary=False, **kw)
    with pytest.raises(ValueError):
        stream.StreamBank(48000, 2, thresholds_db=thr, lookahead_ms=10.0)     # a lookahead on the stationary gate
    # a lookahead whose state would not fit: the error names the size
    with pytest.raises(ValueError) as ei:
        stream.StreamBank(48000, 1024, stationary=False, lookahead_ms=60000.0)
    need = stream.state_bytes(1024, 1024, 1024, 256, 9, int(60000.0 / (256 / 48000 * 1000)), 48000, False)
    assert str(need) in str(ei.value) and need > stream.MAX_STATE_BYTES
    with pytest.raises(ValueError) as ei:
        stream.StreamBank(48000, 2, stationary=False, lookahead_ms=100.0, max_state_bytes=1 << 20)
    assert "bytes" in str(ei.value)
    bank = stream.StreamBank(48000, 2, stationary=False, max_block=4800, lookahead_ms=100.0)
    assert bank.state_bytes == stream.state_bytes(2, 1024, 1024, 256, 9, 18, 4800, False)
    bad = [lambda: bank.push({2: np.zeros(10, np.float32)}), lambda: bank.push({0: np.zeros(4801, np.float32)}),
           lambda: bank.push({0: np.zeros(10, np.int16)}), lambda: bank.push({0: np.zeros((2, 10), np.float32)}),
           lambda: bank.flush([0]), lambda: bank.flush([0], {0: np.zeros(1023, np.float32)}), lambda: bank.flush([5]),
           lambda: bank.set_noise([0], thresholds_db=thr), lambda: bank.set_noise([0], y_noise=np.zeros(48000)),
           lambda: bank.thresholds(), lambda: bank.reset([7])]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert bank._bank is None                                         # nothing touched the device


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from noisereduce_amd import _ffi
    header = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    lib = _ffi.load_library()
    for name in ("sg_stream_create_nonstationary", "sg_stream_state_bytes", "sg_stream_bank_emitted"):
        assert re.search(r"SG_API int %s\(" % name, header), name
        assert name in _ffi.exported_symbols()
        assert hasattr(lib, name)
    assert _ffi.SG_N_STAGES == 27
    assert lib.sg_version() == 100
    import ctypes
    assert ctypes.sizeof(_ffi.SgStreamRec) == 48
