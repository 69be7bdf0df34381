"""StreamBank(algorithm="torchgate") without a GPU: the float64 model of tests/stream_tg_model.py against the oracle
(O.torchgate_T and its stages), the argument checks (all before any library call), from_torchgate's parameter mapping,
the counters and the state bytes, and tests/stream_tg_plan_host.cpp, a stand-alone program around
noisereduce_amd/csrc/stream_plan.hpp that replays every ring access of random block splits."""
import os
import subprocess

import numpy as np
import pytest
import torch

from noisereduce_amd import _ffi, stream
from noisereduce_amd.torchgate import TorchGate
from oracle import spectralgate_oracle as O
from tests import stream_tg_model as M
from tests.test_onepass_plan_host import CXX, ROOT

SRC = os.path.join(ROOT, "tests", "stream_tg_plan_host.cpp")
GEOMS = [(256, 256, 64), (512, 400, 160), (1024, 1024, 256)]
KS = (1, 2, 7, 20)


def make_x(N, seed):
    """tests/gated_stft_cases.make_x's row: white noise, a tone and a ten times louder burst."""
    rng = np.random.default_rng(seed)
    s = np.arange(N)
    env = 1.0 + 9.0 * ((s >= int(0.40 * N)) & (s < int(0.52 * N)))
    return 0.1 * env * rng.standard_normal(N) + 0.5 * np.sin(2 * np.pi * 440.0 * s / 16000.0)


# ---- the model is the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1.0, 0.6])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%d-%d-%d" % g)
def test_model_equals_the_oracle(geom, K, p):
    n_fft, W, H = geom
    for N in (2 * W + 13, (K + 2 * 3 + 12) * H + 13):
        N = max(N, 2 * W + 13)
        x = make_x(N, seed=n_fft + K)
        kw = dict(n_fft=n_fft, win_length=W, hop_length=H, n_movemean_nonstationary=K, prop_decrease=p)
        want, st = O.torchgate_T(x[None], 16000, nonstationary=True, window=M.hann_float32(W), return_stages=True, **kw)
        got, mine = M.stream_tg_model(x, 16000, **kw)
        n = H * (N // H)
        assert want.shape == (1, n) and got.shape == (N,) and mine["mask"].shape == st["mask"][0].shape
        # float64 rounding: the oracle's box is a difference of cumulative sums, its smoothing and the model's an FFT
        # convolution; |X| reaches a few hundred here, so 1e-11 of the largest value is rounding and nothing else
        assert np.max(np.abs(np.abs(st["X"][0]) - mine["A"])) <= 1e-11 * np.max(mine["A"])
        assert np.max(np.abs(mine["raw"] - st["raw"][0])) <= 1e-11
        assert np.max(np.abs(mine["mask"] - st["mask"][0])) <= 1e-11
        assert np.max(np.abs(got[:n] - want[0])) <= 1e-11 * np.max(np.abs(want))
        assert np.all(np.isfinite(got[n:]))


def test_the_order_of_prop_decrease_and_smoothing_shows_at_the_edges():
    """TorchGate applies prop_decrease first and smooths with zero padding; the scipy gate smooths first.  At p = 0.6 the two
    differ at the time and frequency edges of the field by far more than any tolerance of the GPU tests: a bank that took
    the wrong order cannot pass them."""
    n_fft, W, H = 512, 400, 160
    x = make_x(6000, seed=3)
    _, st = O.torchgate_T(x[None], 16000, nonstationary=True, n_fft=n_fft, win_length=W, hop_length=H, prop_decrease=0.6,
                          window=M.hann_float32(W), return_stages=True)
    nf, nt, smooth = O.mask_smoothing_widths(16000, n_fft, H, 500, 50)
    assert smooth
    after = O.conv2_same(st["raw"][0], O.smoothing_filter(nf, nt)) * 0.6 + 0.4
    d = np.abs(after - st["mask"][0])
    assert d[0].max() > 1e-3 and d[-1].max() > 1e-3 and d[:, 0].max() > 1e-3 and d[:, -1].max() > 1e-3
    assert d[nf + 1:-nf - 1, nt + 1:-nt - 1].max() < 1e-12      # (the interior: the two orders agree)


def test_box_level_is_conv1d_same():
    A = np.random.default_rng(0).random((3, 11))
    for K in (1, 2, 3, 7, 11, 20, 30):
        want = torch.nn.functional.conv1d(torch.from_numpy(A)[:, None, :], torch.ones(1, 1, K, dtype=torch.float64) / K,
                                          padding="same")[:, 0].numpy()
        assert np.allclose(M.box_level(A, K), want, rtol=0, atol=1e-14), K
        assert np.allclose(O.boxcar_same(A, K), want, rtol=0, atol=1e-13), K


# ---- arguments --------------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_ffi, "Gate", boom)
    monkeypatch.setattr(_ffi, "load_library", boom)


TG = dict(algorithm="torchgate", stationary=False)


@pytest.mark.parametrize("kw", [
    dict(algorithm="torchgate"),                                   # stationary defaults to True
    dict(algorithm="torchgate", stationary=True),
    dict(TG, y_noise=np.zeros(4000)),
    dict(TG, thresholds_db=np.zeros(513)),
    dict(TG, noise_from_stream=True),
    dict(TG, lookahead_ms=20.0),
    dict(TG, time_constant_s=2.0),
    dict(TG, thresh_n_mult_nonstationary=2),
    dict(TG, sigmoid_slope_nonstationary=10),
    dict(TG, n_fft=512, win_length=401),
    dict(TG, n_movemean_nonstationary=0),
    dict(TG, n_movemean_nonstationary=-3),
    dict(TG, n_movemean_nonstationary=2.5),
    dict(TG, n_movemean_nonstationary=stream.MAX_LOOKAHEAD_FRAMES + 1),
    dict(TG, temp_coeff_nonstationary=0.0),
    dict(algorithm="torch"),
    dict(n_movemean_nonstationary=7),                              # TorchGate's parameters on the scipy gate
    dict(stationary=False, temp_coeff_nonstationary=0.2),
], ids=lambda kw: ",".join(f"{k}" for k in kw))
def test_constructor_errors_come_before_any_library_call(no_library, kw):
    with pytest.raises(ValueError):
        stream.StreamBank(16000, 2, **kw)


def test_refusals_of_a_bank_come_before_any_library_call(no_library):
    bank = stream.StreamBank(16000, 2, n_fft=512, **TG)
    z = np.zeros(100, dtype=np.float32)
    fb = np.ones((257, 4), dtype=np.float32)
    bank.set_filterbank(fb)
    bad = [lambda: bank.push_features({0: z}), lambda: bank.push_features({0: z}, scale="scipy"),
           lambda: bank.flush_features([0], scale="scipy"), lambda: bank.push_spectrum({0: z}),
           lambda: bank.flush_spectrum([0]), lambda: bank.snapshot([0]), lambda: bank.restore({}),
           lambda: bank.restore({0: None}), lambda: bank.state_bytes_of(0), lambda: bank.set_noise([0], thresholds_db=np.zeros(257)),
           lambda: bank.thresholds(), lambda: bank.noise_profile(0)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert bank._bank is None and bank._gate is None, i
    assert stream.StreamGate(16000, n_fft=512, **TG).bank.movemean == 20


def test_the_scipy_banks_are_what_they_were(no_library):
    """algorithm defaults to "scipy"; the None defaults of the scipy gate's parameters are its old values."""
    a = stream.StreamBank(16000, 2, n_fft=512, stationary=False, lookahead_ms=50.0)
    b = stream.StreamBank(16000, 2, n_fft=512, stationary=False, lookahead_ms=50.0, algorithm="scipy", time_constant_s=2.0,
                          thresh_n_mult_nonstationary=2, sigmoid_slope_nonstationary=10)
    assert a.algorithm == "scipy" and a.movemean == 0 and a._gate_kw == b._gate_kw and a.state_bytes == b.state_bytes
    assert a._gate_kw["variant"] == _ffi.SG_VARIANT_S and a._gate_kw["nonstat_thresh"] == 2 and a._gate_kw["nonstat_slope"] == 10
    assert a._gate_kw["iir_b"] == float(stream.iir_coefficient(2.0, 16000, 128))


def test_from_torchgate_reads_every_parameter(no_library):
    tg = TorchGate(sr=16000, nonstationary=True, n_thresh_nonstationary=1.7, temp_coeff_nonstationary=0.25,
                   n_movemean_nonstationary=7, prop_decrease=0.6, n_fft=512, win_length=400, hop_length=160,
                   freq_mask_smooth_hz=250, time_mask_smooth_ms=30)
    bank = stream.StreamBank.from_torchgate(tg, 3, channels=2, max_block=777, precision="float64")
    kw = bank._gate_kw
    nf, nt = tg._n_grad
    assert (bank.n_streams, bank.channels, bank.max_block, bank.exact, bank.algorithm) == (3, 2, 777, True, "torchgate")
    assert (bank.sr, bank.n_fft, bank.win_length, bank.hop_length, bank.movemean) == (16000, 512, 400, 160, 7)
    assert kw["variant"] == _ffi.SG_VARIANT_T and kw["stationary"] is False and kw["n_movemean"] == 7
    assert (kw["n_fft"], kw["win_length"], kw["hop_length"]) == (512, 400, 160)
    assert (kw["n_grad_freq"], kw["n_grad_time"], kw["smooth_mask"]) == (nf, nt, True) and bank.nt == nt
    assert kw["prop_decrease"] == 0.6 and kw["nonstat_thresh"] == 1.7 and kw["nonstat_slope"] == 1.0 / 0.25
    assert (kw["top_db"], kw["ddof"]) == (40.0, 1)                     # what TorchGate._gate_for passes
    assert np.array_equal(kw["window"], torch.hann_window(400).double().numpy())
    assert np.array_equal(kw["window"], M.hann_float32(400))
    plain = stream.StreamBank.from_torchgate(TorchGate(sr=16000, nonstationary=True, freq_mask_smooth_hz=None,
                                                       time_mask_smooth_ms=None), 1)
    assert plain._gate_kw["smooth_mask"] is False and plain.nt == 0 and plain.max_block == 16000 and not plain.exact
    with pytest.raises(ValueError):
        stream.StreamBank.from_torchgate(TorchGate(sr=16000), 1)


# ---- counters and bytes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_counters_follow_the_definition(no_library, K):
    lo, L = (K - 1) // 2, K - 1 - (K - 1) // 2
    assert stream.box_frames(K) == (lo, L) and lo + L + 1 == K and 0 <= L - lo <= 1
    for n_fft, W, H in GEOMS:
        for smooth in (True, False):
            bank = stream.StreamBank(16000, 2, n_fft=n_fft, win_length=W, hop_length=H, n_movemean_nonstationary=K,
                                     freq_mask_smooth_hz=500 if smooth else None, time_mask_smooth_ms=50 if smooth else None,
                                     max_block=3000, **TG)
            nt = int(50 / (H / 16000 * 1000)) if smooth else 0
            assert bank.lookahead_frames == L and bank.nt == nt and bank._lag == nt + L
            assert bank.latency_samples == W + (nt + L + 1) * H
            for n in (0, W // 2 - 1, W // 2, W, W + (nt + L) * H - 1, W + (nt + L) * H, 5 * W + 17):
                bank._n[0] = n
                td = (n + W // 2 - W) // H if n + W // 2 - W >= 0 else -1
                assert bank.frames(0) == max(0, td - nt - L + 1)
                assert stream.emitted(n, W, H, bank._lag) == max(0, (td - nt - L + 1) * H - W // 2)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stream_tg_plan") / "stream_tg_plan_host")
    base = [CXX, "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", path]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:   # (a compiler without the sanitizer runtimes)
        subprocess.run(base, check=True)
    return path


def _plan(exe, n_fft, W, H, nt, K, C, exact, n_slots, max_block, seed):
    r = subprocess.run([exe] + [str(v) for v in (n_fft, W, H, nt, K, C, int(exact), n_slots, max_block, seed)],
                       capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().split("\n")
    assert r.returncode == 0 and lines[-1].startswith("ok "), (r.returncode, lines[-3:], r.stderr[-2000:])
    geo = [int(v) for v in lines[0].split()[1:]]
    lay = [int(v) for v in lines[1].split()[1:]]
    return geo, lay, [int(v) for v in lines[-1].split()[1:]]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%d-%d-%d" % g)
def test_ring_depths_and_state_bytes(exe, geom, K):
    """The header's layout of a box bank against the rule (RF = L + Lb + 1 + max_frames rows of A alone, no forward level)
    and against stream.state_bytes; an existing kind's bytes are not its concern (tests/test_stream_plan_host.py)."""
    n_fft, W, H = geom
    lo, L = stream.box_frames(K)
    F = n_fft // 2 + 1
    FS = (F + 15) // 16 * 16
    for nt, C, exact, n_slots, max_block in ((0, 1, False, 1, 1), (2, 1, False, 3, 300), (3, 2, True, 2, 1600)):
        (gL, gLb, gRC), (RC, RB, RF, mf, fst, fa, mk, total), _ = _plan(exe, n_fft, W, H, nt, K, C, exact, n_slots, max_block, 1)
        assert (gL, gLb) == (L, lo) and gRC == RC == W + (nt + L + 1) * H
        assert mf == (max_block + W // 2) // H + 3 and RF == L + lo + 1 + mf and RB == 2 * nt + 1 + L + mf
        nu = n_slots * C
        assert fst == 0 and fa == nu * RF * FS * 8 and mk == nu * RB * FS * (8 if exact else 4)
        assert total == nu * (RC * 8 + 2 * W * 8) + fa + mk
        assert total == stream.state_bytes(nu, n_fft, W, H, nt, L, max_block, False, False, exact, movemean=K)
    # against the existing non-stationary bank at the same lookahead: Lb rows more, each half as wide, and no fst
    ns = stream.state_bytes(1, n_fft, W, H, 2, L, 300, False)
    mf = (300 + W // 2) // H + 3
    assert stream.state_bytes(1, n_fft, W, H, 2, L, 300, False, movemean=K) == ns - FS * 8 - (L + 1 + mf) * FS * 8 + lo * FS * 8


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%d-%d-%d" % g)
def test_every_row_a_step_reads_is_still_in_its_ring(exe, geom, K):
    """Random block splits with 0-length blocks, single samples, whole max_block blocks, several slots per step, a flush with
    and without a last block and a second stream on the flushed slot: the program replays the decide and smoothing launches'
    ring accesses and fails on the first row that is no longer the one asked for."""
    n_fft, W, H = geom
    reads = 0
    for seed, (nt, C, n_slots, max_block) in enumerate(((0, 1, 2, 1), (2, 1, 3, 37), (3, 2, 2, 3 * H + 5), (1, 1, 4, 8 * W))):
        _, _, (n, steps) = _plan(exe, n_fft, W, H, nt, K, C, False, n_slots, max_block, 100 * K + seed)
        assert steps > 0
        reads += n
    assert reads > 1000
