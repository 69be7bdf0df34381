"""StreamBank without a GPU: the emission arithmetic, the float64 model against the offline oracle, the C ABI surface and
argument checks (all of which happen before any device work)."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import stream_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (sr, n_fft, win_length, hop_length, prop_decrease, samples)
GEOMS = [(48000, 1024, None, None, 1.0, 60000), (16000, 512, 400, 160, 0.8, 30001), (8000, 256, None, 50, 1.0, 9000),
         (44100, 2048, 1500, 333, 0.6, 70000), (48000, 4096, None, None, 1.0, 80000)]


@pytest.mark.parametrize("sr,n_fft,W,H,p,N", GEOMS)
def test_emitted_is_the_models_count(sr, n_fft, W, H, p, N):
    from noisereduce_amd import stream
    n_fft, W, H, nf, nt, smooth, ntl = M.geometry(sr, n_fft, W, H)
    prev = 0
    for n in range(0, 3 * W + 40 * H + 1):
        e = stream.emitted(n, W, H, ntl)
        assert e == M.emitted(n, W, H, ntl)
        assert prev <= e <= n
        prev = e
    for n_tot in (W, W + 1, 3 * W + 7, 3 * W + 40 * H):
        # pushes of 131 samples, then the flush: the lengths sum to the stream's length
        got, e = 0, 0
        for n in list(range(131, n_tot, 131)) + [n_tot]:
            e2 = stream.emitted(n, W, H, ntl)
            got += e2 - e
            e = e2
        assert got + (n_tot - e) == n_tot
    assert stream.emitted(0, W, H, ntl) == 0
    bank = stream.StreamBank(sr, 2, thresholds_db=np.zeros(n_fft // 2 + 1), n_fft=n_fft, win_length=W, hop_length=H)
    assert bank.latency_samples == W + (ntl + 1) * H
    for n in range(0, 3 * W + 40 * H + 1, 17):   # the documented delay bound
        assert n - stream.emitted(n, W, H, ntl) < bank.latency_samples


@pytest.mark.parametrize("sr,n_fft,W,H,p,N", GEOMS)
def test_model_is_the_offline_gate_for_every_block_split(sr, n_fft, W, H, p, N):
    rng = np.random.default_rng(N)
    y = O.synth_signal(N, sr=sr, seed=N).astype(np.float64)
    noise = 0.1 * rng.standard_normal(3 * sr // 4)
    n_fft_, W_, H_, nf, nt, smooth, ntl = M.geometry(sr, n_fft, W, H)
    thresh, _, _ = O.noise_threshold_S(noise[None], n_fft_, W_, H_, 1.5, None, True)
    want = O.reduce_noise_S(y, sr, stationary=True, y_noise=noise, prop_decrease=p, chunk_size=None, padding=0,
                            n_fft=n_fft, win_length=W, hop_length=H)
    peak = np.max(np.abs(want))
    plans = {"whole": (y, []), "cuts": (y, sorted(rng.integers(0, N, 9))), "131": (y, list(range(131, N, 131)))}
    for name, (sig, cuts) in plans.items():
        ref = want
        outs, live = M.stream_model(np.split(sig, cuts), thresh, n_fft_, W_, H_, p, nf, nt, smooth)
        assert live is False
        got = np.concatenate(outs)
        assert got.shape == sig.shape
        err = np.max(np.abs(got - ref)) / peak
        print(f"[stream model] {sr} {n_fft} {name}: {err:.2e} of peak")
        assert err <= 1e-12, (name, err)


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from noisereduce_amd import _ffi
    header = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    lib = _ffi.load_library()
    names = ("sg_stream_create", "sg_stream_destroy", "sg_stream_set_threshold", "sg_stream_push", "sg_stream_reset",
             "sg_stream_emitted", "sg_stream_counters")
    for name in names:
        assert re.search(r"SG_API int %s\(" % name, header), name
        assert name in _ffi.exported_symbols()
        assert hasattr(lib, name)
    assert _ffi.SG_N_STAGES == 27
    assert lib.sg_version() == 100
    # struct sg_stream_rec: field order and size as the header states them
    body = header[header.index("typedef struct sg_stream_rec {"):header.index("} sg_stream_rec;")]
    fields = re.findall(r"^\s*(?:int32_t|int64_t)\s+(\w+);", body, flags=re.M)
    assert fields == [f[0] for f in _ffi.SgStreamRec._fields_]
    assert ctypes.sizeof(_ffi.SgStreamRec) == 48
    import noisereduce_amd as nr
    assert nr.StreamBank is not None and nr.StreamGate is not None


def test_arguments_are_checked_before_any_device_work():
    from noisereduce_amd import stream
    thr = np.zeros(513)
    with pytest.raises(ValueError):
        stream.StreamBank(48000, 2, thresholds_db=thr, n_fft=400)
    with pytest.raises(ValueError):
        stream.StreamBank(48000, 2, thresholds_db=thr, stationary=False)
    with pytest.raises(ValueError):
        stream.StreamBank(48000, 2, thresholds_db=np.zeros(100))
    with pytest.raises(ValueError):
        stream.StreamBank(48000, 2, y_noise=np.zeros(100))          # noise clip shorter than a window
    bank = stream.StreamBank(48000, 2, thresholds_db=thr, max_block=4800)
    assert bank._bank is None                                         # nothing touched the device so far
    bad = [lambda: bank.push({2: np.zeros(10, np.float32)}), lambda: bank.push({-1: np.zeros(10, np.float32)}),
           lambda: bank.push({0: np.zeros(4801, np.float32)}), lambda: bank.push({0: np.zeros(10, np.int16)}),
           lambda: bank.push({0: np.zeros((2, 10), np.float32)}), lambda: bank.flush([0]),
           lambda: bank.flush([0], {0: np.zeros(1023, np.float32)}), lambda: bank.flush([5]),
           lambda: bank.set_noise([0], thresholds_db=np.zeros(3)), lambda: bank.reset([7])]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    assert bank._bank is None
    nobody = stream.StreamBank(48000, 1)
    with pytest.raises(ValueError):
        nobody.push({0: np.zeros(10, np.float32)})                    # no noise profile yet
