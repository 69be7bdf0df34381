"""CPU checks of reduce_noise_batch's planner: the unit table is the reference's chunk grid per clip, routing follows the
batched kernels' coverage, argument errors name the clip, and the new C-ABI symbols are declared and exported."""
import os
import re

import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from noisereduce_amd import batch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _oracle_windows(n, cs, pad):
    """(i1, i2, kept start, kept end) of every window reduce_noise_S filters (base.py:152-222)."""
    if cs is not None and n > cs:
        return [(i * cs - pad, (i + 1) * cs + pad, i * cs, min((i + 1) * cs, n)) for i in range(int((n - 1) / cs) + 1)]
    return [(-pad, n + pad, 0, n)]


@pytest.mark.parametrize("cs,pad", [(1000, 300), (1000, 0), (None, 200), (4096, 1024)])
def test_units_match_the_oracle_chunk_grid(cs, pad):
    rng = np.random.default_rng(3)
    lens = [300, 999, 1000, 1001, 2000, 2001] + [int(v) for v in rng.integers(260, 9000, 12)]
    if cs is None:
        lens = [max(v, 256) for v in lens]
    ys = [np.zeros((1 + i % 2, n) if i % 3 == 0 else n, np.float32) for i, n in enumerate(lens)]
    p = batch.plan(ys, 16000, chunk_size=cs, padding=pad, n_fft=256)
    assert p.routes == [batch.BATCHED] * len(ys)
    for i, (y, n) in enumerate(zip(ys, lens)):
        C = 1 if y.ndim == 1 else y.shape[0]
        units = [u for u in p.units if u.clip == i]
        wins = _oracle_windows(n, cs, pad)
        assert len(units) == C * len(wins)
        for c in range(C):
            uc = [u for u in units if u.channel == c]
            covered = []
            for u, (i1, i2, s, e) in zip(uc, wins):
                chunk = O.read_chunk(np.arange(1, n + 1, dtype=np.float64)[None, :], i1, i2)
                assert u.win0 == i1 and u.Lp == i2 - i1 == chunk.shape[1]
                assert u.T == O.n_frames_for(u.Lp, 256, 64)
                assert u.out0 == s and u.k1 - u.k0 == e - s and u.k0 == pad
                covered.extend(range(u.out0, u.out0 + u.k1 - u.k0))
            assert covered == list(range(n))      # every output sample exactly once, no gap


def test_every_clip_appears_once_in_order():
    ys = [np.zeros(n, np.float32) for n in (5000, 700, 12000, 3000)]
    p = batch.plan(ys, 16000, chunk_size=4000, padding=200)
    clips = [u.clip for u in p.units]
    assert sorted(set(clips)) == [0, 1, 2, 3] and clips == sorted(clips)


def test_routing():
    f32, f64 = np.zeros(3000, np.float32), np.zeros(3000, np.float64)
    i16, i32 = np.zeros(3000, np.int16), np.zeros(3000, np.int32)
    for nfft in (256, 512, 1024, 2048, 4096):
        assert batch.plan([f32, f64], 16000, n_fft=nfft, padding=5000).routes == [batch.BATCHED] * 2
    assert batch.plan([f32], 16000, n_fft=1000).routes == [batch.FALLBACK]
    assert batch.plan([f32], 16000, n_fft=128).routes == [batch.FALLBACK]
    assert batch.plan([f32], 16000, n_fft=8192).routes == [batch.FALLBACK]
    assert batch.plan([f32], 16000, precision="float64").routes == [batch.FALLBACK]
    assert batch.plan([i16, i32], 16000, fast_int=False).routes == [batch.FALLBACK] * 2
    assert batch.plan([i16, i32], 16000, fast_int=True).routes == [batch.BATCHED] * 2
    p = batch.plan([f32], 16000, win_length=700, hop_length=123, chunk_size=None, padding=0, stationary=True)
    assert p.routes == [batch.BATCHED] and (p.win_length, p.hop_length) == (700, 123)


def test_argument_errors_name_the_clip():
    good = np.zeros(3000, np.float32)
    with pytest.raises(ValueError, match="clip 1"):
        batch.plan([good, np.zeros((2, 2, 10), np.float32)], 16000)
    with pytest.raises(ValueError, match="clip 2"):
        batch.plan([good, good, np.zeros(100, np.float32)], 16000, padding=0)
    with pytest.raises(ValueError, match="TorchGate"):
        batch.reduce_noise_batch([good], 16000, use_torch=True)


def test_noise_forms():
    ys = [np.zeros(3000, np.float32)] * 3
    assert [u.noise for u in batch.plan(ys, 16000, stationary=True).units] == [0, 1, 2]
    assert [u.noise for u in batch.plan(ys, 16000, stationary=True, y_noise=np.zeros(2000)).units] == [0, 0, 0]
    yn = [None, np.zeros(2000), None]
    assert [u.noise for u in batch.plan(ys, 16000, stationary=True, y_noise=yn).units] == [0, 1, 2]
    # a list is always per-clip noise; a tuple / array / tensor is one shared noise clip
    with pytest.raises(ValueError, match="one entry per clip"):
        batch.plan(ys, 16000, stationary=True, y_noise=[np.zeros(2000)] * 2)
    shared = (np.zeros(2000), np.zeros(2000), np.zeros(2000))   # three channels of ONE noise clip
    assert [u.noise for u in batch.plan(ys, 16000, stationary=True, y_noise=shared).units] == [0, 0, 0]


def test_new_symbols_declared_and_bound():
    from noisereduce_amd import _ffi
    header = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    debug = open(os.path.join(ROOT, "include", "mi355gate_debug.h")).read()
    for name in ("sg_process_clips", "sg_clips_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _ffi.exported_symbols()
    for name in ("sg_debug_clip_thresholds", "sg_debug_clip_batches"):
        assert re.search(r"\b%s\s*\(" % name, debug)
        assert name in _ffi.exported_symbols()
    n = int(re.search(r"#define SG_N_STAGES (\d+)", debug).group(1))
    assert n == _ffi.SG_N_STAGES == 27
    import ctypes
    assert ctypes.sizeof(_ffi.SgClip) == 48 and ctypes.sizeof(_ffi.SgNoiseSrc) == 32
    assert len(_ffi._PROTOTYPES["sg_clips_workspace_bytes"][1]) == 6   # handle, noise table, n_noise, clips, n_clips, out
