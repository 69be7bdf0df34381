"""StreamBank(noise_from_stream=True) without a GPU: the float64 model of the running noise statistics against the
reference's whole-recording threshold and against directly computed weighted moments, the properties that follow from the
recurrence, the conditions the GPU tests' inputs must meet, the C ABI surface and the argument checks (all of which happen
before any device work)."""
import os
import re

import numpy as np
import pytest

from oracle import spectralgate_oracle as O
from tests import stream_adaptive_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(y, sr, n_fft, W, H, lam=1.0, learn=None, n_std=1.5):
    n_fft, W, H = O.resolve_stft_params(n_fft, W, H)
    y = np.asarray(y, dtype=np.float64)
    T = (len(y) + 2 * (W // 2) - W) // H + 1
    _, db = AM.spectrum(y, T, n_fft, W, H)
    return (db,) + AM.recurrence(db, n_std, lam, learn)


@pytest.mark.parametrize("geom", [(48000, 1024, None, None), (16000, 512, 400, 160)], ids=lambda g: "%d-%d" % g[:2])
def test_anchor_is_the_references_threshold_of_the_whole_signal(geom):
    sr, n_fft, W, H = geom
    n_fft_, W_, H_ = O.resolve_stft_params(n_fft, W, H)
    y = O.synth_signal(int(1.5 * sr), sr=sr, seed=21).astype(np.float64)
    db, x, thr, raw = _fields(y, sr, n_fft, W, H)
    assert np.max(db.max(axis=1) - db.min(axis=1)) < 80.0          # no band's range reaches top_db: both floors idle
    assert np.array_equal(x, db)
    want = O.noise_threshold_S(y[None], n_fft_, W_, H_, 1.5, chunk_size=len(y))[0]
    assert db.shape[1] == O.n_frames_for(len(y), W_, H_)
    err = np.max(np.abs(thr[:, -1] - want))
    print(f"[adaptive model] anchor {geom}: {err:.2e} dB from noise_threshold_S")
    assert err <= 1e-9
    # and through the streaming model, whatever the block split
    _, _, _, nf, nt, smooth, _ = AM.geometry(sr, n_fft, W, H)
    for cuts in ([], list(range(997, len(y), 997))):
        _, thr2, raw2 = AM.adaptive_model(np.split(y, cuts), n_fft_, W_, H_, 1.0, nf, nt, smooth)
        assert np.array_equal(thr2, thr) and np.array_equal(raw2, raw)


@pytest.mark.parametrize("memory_s", [None, 0.25])
def test_recurrence_is_the_weighted_mean_and_deviation(memory_s):
    sr, n_fft, W, H = 16000, 512, 400, 160
    y = AM.swell(int(1.2 * sr), sr, 5)
    lam = AM.forget_factor(memory_s, sr, H)
    assert (lam == 1.0) == (memory_s is None) and 0.0 < lam <= 1.0
    db, x, thr, _ = _fields(y, sr, n_fft, W, H, lam=lam)
    T = x.shape[1]
    worst = 0.0
    for t in range(T):
        w = lam ** np.arange(t, -1, -1.0)
        mean = (x[:, :t + 1] * w).sum(axis=1) / w.sum()
        var = (w * (x[:, :t + 1] - mean[:, None]) ** 2).sum(axis=1) / w.sum()
        worst = max(worst, np.max(np.abs(thr[:, t] - (mean + 1.5 * np.sqrt(var)))))
    print(f"[adaptive model] recurrence, noise_memory_s={memory_s}: {worst:.2e} dB from the direct moments")
    assert worst <= 1e-10


def test_learn_window_holds_the_profile():
    sr, n_fft, W, H = 16000, 512, 400, 160
    y = AM.swell(int(1.2 * sr), sr, 6)
    L = AM.learn_frames(0.3, sr, H)
    assert L == 30
    for lam in (1.0, AM.forget_factor(0.25, sr, H)):
        _, x, thr, _ = _fields(y, sr, n_fft, W, H, lam=lam, learn=L)
        assert np.all(thr[:, L - 1:] == thr[:, L - 1:L])
        _, _, free, _ = _fields(y, sr, n_fft, W, H, lam=lam)
        assert np.array_equal(free[:, :L], thr[:, :L]) and not np.array_equal(free[:, L:], thr[:, L:])


def test_frame_zero_and_constant_bands_are_gated_exactly():
    rng = np.random.default_rng(3)
    db = -40.0 + 10.0 * rng.standard_normal((6, 50))
    db[2, :] = -37.123456789
    db[4, :20] = 20 * np.log10(O.EPS64)                      # leading digital silence, then a signal
    for lam in (1.0, 0.9):
        x, thr, raw = AM.recurrence(db, lam=lam)
        assert np.array_equal(thr[:, 0], x[:, 0]) and not raw[:, 0].any()
        assert np.all(thr[2] == x[2]) and not raw[2].any()
        assert np.all(thr[4, :20] == x[4, :20]) and not raw[4, :20].any()
    db[1, 25] = np.nan                                        # a non-finite frame: the band stays gated, forgetting or not
    for lam in (1.0, 0.9):
        x, thr, raw = AM.recurrence(db, lam=lam)
        assert not raw[1, 25:].any() and np.isnan(thr[1, 25:]).all() and raw[[0, 3, 5]].any()


def _parity_cases():
    for geom in AM.GEOMS:
        for mem in AM.MEMORY_S:
            for ls in AM.LEARN_S:
                for ch in (0, 1):
                    yield geom, mem, ls, ch


@pytest.mark.parametrize("geom", AM.GEOMS, ids=lambda g: "%d-%d" % g[:2])
def test_gpu_inputs_meet_the_input_conditions(geom):
    """The share of passing cells, the movement of the threshold and the distance of every cell from its threshold, on
    the model alone: a GPU failure on these inputs is not the inputs' doing."""
    sr, n_fft, W, H = geom
    for g, mem, ls, ch in _parity_cases():
        if g != geom:
            continue
        y = AM.swell(AM.parity_length(geom), sr, AM.parity_seed(geom, ch))
        lam, L = AM.forget_factor(mem, sr, H), AM.learn_frames(ls, sr, H)
        _, x, thr, raw = _fields(y, sr, n_fft, W, H, lam=lam, learn=L)
        share = raw.mean()
        moved = np.mean((thr[:, 1:].max(axis=1) - thr[:, 1:].min(axis=1)) > 1.0)
        margin = AM.margin_db(x, thr)
        print(f"[adaptive inputs] {geom} memory {mem} learn {ls} ch {ch}: {100 * share:.1f} % pass, threshold moves > 1 dB "
              f"in {100 * moved:.0f} % of the bands, nearest cell {margin:.2e} dB")
        assert 0.05 <= share <= 0.95
        assert moved >= 0.5
        assert margin > 1e-9
        if L is not None:
            assert 1 <= L < x.shape[1] - 1
    if n_fft in (1024, 512):         # the per-hop-block inputs
        for quiet_first, _ in AM.TWO_LEVEL:
            y = AM.two_level(sr, sr, quiet_first=quiet_first)
            _, x, thr, raw = _fields(y, sr, n_fft, W, H)
            T = raw.shape[1]
            print(f"[adaptive inputs] {geom} two-level, quiet first {quiet_first}: nearest cell {AM.margin_db(x, thr):.2e} "
                  f"dB, {100 * raw[:, :T // 2].mean():.1f} % / {100 * raw[:, T // 2:].mean():.1f} % pass per half")
            assert AM.margin_db(x, thr) > 1e-9
            if quiet_first:
                assert raw[:, :T // 2 - 4].mean() > 0.01 and raw[:, T // 2 + 4:].mean() > 0.1   # both halves pass cells


def test_model_does_not_depend_on_the_block_split():
    sr, n_fft, W, H = 16000, 512, 400, 160
    y = AM.swell(int(1.2 * sr), sr, 9).astype(np.float64)
    n_fft_, W_, H_, nf, nt, smooth, _ = AM.geometry(sr, n_fft, W, H)
    kw = dict(lam=AM.forget_factor(0.25, sr, H), learn=AM.learn_frames(0.3, sr, H))
    whole = np.concatenate(AM.adaptive_model([y], n_fft_, W_, H_, 0.7, nf, nt, smooth, **kw)[0])
    outs, _, _ = AM.adaptive_model(np.split(y, list(range(320, len(y), 320))), n_fft_, W_, H_, 0.7, nf, nt, smooth, **kw)
    assert np.max(np.abs(np.concatenate(outs) - whole)) <= 1e-12 * np.max(np.abs(whole))
    u = AM.unit(y, sr, n_fft, W, H, p=0.7, **kw)
    assert np.max(np.abs(u["want"] - whole)) <= 1e-12 * np.max(np.abs(whole))


def test_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from noisereduce_amd import _ffi
    header = open(os.path.join(ROOT, "include", "mi355gate.h")).read()
    lib = _ffi.load_library()
    for name in ("sg_stream_create_adaptive", "sg_stream_noise_profile", "sg_stream_state_bytes_adaptive"):
        assert re.search(r"SG_API int %s\(" % name, header), name
        assert name in _ffi.exported_symbols()
        assert hasattr(lib, name)


def test_arguments_are_checked_before_any_device_work():
    from noisereduce_amd import stream
    import noisereduce_amd as nr
    kw = dict(n_fft=512, win_length=400, hop_length=160)
    thr = np.zeros(257)
    bad = [dict(noise_from_stream=True, y_noise=np.zeros(16000)),
           dict(noise_from_stream=True, thresholds_db=thr),
           dict(noise_from_stream=True, stationary=False),
           dict(noise_memory_s=1.0, thresholds_db=thr),
           dict(noise_learn_s=1.0, thresholds_db=thr),
           dict(noise_memory_s=1.0, stationary=False),
           dict(noise_from_stream=True, noise_memory_s=0.0),
           dict(noise_from_stream=True, noise_memory_s=-1.0),
           dict(noise_from_stream=True, noise_memory_s=float("inf")),
           dict(noise_from_stream=True, noise_memory_s=float("nan")),
           dict(noise_from_stream=True, noise_learn_s=159.0 / 16000),      # below one hop: learn_frames < 1
           dict(noise_from_stream=True, noise_learn_s=0.0),
           dict(noise_from_stream=True, noise_learn_s=float("nan"))]
    for b in bad:
        with pytest.raises(ValueError):
            stream.StreamBank(16000, 2, **kw, **b)
    with pytest.raises(ValueError):
        nr.StreamGate(16000, noise_from_stream=True, noise_learn_s=0.001, **kw)
    bank = stream.StreamBank(16000, 3, channels=2, noise_from_stream=True, noise_memory_s=0.25, noise_learn_s=0.3, **kw)
    assert bank._bank is None                                  # nothing touched the device
    assert bank.noise_forget == float(np.exp(-160 / (16000 * 0.25))) and bank.noise_learn_frames == 30
    assert stream.StreamBank(16000, 1, noise_from_stream=True, noise_learn_s=160.0 / 16000, **kw).noise_learn_frames == 1
    free = stream.StreamBank(16000, 1, noise_from_stream=True, **kw)
    assert free.noise_forget == 1.0 and free.noise_learn_frames == -1
    with pytest.raises(ValueError):
        bank.set_noise([0], thresholds_db=thr)
    with pytest.raises(ValueError, match="noise_profile"):
        bank.thresholds()
    with pytest.raises(ValueError):
        bank.noise_profile(3)
    fixed = stream.StreamBank(16000, 3, thresholds_db=thr, **kw)
    with pytest.raises(ValueError):
        fixed.noise_profile(0)
    # a bank without the new arguments fails as before
    with pytest.raises(ValueError, match="no noise profile"):
        stream.StreamBank(16000, 1, **kw).push({0: np.zeros(100, dtype=np.float32)})
    assert bank._bank is None and fixed._bank is None


def test_state_bytes_counts_the_statistics():
    from noisereduce_amd import stream
    kw = dict(n_fft=512, win_length=400, hop_length=160)
    FS = (257 + 15) // 16 * 16
    a = stream.StreamBank(16000, 3, channels=2, noise_from_stream=True, max_block=4000, **kw)
    f = stream.StreamBank(16000, 3, channels=2, thresholds_db=np.zeros(257), max_block=4000, **kw)
    assert a.state_bytes - f.state_bytes == 6 * 3 * FS * 8
    base = stream.state_bytes(6, 512, 400, 160, a.nt, 0, 4000, True)
    assert base == f.state_bytes
    assert stream.state_bytes(6, 512, 400, 160, a.nt, 0, 4000, True, noise_from_stream=True) == a.state_bytes
