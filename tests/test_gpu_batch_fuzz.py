"""reduce_noise_batch against the float64 oracle: random geometries, chunk grids, gate parameters, sample types and noise
forms (deterministic seeds), and the per-clip edge scenarios inside a batch -- floor-lifted bands, NaN and Inf, digital
silence, a threshold below 20 log10(eps), short clips under large padding.  Every branch of ragged.hip that the batched
path alone has is reached by some case here; each scenario first checks on the oracle side that its
input reaches the branch it is about."""
import numpy as np
import pytest
import torch

from oracle import spectralgate_oracle as O
from tests.test_gpu_batch import _clip, _in_batch, _nonfinite_agree, _peak_err
from tests.test_gpu_geometry import _floor_inputs_geom

pytestmark = pytest.mark.gpu

import noisereduce_amd as nr  # noqa: E402
from noisereduce_amd import _ffi, batch  # noqa: E402

TOL = 1e-4                                              # tests/test_gpu_fuzz.py
EPS = float(np.finfo(np.float64).eps)
EPS_DB = 20.0 * np.log10(EPS)
SAMPLE_BUDGET = 400_000                                 # samples of all clips of one seed (the oracle's cost)
_NFFTS = (256, 512, 1024, 2048, 4096)
_GATE_KW = ("prop_decrease", "time_constant_s", "freq_mask_smooth_hz", "time_mask_smooth_ms",
            "thresh_n_mult_nonstationary", "sigmoid_slope_nonstationary", "n_std_thresh_stationary", "chunk_size",
            "padding", "n_fft", "win_length", "hop_length", "clip_noise_stationary")


def _np(a):
    """numpy float64 view of an array or a tensor (the oracle's input)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def _oracle(y, sr, stationary, y_noise, kw):
    return O.reduce_noise_S(_np(y), sr, stationary=stationary, y_noise=None if y_noise is None else _np(y_noise),
                            **{k: kw[k] for k in _GATE_KW})


def _gate(ys, sr, stationary, y_noise, kw):
    """The batch's cached engine handle for these arguments (thresholds and sub-batch count of its last call)."""
    p = batch.plan(ys, sr, stationary=stationary, y_noise=y_noise, **kw)
    return batch._gate_for(sr, stationary, p, kw, "cuda")


def _signal(rng, n, sr, C, dtype):
    chans = [O.synth_signal(n, sr=sr, seed=int(rng.integers(1 << 30)), tone_hz=float(rng.uniform(100.0, 0.3 * sr)),
                            tone_amp=float(rng.uniform(0.1, 0.6)), noise_sigma=float(rng.uniform(0.02, 0.2)),
                            dtype=np.float64) for _ in range(C)]
    y = (chans[0] if C == 1 else np.stack(chans)) * float(10.0 ** rng.uniform(-1.5, 0.5))
    return y.astype(dtype)


# ---- 1. randomised batches ---------------------------------------------------------------------------------------------
def _case(seed):
    """One reduce_noise_batch call: (sr, stationary, ys, y_noise, kw, io)."""
    rng = np.random.default_rng(9100 + seed)
    n_fft = _NFFTS[seed % 5]                       # with seed % 2 for the gate: every (n_fft, gate) pair in seeds 0..9
    stationary = seed % 2 == 0
    W = n_fft if rng.random() < 0.4 else int(rng.integers(n_fft // 2, n_fft + 1))
    if seed % 3 == 0 and W % 2 == 0:               # odd windows
        W = W + 1 if W < n_fft else W - 1
    r = rng.random()
    if r < 0.35:
        H = W // 4
    elif r < 0.55:
        H = W // 2 - int(rng.integers(0, 3))       # near W / 2
    else:
        H = int(rng.integers(max(1, W // 8), W // 2 + 1))
    sr = int(rng.choice([8000, 16000, 22050, 44100, 48000]))
    cs = None if rng.random() < 0.25 else int(rng.integers(3 * n_fft, max(3 * n_fft + 1, min(8 * n_fft, 24000))))
    pad_mode = int(rng.integers(0, 3))             # 0: none, 1: a fraction of n_fft, 2: more than the shortest clip
    short = None
    if pad_mode == 0:
        pad = 0
    elif pad_mode == 1:
        pad = int(rng.uniform(0.1, 1.5) * n_fft)
        if rng.random() < 0.5:
            short = int(rng.integers(max(1, W - 2 * pad), W))          # shorter than the window, the padded one fits
    else:
        short = int(rng.integers(max(1, W // 8), W))
        pad = short + int(rng.integers(1, 2 * n_fft))
    form = ("none", "shared", "shared_2d", "list")[seed // 2 % 4] if stationary else None
    if form == "none" and seed != 0:
        short = None        # a clip shorter than the window cannot be its own noise clip: ValueError (seed 0 only)
    lens = []
    if cs is not None:
        edges = [cs, cs + 1, int(rng.integers(2, 4)) * cs, int(rng.integers(3 * cs, 4 * cs))]
        lens += [edges[i] for i in sorted(rng.choice(4, size=int(rng.integers(2, 5)), replace=False))]
    lens += [int(rng.integers(W, 6 * n_fft)) for _ in range(int(rng.integers(1, 4)))]
    if short is not None:
        lens.insert(int(rng.integers(0, len(lens) + 1)), short)
    lens = lens[:8]
    while len(lens) < 3:
        lens.append(int(rng.integers(W, 4 * n_fft)))
    chans = [int(rng.choice([1, 1, 2, 3])) for _ in lens]
    while sum(c * n for c, n in zip(chans, lens)) > SAMPLE_BUDGET:      # bound the oracle's work
        j = max(range(len(lens)), key=lambda i: chans[i] * lens[i])
        if chans[j] > 1:
            chans[j] -= 1
        else:
            lens[j] = max(W, lens[j] // 2)
    dtypes = [np.float32, np.float64] + [rng.choice([np.float32, np.float64]) for _ in lens[2:]]
    rng.shuffle(dtypes)
    ys = [_signal(rng, n, sr, C, dt) for n, C, dt in zip(lens, chans, dtypes)]

    kw = dict(chunk_size=cs, padding=pad, n_fft=n_fft, win_length=W, hop_length=H,
              prop_decrease=float(rng.choice([1.0, 0.7])), n_std_thresh_stationary=float(rng.choice([0.5, 1.5, 2.0])),
              clip_noise_stationary=bool(rng.random() < 0.5), time_constant_s=2.0, thresh_n_mult_nonstationary=2,
              sigmoid_slope_nonstationary=10)
    if not stationary and rng.random() < 0.6:
        kw.update(time_constant_s=float(rng.choice([0.3, 1.0, 4.0])),
                  thresh_n_mult_nonstationary=float(rng.choice([1.0, 1.5, 3.0])),
                  sigmoid_slope_nonstationary=float(rng.choice([4.0, 20.0])))
    # smoothing widths >= 1 bin / 1 frame (base.py:105-123), scaled to the geometry as in tests/test_gpu_fuzz.py
    kw["freq_mask_smooth_hz"] = float(rng.choice([1.5, 3.0, 5.5])) * sr / (n_fft / 2) + 1.0
    kw["time_mask_smooth_ms"] = float(rng.choice([1.5, 2.5, 6.0])) * H / sr * 1000.0 + 0.01
    r = rng.random()
    if r < 0.12:
        kw["freq_mask_smooth_hz"] = None
    elif r < 0.24:
        kw["time_mask_smooth_ms"] = None
    elif r < 0.32:
        kw["freq_mask_smooth_hz"] = kw["time_mask_smooth_ms"] = None

    io = "tensor" if seed % 7 == 3 else "numpy"
    y_noise = None
    if stationary:
        nlen = lambda: int(rng.integers(W, 5 * n_fft))                   # noqa: E731
        if form == "shared":
            y_noise = _signal(rng, nlen(), sr, 1, rng.choice([np.float32, np.float64]))
        elif form == "shared_2d":
            y_noise = _signal(rng, nlen(), sr, int(rng.integers(2, 4)), np.float32)
        elif form == "list":
            kinds = ["none", "numpy", "cpu", "cuda"]
            y_noise = []
            for j, y in enumerate(ys):
                k = kinds[(j + seed) % 4]
                if k == "none" and y.shape[-1] < W:
                    k = "numpy"                                          # a clip shorter than the window needs a noise clip
                if k == "none":
                    y_noise.append(None)
                    continue
                a = _signal(rng, nlen(), sr, int(rng.choice([1, 1, 2])), rng.choice([np.float32, np.float64]))
                y_noise.append(a if k == "numpy" else torch.from_numpy(a) if k == "cpu" else torch.from_numpy(a).cuda())
    if io == "tensor":
        ys = [torch.from_numpy(y).cuda() for y in ys]
    return sr, stationary, ys, y_noise, kw, io


def _noise_of(y_noise, i):
    return y_noise[i] if isinstance(y_noise, list) else y_noise


def _check_thresholds(g, ys, y_noise, kw):
    """Thresholds of every noise source of the last call against the oracle's (<= 1e-9 dB)."""
    n_fft, W, H = kw["n_fft"], kw["win_length"], kw["hop_length"]
    srcs = [y_noise] if (y_noise is not None and not isinstance(y_noise, list)) else \
        [ys[i] if _noise_of(y_noise, i) is None else _noise_of(y_noise, i) for i in range(len(ys))]
    thr = g.clip_thresholds(len(srcs))
    for j, s in enumerate(srcs):
        want, _, _ = O.noise_threshold_S(np.atleast_2d(_np(s)), n_fft, W, H, kw["n_std_thresh_stationary"],
                                         kw["chunk_size"], kw["clip_noise_stationary"] and kw["chunk_size"] is not None)
        assert np.max(np.abs(thr[j] - want)) <= 1e-9, (j, np.max(np.abs(thr[j] - want)))
    return thr


@pytest.mark.parametrize("seed", range(28))
def test_random_batch_matches_oracle_per_clip_and_solo(seed):
    sr, stationary, ys, y_noise, kw, io = _case(seed)
    try:
        want = [_oracle(y, sr, stationary, _noise_of(y_noise, i) if stationary else None, kw) for i, y in enumerate(ys)]
    except ValueError:
        with pytest.raises(ValueError):
            nr.reduce_noise_batch(ys, sr, stationary=stationary, y_noise=y_noise, **kw)
        return
    assert batch.plan(ys, sr, stationary=stationary, y_noise=y_noise, **kw).routes == [batch.BATCHED] * len(ys)
    outs = nr.reduce_noise_batch(ys, sr, stationary=stationary, y_noise=y_noise, **kw)
    if stationary:
        thr = _check_thresholds(_gate(ys, sr, stationary, y_noise, kw), ys, y_noise, kw)
    # every clip its own sub-batch: a shared noise threshold is recomputed in each, the outputs do not move
    split = nr.reduce_noise_batch(ys, sr, stationary=stationary, y_noise=y_noise, max_workspace_bytes=1, **kw)
    g = _gate(ys, sr, stationary, y_noise, kw)
    assert g.clip_batches() == len(ys)
    if stationary:
        assert np.array_equal(g.clip_thresholds(len(thr)), thr)
    for i, (y, o, w) in enumerate(zip(ys, outs, want)):
        assert isinstance(o, torch.Tensor) == (io == "tensor")
        assert tuple(o.shape) == tuple(y.shape) and o.dtype == y.dtype, i
        oh = _host(o)
        assert np.array_equal(_host(split[i]), oh), i
        assert O.rel_err(oh, w) < TOL, (i, O.rel_err(oh, w), kw)
        yn = _noise_of(y_noise, i) if stationary else None
        per_clip = nr.reduce_noise(_host(y), sr, stationary=stationary, y_noise=None if yn is None else _np(yn),
                                   **{k: kw[k] for k in _GATE_KW})
        # (2e-6: the per-clip path's float32 non-stationary transforms are themselves ~1.06e-6 of peak off the oracle at
        # seed 23 -- n_fft 2048, sigmoid slope 20 -- where the batch's float64 ones are 1.1e-7 off)
        assert _peak_err(oh, per_clip) < 2e-6, (i, _peak_err(oh, per_clip), O.rel_err(per_clip, w))
        # alone: the same bits (a float32 clip next to a float64 one travels as float64, alone as float32)
        solo = nr.reduce_noise_batch([y], sr, stationary=stationary,
                                     y_noise=[yn] if isinstance(y_noise, list) else y_noise, **kw)[0]
        assert np.array_equal(_host(solo), oh), i


# integer clips with NOISEREDUCE_AMD_FAST_INT=1: float32 segments and output buffer
def _int_clip(n, seed, scale, dtype, C=1):
    y = np.clip(_clip(n, seed, sr=16000, C=C, dtype=np.float64), -1.0, 1.0) * scale
    return np.round(y).astype(dtype)


_INT_CASES = {
    "int16": [(np.int16, 20000.0, 9000, 1), (np.int16, 20000.0, 31000, 2), (np.int16, 20000.0, 70001, 1)],
    "int32": [(np.int32, 1.5e9, 12000, 1), (np.int32, 1.5e9, 50000, 2), (np.int32, 1.5e9, 24000, 1)],
    # the int32 clip forces the whole batch to float64
    "mixed": [(np.int16, 20000.0, 26000, 1), (np.int32, 1.5e9, 41000, 1), (np.float32, 1.0, 33000, 2),
              (np.int16, 20000.0, 8000, 2)],
}


@pytest.mark.parametrize("stationary", [True, False])
@pytest.mark.parametrize("kind", sorted(_INT_CASES))
def test_integer_batches_fast_int(monkeypatch, kind, stationary):
    sr = 16000
    ys = [(_int_clip(n, 300 + i, scale, dt, C) if dt != np.float32 else _clip(n, 300 + i, C=C))
          for i, (dt, scale, n, C) in enumerate(_INT_CASES[kind])]
    kw = dict(chunk_size=30000, padding=3000, n_fft=512)
    monkeypatch.setenv("NOISEREDUCE_AMD_FAST_INT", "1")
    _ffi.clear_gate_cache()
    try:
        assert batch.plan(ys, sr, stationary=stationary, **kw).routes == [batch.BATCHED] * len(ys)
        outs = nr.reduce_noise_batch(ys, sr, stationary=stationary, **kw)
        solos = [nr.reduce_noise_batch([y], sr, stationary=stationary, **kw)[0] for y in ys]
    finally:
        _ffi.clear_gate_cache()
    for i, (y, o) in enumerate(zip(ys, outs)):
        assert o.shape == y.shape and o.dtype == y.dtype, i
        assert np.array_equal(o, solos[i]), i
        want = O.reduce_noise_S(y.astype(np.float64), sr, stationary=stationary, **kw)
        if y.dtype == np.int16:
            assert np.max(np.abs(o.astype(np.int64) - np.trunc(want).astype(np.int64))) <= 1, i
        else:
            # int32: the float32 output buffer holds ~7 digits; float32: the usual bar
            assert O.rel_err(o, want) < TOL, (i, O.rel_err(o, want))


# ---- 2. per-clip edge scenarios inside a batch ---------------------------------------------------------------------------
def _units(N, cs, pad):
    """(window start, window end) of every unit of a clip (base.py:167-226)."""
    if cs is not None and N > cs:
        return [(k * cs - pad, (k + 1) * cs + pad) for k in range(-(-N // cs))]
    return [(-pad, N + pad)]


def _floor_lifted_bands(y, y_noise, kw):
    """Number of (unit, channel, band) whose -top_db floor lies above the stationary threshold (k_rg_fsmooth's 'every
    cell passes' branch), computed by the oracle."""
    n_fft, W, H = O.resolve_stft_params(kw.get("n_fft", 1024), kw.get("win_length"), kw.get("hop_length"))
    thr, _, _ = O.noise_threshold_S(np.atleast_2d(_np(y_noise)), n_fft, W, H, kw.get("n_std_thresh_stationary", 1.5),
                                    kw["chunk_size"])
    y2 = np.atleast_2d(_np(y))
    count = 0
    with np.errstate(all="ignore"):
        for a, b in _units(y2.shape[1], kw["chunk_size"], kw["padding"]):
            for ch in O.read_chunk(y2, a, b):
                top = 20.0 * np.log10(np.abs(O.stft_scipy(ch, n_fft, W, H)).max(axis=1) + EPS)
                count += int(np.count_nonzero(top - 80.0 > thr))
    return count


_FLOOR_KINDS = ["benign", "live", "loud_in_padding", "nan_in_padding", "inf_far_padding"]


@pytest.mark.parametrize("n_fft", _NFFTS)
@pytest.mark.parametrize("kind", _FLOOR_KINDS)
def test_floor_inputs_inside_a_batch(kind, n_fft):
    y, y_noise, cs, pad = _floor_inputs_geom(kind, n_fft)
    sr = 48000
    kw = dict(stationary=True, chunk_size=cs, padding=pad, n_fft=n_fft)
    if kind == "live":
        assert _floor_lifted_bands(y, y_noise, kw) > 0
    with np.errstate(all="ignore"):
        want = O.reduce_noise_S(_np(y), sr, y_noise=_np(y_noise), **kw)
    out = _in_batch(y, y_noise, sr, kw)
    assert out.shape == y.shape and out.dtype == y.dtype
    if kind == "nan_in_padding":
        assert np.isnan(want).any()
        _nonfinite_agree(out, want, TOL)
    elif kind == "inf_far_padding":
        # the stated deviation (an Inf gates its units like a NaN): the oracle's non-finite samples,
        # the per-clip path's finite values in the units the Inf reaches, the oracle's in the units it does not reach
        # (chunks 2.. of the clip).  (At n_fft = 512 the per-clip path marks 128 samples more on each side non-finite
        # than the reference does: compared where both are finite.)
        per_clip = nr.reduce_noise(y, sr, y_noise=y_noise, **kw)
        nf = ~np.isfinite(out)
        assert nf.any() and np.array_equal(nf, ~np.isfinite(want))
        both = ~nf & np.isfinite(per_clip)
        assert _peak_err(out[both], per_clip[both]) < 1e-6
        far = slice(2 * cs, None)
        assert np.isfinite(want[far]).all() and np.isfinite(out[far]).all()
        assert O.rel_err(out[far], want[far]) < TOL
    else:
        assert np.isfinite(want).all()
        assert O.rel_err(out, want) < TOL, O.rel_err(out, want)


def _db_floor_live_input():
    rng = np.random.default_rng(77)
    n = 60000
    y = np.zeros(n)
    y[n // 2:] = 0.5 * rng.standard_normal(n // 2)
    y = y.astype(np.float32)
    quiet = (1e-7 * rng.standard_normal(20000)).astype(np.float32)
    loud = (0.3 * rng.standard_normal(20000)).astype(np.float32)
    return y, quiet, loud


@pytest.mark.parametrize("noise", ["quiet", "loud"])
@pytest.mark.parametrize("prop", [1.0, 0.7])
def test_db_floor_live_inside_a_batch(prop, noise):
    """tests/test_gpu_parity.py::test_db_floor_live: digital silence next to loud noise with a very quiet noise clip lifts
    whole bands by the floor; with the loud noise clip the floor is out of reach (contrast)."""
    y, quiet, loud = _db_floor_live_input()
    y_noise = quiet if noise == "quiet" else loud
    kw = dict(stationary=True, prop_decrease=prop, chunk_size=25000, padding=4000)
    lifted = _floor_lifted_bands(y, y_noise, kw)
    assert (lifted > 0) == (noise == "quiet")
    want = O.reduce_noise_S(_np(y), 48000, y_noise=_np(y_noise), **kw)
    out = _in_batch(y, y_noise, 48000, kw)
    assert O.rel_err(out, want) < TOL, O.rel_err(out, want)


def test_digital_silence_stationary_is_zero():
    z = np.zeros(30000, np.float32)
    assert np.all(O.reduce_noise_S(_np(z), 48000, stationary=True) == 0)
    out = _in_batch(z, None, 48000, dict(stationary=True))
    assert out.shape == z.shape and out.dtype == z.dtype and np.all(out == 0)


def test_digital_silence_nonstationary_is_nan_like_the_reference():
    """nonstationary.py:70: a band that is zero over a whole padded chunk gives 0 / 0 -- the reference returns NaN."""
    for dt in (np.float32, np.float64):
        z = np.zeros(30000, dt)
        with np.errstate(all="ignore"):
            assert np.isnan(O.reduce_noise_S(_np(z), 48000, stationary=False)).all()
        out = _in_batch(z, None, 48000, dict(stationary=False))
        assert out.shape == z.shape and out.dtype == dt and np.isnan(out).all()


def test_one_silent_padded_chunk_nonstationary():
    rng = np.random.default_rng(5)
    cs, pad = 20000, 3000
    y = 0.1 * rng.standard_normal(5 * cs)
    y[2 * cs - pad - 2000:3 * cs + pad + 2000] = 0.0          # chunk 2 with its padding (and a margin) is silent
    y = y.astype(np.float32)
    kw = dict(stationary=False, chunk_size=cs, padding=pad)
    with np.errstate(all="ignore"):
        want = O.reduce_noise_S(_np(y), 48000, **kw)
    assert np.isnan(want[2 * cs:3 * cs]).all() and np.isfinite(want[:2 * cs]).all() and np.isfinite(want[3 * cs:]).all()
    out = _in_batch(y, None, 48000, kw)
    _nonfinite_agree(out, want, TOL)


def test_half_silent_single_window_nonstationary():
    rng = np.random.default_rng(6)
    y = np.zeros(60000)
    y[30000:] = 0.1 * rng.standard_normal(30000)
    y = y.astype(np.float32)
    want = O.reduce_noise_S(_np(y), 48000, stationary=False)
    assert np.isfinite(want).all()
    out = _in_batch(y, None, 48000, dict(stationary=False))
    assert np.isfinite(out).all() and O.rel_err(out, want) < TOL


@pytest.mark.parametrize("stationary", [True, False])
def test_constant_clip(stationary):
    """A DC clip: one band holds the energy, the others only what the clip's two edges spread into them."""
    y = np.full(40000, 0.25, np.float32)
    kw = dict(stationary=stationary, chunk_size=25000, padding=3000)
    with np.errstate(all="ignore"):
        want = O.reduce_noise_S(_np(y), 48000, **kw)
    out = _in_batch(y, None, 48000, kw)
    per_clip = nr.reduce_noise(y, 48000, **kw)
    _nonfinite_agree(out, want, TOL)
    assert np.array_equal(np.isfinite(out), np.isfinite(per_clip))
    assert _peak_err(out[np.isfinite(out)], per_clip[np.isfinite(out)]) < 1e-6


def _bursty_silence(n=30000, amp=1e-13, seed=8):
    """Digital silence with three short bursts so quiet that the floor (band max - 80 dB) stays below 20 log10(eps):
    most frames sit at 20 log10(eps) exactly, a few far above, and mean - 2 std lands below it."""
    rng = np.random.default_rng(seed)
    yn = np.zeros(n)
    for a in (2000, 14000, 26000):
        yn[a:a + 40] = amp * rng.standard_normal(40)
    return yn


@pytest.mark.parametrize("n_fft", [256, 1024, 4096])
def test_threshold_below_eps_db(n_fft):
    """k_rg_noise_final's t2 = -1 branch: a threshold below 20 log10(eps) lets every cell pass -- the frames outside the
    data (zero spectrum, never transformed) included, which sit inside the time smoothing of the first and last live
    frames.  The clip is quiet too, so that its -top_db floor stays below the threshold and only that branch decides."""
    sr = 48000
    yn = _bursty_silence()
    kw = dict(stationary=True, n_fft=n_fft, n_std_thresh_stationary=-2.0, chunk_size=30000, padding=3 * n_fft,
              time_mask_smooth_ms=6.5 * (n_fft / 4) / sr * 1000)
    thr, _, _ = O.noise_threshold_S(yn[None, :], n_fft, n_fft, n_fft // 4, -2.0, 30000)
    assert np.count_nonzero(thr < EPS_DB) > thr.size // 2, (thr.min(), thr.max())
    y = (1e-13 * np.random.default_rng(12).standard_normal(50000)).astype(np.float32)
    assert _floor_lifted_bands(y, yn, kw) == 0
    want = O.reduce_noise_S(_np(y), sr, y_noise=yn, **kw)
    assert O.rel_err(want, _np(y)) < 0.05         # every cell passes: the clip comes back (but for the smoothing's edges)
    out = _in_batch(y, yn, sr, kw)
    assert O.rel_err(out, want) < TOL, O.rel_err(out, want)


def _padding_only_frames(n, pad, W, H):
    """Frames of a one-window unit that read only its zero padding (never transformed by the batched path)."""
    T = O.n_frames_for(n + 2 * pad, W, H)
    return sum(1 for t in range(T) if t * H - W // 2 + W <= pad or t * H - W // 2 >= pad + n)


_SHORT = [(256, 100, 5000), (512, 300, 2000), (1024, 700, 6000), (2048, 1500, 3000), (4096, 2500, 9000),
          (1024, 2000, 20000)]


@pytest.mark.parametrize("stationary", [True, False])
@pytest.mark.parametrize("n_fft,n,pad", _SHORT)
def test_short_clips_under_large_padding(n_fft, n, pad, stationary):
    """padding >> n: the data frames start late (d0 > 0) and most frames of the unit are skipped; k_rg_iir steps through
    them with magnitude 0 and stores forward values only from d0 on."""
    sr = 16000
    W, H = n_fft, n_fft // 4
    assert _padding_only_frames(n, pad, W, H) > O.n_frames_for(n + 2 * pad, W, H) // 2
    rng = np.random.default_rng(n_fft + n)
    y = (0.3 * rng.standard_normal(n)).astype(np.float32)
    yn = _clip(3 * n_fft, 17, sr=sr) if stationary else None
    kw = dict(stationary=stationary, n_fft=n_fft, chunk_size=None if n > 1500 else 40000, padding=pad,
              freq_mask_smooth_hz=3.0 * sr / (n_fft / 2) + 1.0, time_mask_smooth_ms=2.5 * H / sr * 1000.0 + 0.01)
    with np.errstate(all="ignore"):
        want = O.reduce_noise_S(_np(y), sr, y_noise=yn, **kw)
    assert np.isfinite(want).all()
    out = _in_batch(y, yn, sr, kw)
    assert O.rel_err(out, want) < TOL, O.rel_err(out, want)
    # several short clips side by side, each with its own noise (none may read another's padding)
    ys = [y, (0.2 * rng.standard_normal(n // 2 + 1)).astype(np.float32), y[::-1].copy()]
    kws = dict(kw)
    st = kws.pop("stationary")
    outs = nr.reduce_noise_batch(ys, sr, stationary=st, y_noise=[yn] * 3 if st else None, **kws)
    assert np.array_equal(outs[0], out) and np.array_equal(outs[2], nr.reduce_noise_batch(
        [ys[2]], sr, stationary=st, y_noise=[yn] if st else None, **kws)[0])
    with np.errstate(all="ignore"):
        assert O.rel_err(outs[1], O.reduce_noise_S(_np(ys[1]), sr, y_noise=yn, **kw)) < TOL


@pytest.mark.parametrize("stationary", [True, False])
@pytest.mark.parametrize("n_fft,W,H", [(256, 256, 255), (1024, 901, 880), (4096, 4096, 4000), (4096, 3001, 2999)])
def test_hops_beyond_half_the_window(n_fft, W, H, stationary):
    """A hop above W / 2 (the reference takes any hop below W): samples that only one window's tail covers have a squared-
    window sum far below 1 -- some below k_rg_ola's 1e-10, where the sum is not divided by it (as scipy's istft)."""
    sr = 16000
    w2 = O.hann_periodic(W) ** 2
    env = np.zeros(W + 4 * H)
    for t in range(5):
        env[t * H:t * H + W] += w2
    env = env[W // 2:len(env) - W // 2]
    assert env.min() < 1e-3
    y = _clip(9 * W + 17, 23, sr=sr)
    kw = dict(stationary=stationary, n_fft=n_fft, win_length=W, hop_length=H, chunk_size=4 * W, padding=W // 3,
              freq_mask_smooth_hz=2.5 * sr / (n_fft / 2), time_mask_smooth_ms=1.5 * H / sr * 1000.0)
    want = O.reduce_noise_S(_np(y), sr, **kw)
    out = _in_batch(y, None, sr, kw)
    assert O.rel_err(out, want) < TOL, O.rel_err(out, want)
