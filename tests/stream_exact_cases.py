"""The inputs and float64 yardsticks of the exact stream banks (a helper, not a test): shared by
tests/test_stream_exact_host.py, which holds the inputs to their conditions without a GPU, and
tests/test_gpu_stream_exact.py.  The yardsticks are the three host models (tests/stream_model.py,
tests/stream_ns_model.py, tests/stream_adaptive_model.py), built from the oracle alone."""
import functools

import numpy as np

from oracle import spectralgate_oracle as O
from tests import stream_adaptive_model as MA
from tests import stream_model as M
from tests import stream_ns_model as MN

# (sr, n_fft, win_length, hop_length)
GEOMS = [(16000, 512, 400, 160), (16000, 256, None, None)]
LARGE = [(16000, 2048, None, None), (48000, 4096, None, None)]      # the 256-thread tiles
KINDS = ("fixed", "nonstationary", "adaptive")
PLANS = ("whole", "random", "edge", "small")
SCALE = {np.dtype(np.int16): 20000.0, np.dtype(np.int32): 1.5e9}     # tests/test_gpu_dtypes.py's amplitudes
MARGIN = {np.dtype(np.int16): 1e-9, np.dtype(np.int32): 1e-4}        # ... and its "decided" margins
DECIDED_SHARE = 0.9
TC, LOOKAHEAD = 0.1, 3            # non-stationary: time_constant_s; lookahead in frames (a few: blocks emit before the flush)
THRESHOLD_MARGIN_DB = 1e-6        # float64-accuracy cases: no cell of a hard threshold nearer to it than this


def resolve(geom):
    sr, n_fft, W, H = geom
    return (sr,) + tuple(O.resolve_stft_params(n_fft, W, H))


def lookahead_ms(geom, L=LOOKAHEAD):
    sr, _, _, H = resolve(geom)
    return (L + 0.5) * H / sr * 1000.0


def bank_kw(geom, kind, p=1.0, L=LOOKAHEAD):
    """StreamBank arguments of a case (without the noise clip of a fixed-profile bank)."""
    sr, n_fft, W, H = geom
    kw = dict(n_fft=n_fft, win_length=W, hop_length=H, prop_decrease=p)
    if kind == "nonstationary":
        kw.update(stationary=False, lookahead_ms=lookahead_ms(geom, L), time_constant_s=TC)
    if kind == "adaptive":
        kw.update(noise_from_stream=True)
    return kw


def cuts(kind, N, W, H, rng):
    """tests/test_gpu_stream.py's four block plans."""
    if kind == "whole":
        return []
    if kind == "random":
        return sorted(int(c) for c in rng.integers(0, N + 1, 7))
    if kind == "edge":
        e = 3 * H - W // 2 + W
        return sorted(min(c, N) for c in (e - 3, e - 2, e - 1, e, e, e, e + 1, e + 2, N // 2, N // 2))
    if kind == "small":
        return list(range(131, N, 131))
    raise KeyError(kind)


def length(geom, seed):
    """W + 5 ... 6 W + 20 H samples."""
    _, _, W, H = resolve(geom)
    return int(np.random.default_rng(seed).integers(W + 5, 6 * W + 20 * H))


def noise_clip(sr, scale=1.0, seed=7):
    return scale * 0.1 * np.random.default_rng(seed).standard_normal(3 * sr // 4)


def signal(geom, seed, dtype, N=None):
    """A stream of the case's length: tone + noise, integers at tests/test_gpu_dtypes.py's amplitudes."""
    dtype = np.dtype(dtype)
    N = length(geom, seed) if N is None else N
    y = O.synth_signal(N, sr=geom[0], seed=seed, dtype=np.float64)
    if dtype.kind == "i":
        return np.round(y * SCALE[dtype]).astype(dtype)
    return y.astype(dtype)


def scale_of(dtype):
    return SCALE.get(np.dtype(dtype), 1.0)


def fixed_threshold(geom, scale=1.0):
    sr, n_fft, W, H = resolve(geom)
    return O.noise_threshold_S(np.atleast_2d(noise_clip(sr, scale)), n_fft, W, H, 1.5, None, True)[0]


def model(geom, kind, y, p=1.0, L=LOOKAHEAD, direct=False):
    """The float64 model's output for the whole stream y (any sample type; the models work on its float64 values) and a
    dict of what the host test looks at: `live` (fixed: the causal floor differs from the offline one) and `margin_db`
    (fixed / adaptive: the smallest distance of a cell from its threshold)."""
    sr, n_fft, W, H = resolve(geom)
    _, _, _, nf, nt, smooth, _ = M.geometry(sr, n_fft, W, H, 500, 50)
    y64 = np.asarray(y, dtype=np.float64)
    T = (len(y64) + 2 * (W // 2) - W) // H + 1
    info = {}
    if kind == "fixed":
        thr = fixed_threshold(geom, scale_of(np.asarray(y).dtype))
        outs, info["live"] = M.stream_model([y64], thr, n_fft, W, H, p, nf, nt, smooth)
        _, db = MA.spectrum(y64, T, n_fft, W, H)
        x = np.maximum(db, np.maximum.accumulate(db, axis=1) - 80.0)
        d = np.abs(x - thr[:, None])
        info["margin_db"] = float(d[np.isfinite(d)].min())
    elif kind == "nonstationary":
        b = O.iir_coefficient(TC, sr, H)
        outs = MN.stream_ns_model([y64], n_fft, W, H, p, nf, nt, smooth, b, L, direct=direct)
    elif kind == "adaptive":
        outs, _, _ = MA.adaptive_model([y64], n_fft, W, H, p, nf, nt, smooth)
        _, db = MA.spectrum(y64, T, n_fft, W, H)
        x, thr, _ = MA.recurrence(db)
        info["margin_db"] = MA.margin_db(x, thr)
    else:
        raise KeyError(kind)
    return np.concatenate(outs), info


def decided(want64, dtype):
    """tests/test_gpu_dtypes.py: a sample is decided when the float64 value lies further from an integer than the
    rounding noise of another evaluation order can carry it."""
    with np.errstate(invalid="ignore"):
        return np.abs(want64 - np.round(want64)) > MARGIN[np.dtype(dtype)]


def trunc(want64, dtype):
    """The exact bank's integer store: NaN -> 0, then truncation toward zero (ndarray.astype)."""
    return np.where(np.isnan(want64), 0.0, want64).astype(dtype)


# ---- the cases of the GPU file ------------------------------------------------------------------------------------------
# integers, bit for bit: every kind of bank x both integer types x both prop_decrease values, the geometries alternating
INT_CASES = [(GEOMS[(i + j + k) % 2], kind, np.dtype(dt), p, 500 + 100 * i + 10 * j + k)
             for i, kind in enumerate(KINDS) for j, dt in enumerate((np.int16, np.int32)) for k, p in enumerate((1.0, 0.7))]
# the 256-thread tiles: 2 W + 3 samples, int16, fixed profile
LARGE_CASES = [(g, "fixed", np.dtype(np.int16), 1.0, 900 + i) for i, g in enumerate(LARGE)]
# float64 accuracy: one stream per block plan, the three kinds of bank x both geometries
F64_CASES = [(g, kind, 700 + 10 * i + j) for i, kind in enumerate(KINDS) for j, g in enumerate(GEOMS)]
SILENCE_SEED = 950


def large_signal(geom, seed):
    _, _, W, _ = resolve(geom)
    return signal(geom, seed, np.int16, N=2 * W + 3)


def silence_signal(geom=GEOMS[0], seed=SILENCE_SEED):
    """int16 digital silence, then signal (non-stationary: 0 / 0 = NaN where the level is 0)."""
    y = signal(geom, seed, np.int16, N=6000)
    y[:2500] = 0
    return y


@functools.lru_cache(maxsize=None)
def int_case(i, large=False):
    """(geom, kind, dtype, p, y, want64) of integer case i: computed once, shared, read-only."""
    geom, kind, dt, p, seed = (LARGE_CASES if large else INT_CASES)[i]
    y = large_signal(geom, seed) if large else signal(geom, seed, dt)
    want64, info = model(geom, kind, y, p)
    y.setflags(write=False)
    want64.setflags(write=False)
    return geom, kind, dt, p, y, want64, info


@functools.lru_cache(maxsize=None)
def f64_case(i):
    """(geom, kind, streams): four float64 streams, one per block plan, each (y, model output, info, model output of
    y.astype(float32), its info)."""
    geom, kind, seed = F64_CASES[i]
    streams = []
    for j in range(4):
        y = signal(geom, seed + 100 * j, np.float64)
        want, info = model(geom, kind, y)
        want32, info32 = model(geom, kind, y.astype(np.float32))
        for a in (y, want, want32):
            a.setflags(write=False)
        streams.append((y, want, info, want32, info32))
    return geom, kind, streams
