"""Stage-by-stage, local parity metrics for the gate paths (plain helper module: pure numpy / scipy, no GPU).

The suite's usual bar, ``O.rel_err(got, want) < 1e-4``, divides the largest error anywhere by the largest sample
anywhere.  It is ~500 x looser than the float32 kernels and blind to everything in a quiet part of a recording.  The
helpers here hold a kernel to the float64 oracle per stage and per hop block instead:

* ``signals``          deterministic float32-valued inputs with a loud and a quiet part, DC / Nyquist content, tones
                       exactly on bins, bursts at chunk seams;
* ``oracle_units``     what ``O.reduce_noise_S`` does, keeping the oracle's stages per (channel, chunk) unit --
                       ``torchgate_units`` likewise for ``O.torchgate_T``;
* ``emulate_f32``      the same operation in the kernels' arithmetic (float32 frames, window, pocketfft transforms,
                       mask multiply, overlap-add, envelope division) as a plain reference: its distance from the
                       float64 oracle is the error a correct float32 implementation is entitled to;
* ``local_error`` / ``budget`` / ``local_check``   per hop block: max |got - want| against FACTOR x the emulation's;
* ``bit_diff``         decision bits against the oracle's ``raw``, leaving out cells within ``DELTA_DB`` of the threshold;
* ``mask_bound``       what a float32 smoothed mask may differ from the oracle's by.

Where the numbers come from (none is taken from the code under test):

``DELTA_DB = 1e-8``  the project pins its threshold to 1e-9 dB of the reference and decides in float64; ten times that
                     covers the evaluation order of the dB field itself.
``LEFT_OUT_CAP = 1e-5``  share of a unit's cells that may fall inside the margin (the oracle alone leaves out none on
                     the matrix inputs: tests/test_parity_budget_host.py).
``FACTOR = 8``       the kernels use another factorisation and table twiddles (up to ~2 x in RMS rounding error against
                     pocketfft), the maximum over H samples of two independent error sequences differs by up to ~2 x,
                     and 2 x on top.  The additive term ``4 eps32 max|want|`` is the output's own float32 rounding.
``mask_bound``       stationary smoothing is exact integer arithmetic over the filter's integer taps, so a float32
                     field is within one rounding: 2^-23 (prop_decrease = 1), 3 * 2^-24 with one more multiply-add.
``F64_REL = 1e-12``  the project's own float64 bar, here of the LOCAL block peak (floor: 1e-3 of the global peak).
"""
import functools

import numpy as np
import scipy.fft

from oracle import spectralgate_oracle as O

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
DELTA_DB = 1e-8
LEFT_OUT_CAP = 1e-5
FACTOR = 8.0
F64_REL = 1e-12
POOL = 2              # a block's budget is the emulation's largest error over blocks b - POOL .. b + POOL


# ----------------------------------------------------------------------------------------------------------------
# signals
# ----------------------------------------------------------------------------------------------------------------
class signals:
    """Deterministic generators; every one returns a float32 array."""

    @staticmethod
    def _base(n, sr, seed, tone_hz=1000.0, tone_amp=0.5, sigma=0.1):
        rng = np.random.default_rng(seed)
        t = np.arange(n, dtype=np.float64) / sr
        return sigma * rng.standard_normal(n) + tone_amp * np.sin(2 * np.pi * tone_hz * t)

    @staticmethod
    def two_level(n, sr=48000, seed=1):
        """Tone + noise; the second half is scaled by 1e-3 (60 dB down, not silent)."""
        y = signals._base(n, sr, seed)
        y[n // 2:] *= 1e-3
        return y.astype(F32)

    @staticmethod
    def dc_nyquist(n, sr=48000, seed=2):
        """Tone + noise + 0.01 DC + 0.02 (-1)^n: the two bins a packed real transform unpacks separately."""
        y = signals._base(n, sr, seed, tone_hz=1370.0)
        y += 0.01 + 0.02 * (1.0 - 2.0 * (np.arange(n) % 2))
        return y.astype(F32)

    @staticmethod
    def bin_centred(n, n_fft=1024, seed=3):
        """Tones exactly on bins k = 1, F - 2 and three bins between (0 < k < F - 1), over 0.05 white noise."""
        F = n_fft // 2 + 1
        ks = sorted({1, F - 2, max(2, F // 7), max(2, F // 3), max(2, (2 * F) // 3)} - {0, F - 1})
        rng = np.random.default_rng(seed)
        i = np.arange(n, dtype=np.float64)
        y = 0.05 * rng.standard_normal(n)
        for j, k in enumerate(ks):
            y += 0.15 * np.sin(2 * np.pi * k * i / n_fft + 0.3 * j)
        return y.astype(F32)

    @staticmethod
    def burst_at_seam(n, chunk_size, padding, sr=48000, seed=4):
        """A quiet tone + noise with two 30 dB bursts: one straddling the first chunk boundary, one lying wholly
        inside the left padding of the third chunk (only the second chunk's right padding and the third chunk's
        left padding see it as padding; it is kept output of the second chunk)."""
        y = signals._base(n, sr, seed, tone_hz=800.0, tone_amp=0.012, sigma=0.003)
        g = 10.0 ** (30.0 / 20.0)
        half = max(24, chunk_size // 24)
        a, b = max(0, chunk_size - half), min(n, chunk_size + half)
        y[a:b] *= g
        if padding >= 8 and 2 * chunk_size <= n:
            y[2 * chunk_size - (3 * padding) // 4:2 * chunk_size - padding // 4] *= g
        return y.astype(F32)


# ----------------------------------------------------------------------------------------------------------------
# the oracle, unit by unit
# ----------------------------------------------------------------------------------------------------------------
def _final_mask(raw, cfg):
    """raw bits / raw sigmoid -> final mask in float64 with the smoothing summed directly (O.conv2_same_direct)."""
    raw = np.asarray(raw, dtype=np.float64)
    conv = (lambda m: O.conv2_same_direct(m, cfg["filt"])) if cfg["filt"] is not None else (lambda m: m)
    if cfg["variant"] == "T":
        return conv(cfg["prop"] * (raw - 1.0) + 1.0)
    if cfg["stationary"]:
        return conv(raw * cfg["prop"] + (1.0 - cfg["prop"]))
    return conv(raw) * cfg["prop"] + (1.0 - cfg["prop"])


def oracle_units(y, sr, stationary=False, y_noise=None, prop_decrease=1.0, time_constant_s=2.0,
                 freq_mask_smooth_hz=500, time_mask_smooth_ms=50, thresh_n_mult_nonstationary=2,
                 sigmoid_slope_nonstationary=10, n_std_thresh_stationary=1.5, chunk_size=600000, padding=30000,
                 n_fft=1024, win_length=None, hop_length=None, clip_noise_stationary=True):
    """``O.reduce_noise_S`` with its stages kept.  Returns ``(out, units)``: ``out`` the float64 (C, N) / (N,) result
    (not cast to the input's dtype), ``units`` one dict per (channel, chunk) in the engine's unit order (channel-major):

    ``ch, chunk``  indices;  ``x`` the padded chunk (Lp,);  ``Z`` (F, T) complex128;  ``db`` the floored dB field
    (stationary);  ``thresh`` (F,);  ``raw`` bits (stationary) / raw sigmoid;  ``mask`` the final mask;  ``y`` the
    gated padded chunk (Lp,), zeros beyond the inverse transform's length;  ``keep = (k0, k1)`` the kept range of
    ``y``;  ``dst = (s0, e0)`` where it lands in the recording;  ``want = y[k0:k1]``;  ``cfg`` the parameters."""
    y = np.asarray(y)
    flat = y.ndim == 1
    y2 = (y[None, :] if flat else y).astype(np.float64)
    C, N = y2.shape
    n_fft, W, H = O.resolve_stft_params(n_fft, win_length, hop_length)
    nf, nt, smooth = O.mask_smoothing_widths(sr, n_fft, H, freq_mask_smooth_hz, time_mask_smooth_ms)
    filt = O.smoothing_filter(nf, nt) if smooth else None
    cfg = dict(variant="S", stationary=bool(stationary), n_fft=n_fft, W=W, H=H, prop=float(prop_decrease), nf=nf, nt=nt,
               filt=filt, iir_b=None, thresh_n_mult=thresh_n_mult_nonstationary, slope=sigmoid_slope_nonstationary)
    thresh = None
    if stationary:
        yn2 = y2 if y_noise is None else np.atleast_2d(np.asarray(y_noise, dtype=np.float64))
        thresh, _, _ = O.noise_threshold_S(yn2, n_fft, W, H, n_std_thresh_stationary, chunk_size, clip_noise_stationary)
    else:
        cfg["iir_b"] = float(O.iir_coefficient(time_constant_s, sr, H))

    if chunk_size is not None and N > chunk_size:
        grid = [(i * chunk_size, (i + 1) * chunk_size, min((i + 1) * chunk_size, N))
                for i in range(int((N - 1) / chunk_size) + 1)]
    else:
        grid = [(0, N, N)]
    out = np.zeros((C, N))
    per = {}
    for ich, (s0, e_full, e0) in enumerate(grid):
        i1, i2 = s0 - padding, e_full + padding
        chunk = O.read_chunk(y2, i1, i2)
        if stationary:
            res, stages = O.gate_stationary_S(chunk, thresh, n_fft, W, H, prop_decrease, filt, return_stages=True)
        else:
            res, stages = O.gate_nonstationary_S(chunk, n_fft, W, H, prop_decrease, filt, cfg["iir_b"],
                                                 thresh_n_mult_nonstationary, sigmoid_slope_nonstationary,
                                                 return_stages=True)
        k0, k1 = s0 - i1, s0 - i1 + (e0 - s0)
        for ci in range(C):
            st = stages[ci]
            # the final mask once more by direct summation: O.conv2_same goes through an FFT whose ~1e-17 noise is all
            # there is where the exact mask is 0 (fully gated cells); the kernels' exact zeros must not be judged by it
            mask = _final_mask(st["raw"], cfg)
            assert np.max(np.abs(mask - st["mask"])) < 1e-13
            yy = O.istft_scipy(st["Z"] * mask, n_fft, W, H)
            yfull = np.zeros(chunk.shape[1])
            yfull[:min(len(yy), len(yfull))] = yy[:len(yfull)]
            assert np.max(np.abs(yfull - res[ci])) <= 1e-13 * max(1.0, np.max(np.abs(res[ci])))
            out[ci, s0:e0] = yfull[k0:k1]
            per[(ci, ich)] = dict(ch=ci, chunk=ich, x=chunk[ci], Z=st["Z"], raw=st["raw"], mask=mask, thresh=thresh,
                                  db=O.amp_to_db(st["Z"], 80.0) if stationary else None, y=yfull, keep=(k0, k1),
                                  dst=(s0, e0), want=yfull[k0:k1], cfg=cfg)
    units = [per[(ci, ich)] for ci in range(C) for ich in range(len(grid))]
    return (out[0] if flat else out), units


def torchgate_units(x, sr, xn=None, window=None, **kw):
    """``O.torchgate_T(return_stages=True)`` as one unit per batch row (same keys as ``oracle_units``; ``keep`` is the
    whole output row).  ``window``: the (W,) table the engine was given (TorchGate: float32 Hann)."""
    x = np.asarray(x, dtype=np.float64)
    n_fft, W, H = O.resolve_stft_params(kw.get("n_fft", 1024), kw.get("win_length"), kw.get("hop_length"))
    y, st = O.torchgate_T(x, sr, xn=xn, window=window, return_stages=True, **kw)
    nonstat = bool(kw.get("nonstationary", False))
    nf, nt, smooth = O.mask_smoothing_widths(sr, n_fft, H, kw.get("freq_mask_smooth_hz", 500),
                                             kw.get("time_mask_smooth_ms", 50))
    cfg = dict(variant="T", stationary=not nonstat, n_fft=n_fft, W=W, H=H, prop=float(kw.get("prop_decrease", 1.0)),
               nf=nf, nt=nt, filt=O.smoothing_filter(nf, nt) if smooth else None, window=window,
               n_movemean=kw.get("n_movemean_nonstationary", 20), n_thresh=kw.get("n_thresh_nonstationary", 1.3),
               temp=kw.get("temp_coeff_nonstationary", 0.1))
    units = []
    y = np.array(y)
    for b in range(x.shape[0]):
        mask = _final_mask(st["raw"][b], cfg)
        assert np.max(np.abs(mask - st["mask"][b])) < 1e-13
        yb = O.istft_torch((st["X"][b] * mask)[None], n_fft, W, H, window)[0]
        assert np.max(np.abs(yb - y[b])) <= 1e-13 * max(1.0, np.max(np.abs(y[b])))
        y[b] = yb
        units.append(dict(ch=b, chunk=0, x=x[b], Z=st["X"][b], raw=st["raw"][b], mask=mask,
                          thresh=None if nonstat else st["thresh"][b if st["thresh"].shape[0] > 1 else 0],
                          db=None if nonstat else O.amp_to_db(st["X"][b], 40.0), y=yb, keep=(0, y.shape[1]),
                          dst=(0, y.shape[1]), want=yb, cfg=cfg))
    return y, units


def regate(unit, raw=None, mask=None):
    """The oracle's float64 output of ``unit`` (Lp,) with a stage replaced: ``raw`` (stationary decision bits; the
    smoothing is redone) or ``mask`` (the final mask).  For planting defects in the oracle's own stages."""
    c = unit["cfg"]
    if mask is None:
        mask = smooth_mask(unit["raw"] if raw is None else raw, c)
    if c["variant"] == "S":
        yy = O.istft_scipy(unit["Z"] * mask, c["n_fft"], c["W"], c["H"])
    else:
        yy = O.istft_torch((unit["Z"] * mask)[None], c["n_fft"], c["W"], c["H"], c["window"])[0]
    out = np.zeros(len(unit["y"]))
    out[:min(len(yy), len(out))] = yy[:len(out)]
    return out


def smooth_mask(raw, cfg):
    """Stationary gates: decision bits -> final mask, as the oracle does it (float64)."""
    assert cfg["stationary"]
    return _final_mask(raw, cfg)


# ----------------------------------------------------------------------------------------------------------------
# the same operation in float32
# ----------------------------------------------------------------------------------------------------------------
def _conv2_same_f32(m, K):
    """Zero-padded centred 2-D convolution by direct summation, every product and sum in float32."""
    K = np.asarray(K, dtype=F32)
    a, b = K.shape
    ha, hb = (a - 1) // 2, (b - 1) // 2
    P = np.zeros((m.shape[0] + a - 1, m.shape[1] + b - 1), dtype=F32)
    P[ha:ha + m.shape[0], hb:hb + m.shape[1]] = m
    out = np.zeros(m.shape, dtype=F32)
    for i in range(a):
        for j in range(b):
            out += K[a - 1 - i, b - 1 - j] * P[i:i + m.shape[0], j:j + m.shape[1]]
    return out


def _filtfilt_onepole_f32(b, A):
    b, one_b = F32(b), F32(1.0 - b)
    T = A.shape[-1]
    fwd = np.empty_like(A)
    prev = A[..., 0].copy()
    for t in range(T):
        prev = b * A[..., t] + one_b * prev
        fwd[..., t] = prev
    out = np.empty_like(A)
    prev = fwd[..., T - 1].copy()
    for t in range(T - 1, -1, -1):
        prev = b * fwd[..., t] + one_b * prev
        out[..., t] = prev
    return out


def _boxcar_same_f32(A, k):
    T = A.shape[-1]
    left = (k - 1) // 2
    P = np.zeros(A.shape[:-1] + (T + k - 1,), dtype=F32)
    P[..., left:left + T] = A
    s = np.zeros_like(A)
    for j in range(k):
        s += P[..., j:j + T]
    return s / F32(k)


def _sigmoid_f32(r, shift, mult):
    with np.errstate(over="ignore"):
        return (F32(1.0) / (F32(1.0) + np.exp(-(r + F32(shift)) * F32(mult)))).astype(F32)


def emulate_stages_f32(unit):
    """``(y32, raw32, mask32)`` of a unit evaluated in float32 (see ``emulate_f32``)."""
    c = unit["cfg"]
    n_fft, W, H = c["n_fft"], c["W"], c["H"]
    x = np.asarray(unit["x"], dtype=F32)
    if c["variant"] == "S":
        w = O.hann_periodic(W).astype(F32)
        wsum = F32(np.sum(w.astype(np.float64)))
        p, n_frame = W // 2, W
        wf = w
    else:
        wf = O._centered_window(n_fft, W, c["window"]).astype(F32)
        p, n_frame = n_fft // 2, n_fft
    ext = np.concatenate([np.zeros(p, dtype=F32), x, np.zeros(p, dtype=F32)])
    T = (ext.shape[0] - n_frame) // H + 1
    idx = np.arange(n_frame)[None, :] + H * np.arange(T)[:, None]
    frames = ext[idx] * wf[None, :]
    Z = scipy.fft.rfft(frames, n=n_fft, axis=-1)
    assert Z.dtype == np.complex64, "scipy.fft left float32"
    if c["variant"] == "S":
        Z = Z * (F32(1.0) / wsum)
    Z = Z.T                                                   # (F, T) complex64
    # ---- mask ----
    raw32 = None
    if c["stationary"]:
        mask = np.asarray(unit["mask"], dtype=np.float64).astype(F32)   # decisions are exact: not part of the budget
    else:
        A = np.abs(Z).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            if c["variant"] == "S":
                S = _filtfilt_onepole_f32(c["iir_b"], A)
                raw32 = _sigmoid_f32((A - S) / S, -c["thresh_n_mult"], c["slope"])
            else:
                S = _boxcar_same_f32(A, c["n_movemean"])
                raw32 = _sigmoid_f32((A - S) / S, -c["n_thresh"], 1.0 / c["temp"])
        prop = F32(c["prop"])
        if c["variant"] == "S":
            m = _conv2_same_f32(raw32, c["filt"]) if c["filt"] is not None else raw32
            mask = m * prop + F32(1.0 - c["prop"])
        else:
            m = prop * (raw32 - F32(1.0)) + F32(1.0)
            mask = _conv2_same_f32(m, c["filt"]) if c["filt"] is not None else m
        mask = mask.astype(F32)
    # ---- masked inverse transform, overlap-add, envelope ----
    xs = scipy.fft.irfft((Z * mask).T, n=n_fft, axis=-1)      # (T, n_fft) float32
    assert xs.dtype == F32
    if c["variant"] == "S":
        xs = xs[:, :W] * wsum
    out_len = n_frame + (T - 1) * H
    acc = np.zeros(out_len, dtype=F32)
    env = np.zeros(out_len, dtype=F32)
    w2 = wf * wf
    for t in range(T):
        acc[t * H:t * H + n_frame] += xs[t] * wf
        env[t * H:t * H + n_frame] += w2
    acc, env = acc[p:out_len - p], env[p:out_len - p]
    if c["variant"] == "S":
        yy = acc / np.where(env > F32(1e-10), env, F32(1.0))
    else:
        yy = acc / env
    out = np.zeros(len(unit["y"]), dtype=F32)
    out[:min(len(yy), len(out))] = yy[:len(out)]
    return out, raw32, mask


def emulate_f32(unit):
    """The unit's gate in the kernels' arithmetic, as a plain reference: frames and window in float32, scipy.fft's
    rfft / irfft on float32 (complex64 throughout), mask multiply, overlap-add and envelope division in float32.
    Stationary: the mask is the oracle's float64 mask rounded to float32.  Non-stationary: |X|, the forward-backward
    one-pole recurrence (variant T: the moving mean), the sigmoid and the smoothing are float32 too.  Returns the gated
    padded chunk (Lp,) float32, laid out like ``unit['y']``."""
    return emulate_stages_f32(unit)[0]


# ----------------------------------------------------------------------------------------------------------------
# metrics
# ----------------------------------------------------------------------------------------------------------------
def _blocks(v, H):
    """max |v| per block of H samples (the last block may be short)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    nb = -(-len(v) // H)
    padded = np.zeros(nb * H)
    padded[:len(v)] = v
    return padded.reshape(nb, H).max(axis=1) if nb else np.zeros(0)


def _pool(v, r=POOL):
    """v[b] -> max(v[b - r .. b + r])."""
    n = len(v)
    out = np.array(v, dtype=np.float64)
    for d in range(1, r + 1):
        out[d:] = np.maximum(out[d:], v[:n - d])
        out[:n - d] = np.maximum(out[:n - d], v[d:])
    return out


def local_error(got, want, H):
    """Per hop block b of the kept range: max |got - want|."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return _blocks(got - want, H)


def budget(unit, emu=None):
    """Per hop block: max |emulate_f32 - want| over blocks b - 2 .. b + 2 (a rounding error is a random variable; one
    block's maximum is too noisy to divide by)."""
    k0, k1 = unit["keep"]
    emu = emulate_f32(unit) if emu is None else emu
    return _pool(local_error(emu[k0:k1], unit["want"], unit["cfg"]["H"]))


def allowed_f32(unit, bud=None):
    """What a float32 kernel's block may be off by: FACTOR * budget[b] + 4 eps32 max |want| over b - 2 .. b + 2."""
    bud = budget(unit) if bud is None else bud
    return FACTOR * bud + 4.0 * EPS32 * _pool(_blocks(unit["want"], unit["cfg"]["H"]))


def allowed_f64(unit, global_peak):
    """float64 pipeline: 1e-12 of the block's own peak, floored at 1e-12 of 1e-3 of the global peak."""
    return F64_REL * np.maximum(_blocks(unit["want"], unit["cfg"]["H"]), 1e-3 * global_peak)


def local_check(got, unit, bud=None, precision="float32", global_peak=None):
    """got: the kernel's kept samples of this unit.  Returns ``(bad_blocks, ratio)``: indices of hop blocks over their
    bound, and the largest local_error / budget over blocks with a non-zero budget (float32), or the largest
    local_error / bound (float64)."""
    err = local_error(got, unit["want"], unit["cfg"]["H"])
    if precision == "float64":
        ok = allowed_f64(unit, global_peak)
        return np.flatnonzero(err > ok), float(np.max(err / ok)) if len(err) else 0.0
    bud = budget(unit) if bud is None else bud
    ok = allowed_f32(unit, bud)
    nz = bud > 0
    ratio = float(np.max(err[nz] / bud[nz])) if np.any(nz) else 0.0
    return np.flatnonzero(err > ok), ratio


def bit_diff(bits, unit, delta_db=DELTA_DB, frames=None):
    """Kernel decision bits (F, T) against the oracle's ``raw``, over frames ``[d0, d1)`` (default: all), leaving out
    cells with |dB - thresh| <= delta_db.  Returns ``(cells, left_out)``: an (n, 2) array of differing (band, frame)
    cells, and the share of the compared cells that was left out."""
    d0, d1 = (0, unit["raw"].shape[1]) if frames is None else frames
    bits = np.asarray(bits, dtype=bool)
    assert bits.shape == unit["raw"].shape, (bits.shape, unit["raw"].shape)
    amb = np.abs(unit["db"] - unit["thresh"][:, None]) <= delta_db
    diff = (bits != unit["raw"].astype(bool)) & ~amb
    cells = np.argwhere(diff[:, d0:d1])
    cells[:, 1] += d0
    left = float(np.mean(amb[:, d0:d1])) if d1 > d0 else 0.0
    return cells, left


def nearest_margin_db(unit):
    """Smallest |dB - thresh| of a stationary unit (how far the oracle itself is from an ambiguous decision)."""
    return float(np.min(np.abs(unit["db"] - unit["thresh"][:, None])))


def mask_bound(cfg, integer_taps=True):
    """Stationary float32 smoothed mask against the oracle's.  Where the smoothing is exact integer arithmetic over the
    filter's integer taps (the bit-mask stages: uint16 sums / ktot): 2^-23 (prop_decrease = 1), else 3 * 2^-24.
    ``integer_taps=False``: the materialised route (SG_OPT_FORCE_UNFUSED) convolves a float field with float taps in two
    separable float32 passes; the premise of the bound above does not hold there.  The standard dot-product bound does:
    a pass of n = 2 m + 1 taps errs by at most (n + 1) u of sum |tap x value| <= 1 (n - 1 additions, n products, the
    taps' own rounding; u = 2^-24), the second pass carries the first one's error through weights that sum to 1, and
    p x acc + (1 - p) x edge adds 3 u: (2 nf + 2 nt + 7) u.  Still 100 x under the smallest tap at the widths used here."""
    if integer_taps:
        return 2.0 ** -23 if cfg["prop"] == 1.0 else 3.0 * 2.0 ** -24
    return (2 * cfg["nf"] + 2 * cfg["nt"] + 7) * 2.0 ** -24


def mask_diff(M, unit, frames=None, bound=None):
    """Cells (band, frame) of ``[d0, d1)`` where a float mask field differs from the oracle's final mask by more than
    ``bound`` (default ``mask_bound``), and the largest difference."""
    d0, d1 = (0, unit["mask"].shape[1]) if frames is None else frames
    M = np.asarray(M, dtype=np.float64)
    assert M.shape == unit["mask"].shape, (M.shape, unit["mask"].shape)
    d = np.abs(M - unit["mask"])[:, d0:d1]
    bound = mask_bound(unit["cfg"]) if bound is None else bound
    cells = np.argwhere(d > bound)
    cells[:, 1] += d0
    return cells, float(d.max()) if d.size else 0.0


# ----------------------------------------------------------------------------------------------------------------
# the matrix shared by tests/test_parity_budget_host.py (conditions on the oracle) and tests/test_gpu_stagewise.py
# ----------------------------------------------------------------------------------------------------------------
SR = 48000
FAMILIES = {
    "register": [1024, 512, 256, 2048],          # one-pass register gates (and the same with SG_OPT_FORCE_SPLIT)
    "lds_pow2": [64, 128, 4096, 8192],           # general LDS power of two, sub-wavefront teams
    "mixed_radix": [400, 1000, 1536, 3000, 4000],
    "chirp_z": [777, 601, 5000],
    "four_step": [16384],
}
# column settings; every family meets each one (the n_fft of a family rotate through them)
COLUMNS = [
    dict(stationary=True, layout="one", C=1, signal="two_level", y_noise="quiet"),
    dict(stationary=True, layout="grid_pad", C=3, signal="dc_nyquist", y_noise=True),
    dict(stationary=True, layout="grid_nopad", C=1, signal="bin_centred", prop_decrease=0.7, dtype="float64"),
    dict(stationary=True, layout="grid_pad", C=1, signal="burst_at_seam", short_window=True),
    dict(stationary=False, layout="one", C=3, signal="dc_nyquist"),
    dict(stationary=False, layout="grid_pad", C=1, signal="two_level", prop_decrease=0.7, dtype="float64"),
    dict(stationary=False, layout="grid_nopad", C=1, signal="burst_at_seam", short_window=True),
    dict(stationary=True, layout="grid_pad", C=1, signal="two_level", y_noise="quiet", dtype="float64", precision="float64"),
    dict(stationary=False, layout="one", C=1, signal="bin_centred", dtype="float64", precision="float64"),
]


# a seed that lands a decision within 1e-6 dB of its threshold is changed (tests/test_parity_budget_host.py checks)
_RESEED = {(8192, 7): 1}


# The rotation below hands a size whatever columns its position gives it.  A register geometry only exists with
# win_length = n_fft and hop = n_fft / 4 and outside the float64 pipeline, so EVERY register size also gets, explicitly,
# the float32 stationary chunk grid (column 1: one-pass gate and its FORCE_SPLIT form) and a float32 non-stationary
# cell with the default window (column 4); mixed radix 4000 gets the stationary grid (fused bit-mask route) too.
_EXPLICIT = [("register", n, col) for n in (1024, 512, 256, 2048) for col in (1, 4)] + [("mixed_radix", 4000, 1)]


def _cells():
    cells, seen = [], set()

    def add(fam, n_fft, col):
        if (fam, n_fft, col) not in seen:
            seen.add((fam, n_fft, col))
            cells.append(dict(COLUMNS[col], family=fam, n_fft=n_fft, col=col))
    for fam, sizes in FAMILIES.items():
        # every size of the family at least once, every column at least once
        for i in range(max(len(COLUMNS), len(sizes))):
            add(fam, sizes[i % len(sizes)], i % len(COLUMNS))
    for fam, n_fft, col in _EXPLICIT:
        add(fam, n_fft, col)
    return cells


CELLS = _cells()


def kernel_family(c):
    """The kernels a cell really runs: a register size with win_length < n_fft / an odd hop has no register geometry
    and runs the general LDS power-of-two kernels."""
    return "lds_pow2" if c["family"] == "register" and c.get("short_window") else c["family"]


def cell_id(c):
    tag = "(runs lds_pow2)" if kernel_family(c) != c["family"] else ""
    return "%s-%d-c%d%s%s" % (c["family"], c["n_fft"], c["col"], "-shortwin" if c.get("short_window") else "", tag)


@functools.lru_cache(maxsize=None)
def _cell_case(family, n_fft, col):
    c = dict(COLUMNS[col], family=family, n_fft=n_fft, col=col)
    if c.get("short_window"):
        W = (3 * n_fft) // 4
        H = (W // 4) | 1                           # an odd hop
    else:
        W, H = n_fft, n_fft // 4
    frames = 8 if n_fft >= 16384 else 32           # frames per chunk (+ 2 x 2 or 4 of padding)
    pad_frames = 2 if n_fft >= 16384 else 4
    cs = frames * H + 5
    pad = 0 if c["layout"] == "grid_nopad" else pad_frames * H + 3
    N = cs - 9 if c["layout"] == "one" else 2 * cs + cs // 3
    kw = dict(stationary=c["stationary"], n_fft=n_fft, chunk_size=cs, padding=pad, prop_decrease=c.get("prop_decrease", 1.0))
    if c.get("short_window"):
        kw.update(win_length=W, hop_length=H)
    if n_fft not in (1024, 512, 256, 2048) or c.get("short_window"):
        # the default 500 Hz / 50 ms do not exist at every size: three bins, two frames
        kw.update(freq_mask_smooth_hz=3.02 * SR / (n_fft / 2), time_mask_smooth_ms=2.02 * H / SR * 1000)
    seed = 1000 * col + n_fft % 997 + _RESEED.get((n_fft, col), 0)
    C = c["C"]
    gen = {"two_level": lambda s: signals.two_level(N, SR, s), "dc_nyquist": lambda s: signals.dc_nyquist(N, SR, s),
           "bin_centred": lambda s: signals.bin_centred(N, n_fft, s),
           "burst_at_seam": lambda s: signals.burst_at_seam(N, cs, pad, SR, s)}[c["signal"]]
    y = np.stack([gen(seed + 17 * ci) for ci in range(C)]) if C > 1 else gen(seed)
    y_noise = None
    if c.get("y_noise"):
        # "quiet": room tone at the level of two_level's quiet half, so that its loud half passes and the quiet half's
        # tone stands over a gated floor (with the recording's own statistics two_level is gated to silence)
        sigma = 1e-4 if c["y_noise"] == "quiet" else 0.1
        y_noise = (sigma * np.random.default_rng(seed + 5).standard_normal(max(24 * H, 2 * W))).astype(F32)
    return dict(cell=c, y=y, y_noise=y_noise, kw=kw, dtype=c.get("dtype", "float32"), precision=c.get("precision"))


def cell_case(c):
    """Input and keyword arguments of a matrix cell: ``dict(cell, y, y_noise, kw, dtype, precision)``; ``y`` is float32
    valued (C, N) or (N,); ``kw`` goes to reduce_noise / ``oracle_units`` alike (sr = SR)."""
    return _cell_case(c["family"], c["n_fft"], c["col"])


@functools.lru_cache(maxsize=8)
def _cell_oracle(family, n_fft, col):
    case = _cell_case(family, n_fft, col)
    return oracle_units(case["y"].astype(np.float64), SR,
                        y_noise=None if case["y_noise"] is None else case["y_noise"].astype(np.float64), **case["kw"])


def cell_oracle(c):
    return _cell_oracle(c["family"], c["n_fft"], c["col"])


# TorchGate.forward cells: (n_fft, rows, lengths?, xn?, nonstationary)
T_CELLS = [
    dict(n_fft=1024, B=160, path="row_gate"),
    dict(n_fft=1024, B=6, path="four_kernel", xn=True),
    dict(n_fft=1024, B=5, path="rows", lengths=True),
    dict(n_fft=512, B=4, path="four_kernel"),
    dict(n_fft=512, B=5, path="rows", lengths=True, xn=True),
    dict(n_fft=2048, B=3, path="four_kernel", xn=True),
    dict(n_fft=2048, B=4, path="rows", lengths=True),
    dict(n_fft=400, B=3, path="four_kernel"),
    dict(n_fft=400, B=3, path="rows", lengths=True),
    dict(n_fft=1024, B=3, path="four_kernel", nonstationary=True),
]
T_SR = 16000


def t_cell_id(c):
    return "%d-%s%s%s" % (c["n_fft"], c["path"], "-xn" if c.get("xn") else "", "-ns" if c.get("nonstationary") else "")


@functools.lru_cache(maxsize=None)
def _t_case(i):
    c = T_CELLS[i]
    n_fft, B = c["n_fft"], c["B"]
    H = n_fft // 4
    L = 60 * H + 13 if c["path"] != "row_gate" else 16000        # row gate: rows of <= 64 frames (1 s at 16 kHz: 63)
    rng = np.random.default_rng(900 + i)
    kinds = [signals.two_level, signals.dc_nyquist]
    x = np.stack([kinds[b % 2](L, T_SR, 50 * i + b) if b < 8 else signals.two_level(L, T_SR, 50 * i + b)
                  for b in range(B)])
    lengths = None
    if c.get("lengths"):
        lengths = np.array([L] + [int(v) for v in rng.integers(2 * n_fft, L, size=B - 1)], dtype=np.int64)
    xn = (0.1 * rng.standard_normal((1, 30 * H))).astype(F32) if c.get("xn") else None
    kw = dict(n_fft=n_fft, nonstationary=bool(c.get("nonstationary", False)))
    if n_fft not in (1024, 512):
        kw.update(freq_mask_smooth_hz=3.02 * T_SR / (n_fft / 2), time_mask_smooth_ms=2.02 * H / T_SR * 1000)
    return dict(cell=c, x=x, xn=xn, lengths=lengths, kw=kw)


def t_case(i):
    return _t_case(i)
