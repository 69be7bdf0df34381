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
* ``mask_bound``       what a float32 smoothed mask may differ from the oracle's by;
* ``TILE_CELLS``       the matrix of the three table-driven paths (clips, rows, streams);
* ``adjoint_f64`` / ``emulate_adjoint_f32`` / ``adjoint_unit`` / ``B_CELLS``   TorchGate's backward: the float64 adjoint of
                       the fixed-mask gate, the same in the kernels' arithmetic, and the matrix of the backward routes,
                       further down;
* ``F_CELLS`` / ``floor_gate_case`` / ``S_CLIPS`` / ``floor_stats_case``   the -80 dB floor band by band: gate inputs with
                       a few lifted bands per unit and one band +g / -g dB from its switch, and noise clips that reach
                       every branch of the single-pass statistics;
* ``R_CELLS`` / ``r_case`` / ``r_oracle`` / ``r_budget``   the routes of TorchGate.forward without lengths= (rows per unit batch,
                       frames per row, noise rows, unit batches) on rows that all differ from each other;
* ``W_CELLS`` / ``TW_CELLS`` / ``M_CELLS`` / ``w_route`` / ``tw_route``   mask smoothing half-widths and moving-mean lengths on
                       both sides of every edge the engine routes on, with the routing predicates restated, at the end of
                       the module.

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

    @staticmethod
    def dappled(n, n_fft, blocks, sigma, seed):
        """Three kinds of block for the width matrix (``W_CELLS``); ``blocks``: (start, stop, kind) sample ranges.

        ``loud``    every decision is 1, in every band and frame that lies inside the block, by construction and not by
                    chance: one sinusoid on every bin centre k = 0 .. n_fft / 2 (DC and Nyquist included), equal
                    amplitudes, phases pi k^2 / 4, rms 0.25.  Under a Hann window of n_fft samples bin k holds
                    c_k - (c_{k-1} + c_{k+1}) / 2; a hop of n_fft / 4 turns neighbouring bins by pi / 2 against each other,
                    and with these phases the neighbours always stand at an odd multiple of pi / 4 to c_k: no frame's bin
                    falls more than 10.7 dB under the single tone.  DC and Nyquist carry twice the amplitude: a real bin
                    holds c_0 - Re(c_1 e^(i theta)), which vanishes at some frame offsets theta with equal amplitudes.
                    Over every frame offset and bin the windowed tone sum then stays within 3.0 dB of one tone alone
                    (8.3 dB at the odd size 601; summed numerically), 30 dB over the noise clip's mean at ``sigma`` = -40 dB.
        ``steady``  (non-stationary cells) tones on every fourth bin only, so that no two leak into the same bin and every
                    |X| is the same in every frame inside the block, over noise at ``sigma``: the sigmoid saturates at
                    the block's onset and decays with the recurrence, instead of hovering mid-slope on the 4-frame
                    pattern of ``loud`` (where the float32 emulation's error, times the slope, is no fair yardstick).
        ``sparse``  white noise 1 dB over the noise clip's own level ``sigma``: the threshold (mean + 1.5 std of the
                    clip's dB) lies 5.85 dB over the clip's mean power for a complex Gaussian bin, which a bin at the clip's
                    level passes with probability exp(-3.85) = 2.1 % -- on the edge of the density the host test wants; at
                    + 1 dB it is exp(-3.05) = 4.7 %.
        ``quiet``   white noise 20 dB under the clip: no decision is 1.
        Samples outside every block are zero."""
        rng = np.random.default_rng(seed)
        F = n_fft // 2 + 1
        k = np.arange(F, dtype=np.float64)
        spec = (n_fft / 2.0) * np.exp(1j * np.pi * k * k / 4.0)
        spec[0] = 4.0 * spec[0].real            # (a real bin holds the whole amplitude, a complex one half of it; x 2)
        if n_fft % 2 == 0:
            spec[-1] = 4.0 * spec[-1].real
        period = np.fft.irfft(spec, n=n_fft)
        period *= 0.25 / np.sqrt(np.mean(period ** 2))
        steady = np.fft.irfft(np.where(np.arange(F) % 4 == 0, spec, 0.0), n=n_fft)
        steady *= 0.25 / np.sqrt(np.mean(steady ** 2))
        y = np.zeros(n)
        for a, b, kind in blocks:
            a, b = max(0, a), min(n, b)
            if b <= a:
                continue
            if kind == "loud":
                y[a:b] = period[np.arange(a, b) % n_fft]
            elif kind == "steady":
                y[a:b] = steady[np.arange(a, b) % n_fft] + sigma * rng.standard_normal(b - a)
            else:
                y[a:b] = sigma * {"sparse": 10.0 ** (1.0 / 20.0), "quiet": 0.1}[kind] * rng.standard_normal(b - a)
        return y.astype(F32)


# ----------------------------------------------------------------------------------------------------------------
# the oracle, unit by unit
# ----------------------------------------------------------------------------------------------------------------
def _final_mask(raw, cfg):
    """raw bits / raw sigmoid -> final mask in float64 with the smoothing summed directly (O.conv2_same_direct)."""
    raw = np.asarray(raw, dtype=np.float64)
    conv = (lambda m: O.conv2_same_direct(m, cfg["filt"])) if cfg["filt"] is not None else (lambda m: m)
    if cfg["filt"] is not None and cfg.get("separable"):
        conv = lambda m: conv2_same_separable(m, cfg["nf"], cfg["nt"])   # noqa: E731
    if cfg["variant"] == "T":
        return conv(cfg["prop"] * (raw - 1.0) + 1.0)
    if cfg["stationary"]:
        return conv(raw * cfg["prop"] + (1.0 - cfg["prop"]))
    return conv(raw) * cfg["prop"] + (1.0 - cfg["prop"])


def conv2_same_separable(m, nf, nt, drop_f=False, drop_t=False, replicate=False):
    """``O.conv2_same_direct(m, O.smoothing_filter(nf, nt))`` summed axis by axis in float64 with the filter's INTEGER
    taps [1 .. n + 1 .. 1] and one division by (nf + 1)^2 (nt + 1)^2 at the end (a field of 0 / 1 decisions is summed
    exactly): 2 nf + 2 nt + 2 passes over the field instead of (2 nf + 1)(2 nt + 1).  tests/test_smoothing_widths_host.py
    holds it against the direct sum.  The three switches plant defects: the taps at |df| = nf / |dt| = nt left out (the
    divisor stays), frames beyond the field replicated from frame 0 / T - 1 instead of zero."""
    m = np.asarray(m, dtype=np.float64)
    F, T = m.shape
    P = np.zeros((F + 2 * nf, T))
    P[nf:nf + F] = m
    a = np.zeros((F, T))
    for d in range(-nf, nf + 1):
        if not (drop_f and abs(d) == nf):
            a += (nf + 1 - abs(d)) * P[nf + d:nf + d + F]
    P = np.zeros((F, T + 2 * nt))
    P[:, nt:nt + T] = a
    if replicate:
        P[:, :nt] = a[:, :1]
        P[:, nt + T:] = a[:, -1:]
    out = np.zeros((F, T))
    for d in range(-nt, nt + 1):
        if not (drop_t and abs(d) == nt):
            out += (nt + 1 - abs(d)) * P[:, nt + d:nt + d + T]
    return out / float((nf + 1) ** 2 * (nt + 1) ** 2)


def oracle_units(y, sr, stationary=False, y_noise=None, prop_decrease=1.0, time_constant_s=2.0,
                 freq_mask_smooth_hz=500, time_mask_smooth_ms=50, thresh_n_mult_nonstationary=2,
                 sigmoid_slope_nonstationary=10, n_std_thresh_stationary=1.5, chunk_size=600000, padding=30000,
                 n_fft=1024, win_length=None, hop_length=None, clip_noise_stationary=True, separable=False):
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
               filt=filt, iir_b=None, thresh_n_mult=thresh_n_mult_nonstationary, slope=sigmoid_slope_nonstationary,
               separable=bool(separable))      # (the final mask summed axis by axis: conv2_same_separable)
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


def torchgate_units(x, sr, xn=None, window=None, separable=False, **kw):
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
               temp=kw.get("temp_coeff_nonstationary", 0.1), separable=bool(separable))
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


def _spectrum_f32(unit):
    """The unit's transform in float32: ``(Z (F, T) complex64, wf, wsum, p, n_frame, T)``."""
    c = unit["cfg"]
    n_fft, W, H = c["n_fft"], c["W"], c["H"]
    x = np.asarray(unit["x"], dtype=F32)
    wsum = None
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
    return Z.T, wf, wsum, p, n_frame, T                       # (F, T) complex64


def spectrum_f32(unit):
    """(F, T) complex64: the unit's float32 transform (float32 frames, window, pocketfft) alone."""
    return _spectrum_f32(unit)[0]


def emulate_stages_f32(unit):
    """``(y32, raw32, mask32)`` of a unit evaluated in float32 (see ``emulate_f32``)."""
    c = unit["cfg"]
    n_fft, W, H = c["n_fft"], c["W"], c["H"]
    Z, wf, wsum, p, n_frame, T = _spectrum_f32(unit)
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


# ----------------------------------------------------------------------------------------------------------------
# non-stationary float fields (tests/test_gpu_stagewise.py, tests/test_gpu_tile_parity.py)
# ----------------------------------------------------------------------------------------------------------------
def _field_rule(M, want, emu, what):
    """Non-stationary float fields (<= 1): max |M - want| over the unit's field within FACTOR x the float32 emulation's
    largest error over the same field + 4 eps32.  The budget is pooled over the WHOLE field, not over five columns as
    for the output: a cell's error is the transform's error (~eps32 of the frame's peak bin, whatever |X| is) times
    slope x m (1 - m) / S, which spans orders of magnitude from cell to cell -- the field's maximum sits in the few
    cells that are both mid-slope and far below the frame's peak, and which frames hold such a cell differs between
    two correct float32 transforms.  (Per column over t - 2 .. t + 2 this rule measured 9.7 x in one column of
    mixed_radix-400-c5, all of it one such cell: band 192, frame 18, |X| = 2.6e-3 of the peak bin, kernel 0.5 eps32
    of that peak off.)"""
    err = np.abs(M.astype(np.float64) - want)
    bud = float(np.max(np.abs(emu.astype(np.float64) - want)))
    f, t = np.unravel_index(np.argmax(err), err.shape)
    assert err[f, t] <= FACTOR * bud + 4 * EPS32, "%s: off by %.3g at (band %d, frame %d); the emulation's largest " \
                                                        "error over the field is %.3g" % (what, err[f, t], f, t, bud)
    return err[f, t] / bud if bud > 0 else 0.0


# ----------------------------------------------------------------------------------------------------------------
# the tile matrix: the three table-driven paths (clips: csrc/ragged.hip, rows: csrc/rows.hip, stream: csrc/stream.hip),
# shared by tests/test_tile_parity_host.py (conditions on the oracle) and tests/test_gpu_tile_parity.py
# ----------------------------------------------------------------------------------------------------------------
# Shapes are in units of the hop and the smallest that still cross every seam of csrc/tile_core.hpp: 8 frames per
# transform tile (2 in the stream), 16 rows per smoothing tile, 256 positions per overlap-add tile, the 64-band words of
# a bit row (F = n_fft / 2 + 1 leaves the Nyquist bit alone in the last word).
#
# Two inputs of column T0 differ from "two_level over a sigma = 1e-4 profile", because the oracle itself says that input
# checks nothing there (tests/test_tile_parity_host.py holds both conditions):
# * rows-S: TorchGate floors a band at its maximum - 40 dB.  two_level's quiet half lies 60 dB down, so every cell of it
#   sits on the floor, 20 dB above a 1e-4 profile's threshold: the mask is all-pass.  The rows take two_level with the
#   quiet half 30 dB down (inside the 40 dB) and the profile at that half's level, sigma = 0.1 x 10^(-30/20).
# * stream-S: the offline oracle is the stream's truth only where no band's maximum - 80 dB exceeds its threshold (the
#   causal floor, tests/stream_model.py: ``live is False``).  two_level's 0.5 tone stands ~100 dB over a 1e-4 profile's
#   threshold in its band at n_fft = 4096.  The streams take the profile at sigma = 2e-3: the loud half passes, the
#   quiet half's noise is gated, its tone passes.
TILE_NFFT = (256, 512, 1024, 2048, 4096)
TILE_PATHS = ("clips-S", "clips-NS", "rows-S", "rows-NS", "stream-S", "stream-NS")
TILE_COLUMNS = [
    dict(name="T0", signal="two_level", prop=1.0, smooth="3x2", noise="quiet"),
    dict(name="T1", signal="dc_nyquist", prop=0.7, smooth="3x2", short_window=True),
    dict(name="T2", signal="bin_centred", prop=1.0, smooth="off", dtype="float64"),
    dict(name="T3", signal="burst_at_seam", prop=0.7, smooth="t9"),
]
# level of the noise clip a stationary cell is given where the path cannot take the statistics from the signal itself
_TILE_SIGMA = {"two_level": 1e-4, "dc_nyquist": 0.1, "bin_centred": 0.05, "burst_at_seam": 0.003}
_ROWS_QUIET = 10.0 ** (-30.0 / 20.0)
_STREAM_QUIET_SIGMA = 2e-3
# (path, n_fft, col) -> seed offset: a seed that lands a stationary decision within 1e-6 dB of its threshold, or leaves a
# non-stationary unit without a cell below 0.1 / above 0.9, is changed (tests/test_tile_parity_host.py checks)
_TILE_RESEED = {("rows-S", 256, 3): 7}


def _tile_cells():
    cells = []
    for p, path in enumerate(TILE_PATHS):
        for i, n_fft in enumerate(TILE_NFFT):
            for col in (0, 1 + (p + i) % 3):      # T0 plus one of T1..T3 by rotation
                cells.append(dict(TILE_COLUMNS[col], path=path, n_fft=n_fft, col=col, stationary=path.endswith("-S")))
    return cells


TILE_CELLS = _tile_cells()


def tile_cell_id(c):
    return "%s-%d-%s" % (c["path"], c["n_fft"], c["name"])


def _tile_geometry(n_fft, col):
    """(W, H, keyword arguments of the window and the smoothing) of a column."""
    c = TILE_COLUMNS[col]
    if c.get("short_window"):
        W = (3 * n_fft) // 4
        H = (W // 4) | 1
        kw = dict(n_fft=n_fft, win_length=W, hop_length=H)
    else:
        W, H = n_fft, n_fft // 4
        kw = dict(n_fft=n_fft)
    ms = 1000.0 * H / SR
    kw.update({"3x2": dict(freq_mask_smooth_hz=3.02 * SR / (n_fft / 2), time_mask_smooth_ms=2.02 * ms),
               "off": dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=None),
               "t9": dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=9.02 * ms)}[c["smooth"]])
    kw["prop_decrease"] = c["prop"]
    return W, H, kw


def _tile_signal(kind, n, seed, n_fft, cs, pad, quiet=1e-3):
    if kind == "two_level":
        y = signals._base(n, SR, seed)
        y[n // 2:] *= quiet
        return y.astype(F32)
    if kind == "dc_nyquist":
        return signals.dc_nyquist(n, SR, seed)
    if kind == "bin_centred":
        return signals.bin_centred(n, n_fft, seed)
    return signals.burst_at_seam(n, cs, pad, SR, seed)


def _tile_noise(sigma, n, seed):
    return (sigma * np.random.default_rng(seed).standard_normal(n)).astype(F32)


def _primes_near(x):
    """The prime closest to x from above."""
    p = max(2, int(x))
    while any(p % d == 0 for d in range(2, int(p ** 0.5) + 1)):
        p += 1
    return p


def stream_cuts(kind, N, W, H, rng):
    """Block plans of a stream of N samples (``whole`` / ``edge`` / ``random``: tests/test_gpu_stream.py's ``_cuts``)."""
    if kind == "whole":
        return []
    if kind == "edge":       # 1-sample blocks around the sample that completes a frame, and a few 0-sample blocks
        e = 3 * H - W // 2 + W
        return sorted(min(c, N) for c in (e - 3, e - 2, e - 1, e, e, e, e + 1, e + 2, N // 2, N // 2))
    if kind == "prime":      # blocks of a prime number of samples near 1.3 hops
        p = _primes_near(1.3 * H)
        return list(range(p, N, p))
    if kind == "random":
        return sorted(int(c) for c in rng.integers(0, N + 1, 7))
    raise KeyError(kind)


STREAM_PLANS = ("whole", "edge", "prime", "random")


def tile_window(W):
    """The (W,) table TorchGate hands the engine: torch's float32 Hann window, as float64 (torch is imported here only:
    a numpy float32 Hann may differ from torch's in the last bit, which is the size of the budget)."""
    import torch
    return torch.hann_window(W).double().numpy()


@functools.lru_cache(maxsize=None)
def _tile_case(path, n_fft, col):
    c = dict(TILE_COLUMNS[col], path=path, n_fft=n_fft, col=col, stationary=path.endswith("-S"))
    stationary = c["stationary"]
    W, H, kw = _tile_geometry(n_fft, col)
    dtype = c.get("dtype", "float32")
    kind = c["signal"]
    seed = 7000 * TILE_PATHS.index(path) + 100 * col + n_fft % 997 + _TILE_RESEED.get((path, n_fft, col), 0)
    nlen = max(24 * H, 2 * W)
    sigma = _TILE_SIGMA[kind]
    case = dict(cell=c, W=W, H=H, kw=kw, dtype=dtype, seed=seed)
    if path.startswith("clips"):
        cs, pad = 24 * H + 5, 4 * H + 3
        lens = [2 * cs + cs // 3, cs, cs + 1, W - 3, 8 * H * 3 - 1]
        chans = [1, 2, 1, 1, 2]
        ys = []
        for i, (n, C) in enumerate(zip(lens, chans)):
            ch = [_tile_signal(kind, n, seed + 31 * i + 7 * k, n_fft, cs, pad) for k in range(C)]
            if i == 2:        # time-reversed: the one kept sample of its second chunk (and that chunk's frames) is loud
                ch = [v[::-1].copy() for v in ch]
            ys.append(np.stack(ch) if C > 1 else ch[0])
        y_noise = None
        if stationary and col == 0:
            y_noise = _tile_noise(sigma, nlen, seed + 5)                      # one shared noise clip
        elif stationary:                                                      # per clip; clip 1 (2 channels) is its own
            y_noise = [None if i == 1 else _tile_noise(sigma * (1.0, 0.0, 0.5, 1.0, 0.7)[i], nlen, seed + 5 + i)
                       for i in range(len(ys))]                                # (profiles of different levels)
        case.update(ys=ys, y_noise=y_noise, kw=dict(kw, chunk_size=cs, padding=pad, stationary=stationary))
    elif path.startswith("rows"):
        L = 40 * H + 13
        lens = [L, 2 * W, 2 * W + 1, 15 * H + 3, 16 * H, 23 * H + H - 1, 24 * H + 1]      # T = 1 + n // H: .., 16, 17, 24, 25
        x = np.full((len(lens), L), np.nan, dtype=F32)
        for b, n in enumerate(lens):
            # (bursts at a quarter and inside the second half of the row: two 2 x H bursts in a 2 W row leave the row's own
            # statistics without a passing cell when they sit in the middle)
            x[b, :n] = _tile_signal(kind, n, seed + 31 * b, n_fft, n // 4, 2 * H, quiet=_ROWS_QUIET)
        xn = _tile_noise(0.1 * _ROWS_QUIET, nlen, seed + 5)[None, :] if (stationary and col == 0) else None
        case.update(x=x, lengths=np.array(lens, dtype=np.int64), xn=xn, kw=dict(kw, nonstationary=not stationary))
    else:
        C = 2 if col == 0 else 1
        N = W + 40 * H + 13
        ch = [_tile_signal(kind, N, seed + 7 * k, n_fft, N // 3, 4 * H) for k in range(C)]
        y = np.stack(ch) if C > 1 else ch[0]
        rng = np.random.default_rng(seed + 3)
        plans = {k: stream_cuts(k, N, W, H, rng) for k in STREAM_PLANS}
        noise = _tile_noise(_STREAM_QUIET_SIGMA if col == 0 else sigma, nlen, seed + 5) if stationary else None
        T = (N + 2 * (W // 2) - W) // H + 1
        case.update(y=y, C=C, plans=plans, y_noise=noise, frames=T, lookahead_ms=(T + 2) * H / SR * 1000.0,
                    kw=dict(kw, stationary=stationary, chunk_size=None, padding=0))
    return case


def tile_case(c):
    """Inputs of a tile cell (float32-valued arrays; ``dtype`` is what the call is given).  clips: ``ys``, ``y_noise``
    (None, one array, or a per-clip list), ``kw`` for reduce_noise_batch / ``oracle_units``.  rows: ``x`` (B, L) with
    NaN beyond ``lengths``, ``xn``, ``kw`` for TorchGate / ``torchgate_units``.  stream: ``y``, ``C``, ``plans`` {name:
    cuts}, ``y_noise``, ``lookahead_ms`` (covers the stream), ``kw`` for ``oracle_units``."""
    return _tile_case(c["path"], c["n_fft"], c["col"])


@functools.lru_cache(maxsize=6)
def _tile_oracle(path, n_fft, col):
    case = _tile_case(path, n_fft, col)
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)   # noqa: E731
    if path.startswith("clips"):
        yn = case["y_noise"]
        return [oracle_units(f64(y), SR, y_noise=f64(yn[i]) if isinstance(yn, list) else f64(yn), **case["kw"])[1]
                for i, y in enumerate(case["ys"])]
    if path.startswith("rows"):
        window = tile_window(case["W"])
        return [torchgate_units(f64(case["x"][b:b + 1, :int(n)]), SR, xn=f64(case["xn"]), window=window, **case["kw"])[1]
                for b, n in enumerate(case["lengths"])]
    return [oracle_units(f64(case["y"]), SR, y_noise=f64(case["y_noise"]), **case["kw"])[1]]


def tile_oracle(c):
    """The oracle's units of a tile cell: one list per clip / row / stream (channel-major, then chunks)."""
    return _tile_oracle(c["path"], c["n_fft"], c["col"])


def live_frames(unit):
    """First and last frame of a variant-S unit whose window reaches a kept sample."""
    c = unit["cfg"]
    k0, k1 = unit["keep"]
    T = unit["raw"].shape[1]
    h = c["W"] // 2
    lo = max(0, -(-(k0 + h - c["W"] + 1) // c["H"]))
    hi = min(T - 1, (k1 - 1 + h) // c["H"])
    return lo, hi


@functools.lru_cache(maxsize=None)
def causal_floor_case(n_fft):
    """The input of test_causal_floor_is_the_models_and_not_the_offline_one (tests/test_gpu_stream.py) at another n_fft:
    1e-5 noise, a 0.5 tone from the middle on, a 1e-5 noise profile -- the running band maximum lifts the floor above
    the threshold from the middle on, so the truth is the causal model (tests/stream_model.py), not the offline oracle.
    Returns ``dict(y, noise, kw, unit)``: ``unit`` is the offline oracle's with ``raw`` / ``mask`` / ``y`` / ``want`` redone
    under the causal floor (same keys; local_check / emulate_f32 apply as they stand)."""
    H = n_fft // 4
    rng = np.random.default_rng(11 + n_fft)
    N = n_fft + 40 * H + 13
    y = 1e-5 * rng.standard_normal(N)
    y[N // 2:] += 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(N - N // 2) / SR)
    y = y.astype(F32)
    noise = (1e-5 * rng.standard_normal(max(24 * H, 2 * n_fft))).astype(F32)
    kw = dict(n_fft=n_fft, stationary=True, chunk_size=None, padding=0, freq_mask_smooth_hz=3.02 * SR / (n_fft / 2),
              time_mask_smooth_ms=2.02 * 1000.0 * H / SR)
    _, units = oracle_units(y.astype(np.float64), SR, y_noise=noise.astype(np.float64), **kw)
    u = dict(units[0])
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(np.abs(u["Z"]) + O.EPS64)
    u["db"] = np.maximum(db, np.maximum.accumulate(db, axis=1) - 80.0)
    u["raw"] = u["db"] > u["thresh"][:, None]
    u["mask"] = smooth_mask(u["raw"], u["cfg"])
    u["y"] = regate(u, mask=u["mask"])
    k0, k1 = u["keep"]
    u["want"] = u["y"][k0:k1]
    return dict(y=y, noise=noise, kw=kw, unit=u, offline=units[0])


# ----------------------------------------------------------------------------------------------------------------
# TorchGate's backward (tests/test_backward_parity_host.py)
# ----------------------------------------------------------------------------------------------------------------
# y = D^-1 trim( OLA( Ws irfft( M rfft( Wa frames( pad(x) ) ) ) ) ) with the mask M fixed (O.stft_torch, O.istft_torch) is
# linear in x.  irfft(M rfft(.)) with a real M is a circular convolution with a real even kernel, hence its own adjoint;
# Wa = Ws = the window padded to n_fft.  So
#   g_x = trim_L( frames^T( Wa irfft( M rfft( Ws frames( pad( g_y / env ) ) ) ) ) )
# where frames^T is an UN-normalised overlap-add onto the padded input (L + 2 (n_fft // 2) samples) and trim_L drops
# the centre padding: all L input samples get a gradient, the tail [Lq, L) the forward never writes included.
def adjoint_geometry(cfg, L):
    """``(p, T, Lq)``: centre padding, frames, output samples of a row of L input samples (torch.stft / torch.istft)."""
    n_fft, H = cfg["n_fft"], cfg["H"]
    p = n_fft // 2
    T = 1 + (L + 2 * p - n_fft) // H
    return p, T, n_fft + (T - 1) * H - 2 * p


def adjoint_envelope(cfg, L):
    """torch.istft's window envelope after the n_fft // 2 trim, (Lq,) float64."""
    p, T, Lq = adjoint_geometry(cfg, L)
    w2 = O._centered_window(cfg["n_fft"], cfg["W"], cfg["window"]) ** 2
    env = np.zeros(cfg["n_fft"] + (T - 1) * cfg["H"])
    for t in range(T):
        env[t * cfg["H"]:t * cfg["H"] + cfg["n_fft"]] += w2
    return env[p:p + Lq]


def adjoint_frames_f64(gy, mask, cfg, L, env=None):
    """The per-frame terms of the adjoint before the scatter, (T, n_fft) float64: Wa irfft(M rfft(Ws frames(g_y / env))).
    ``env``: another envelope than ``adjoint_envelope`` (planted defects)."""
    n_fft, H = cfg["n_fft"], cfg["H"]
    p, T, Lq = adjoint_geometry(cfg, L)
    gy = np.asarray(gy, dtype=np.float64)
    mask = np.asarray(mask, dtype=np.float64)
    assert gy.shape == (Lq,) and mask.shape == (n_fft // 2 + 1, T), (gy.shape, mask.shape, Lq, T)
    wf = O._centered_window(n_fft, cfg["W"], cfg["window"])
    buf = np.zeros(n_fft + (T - 1) * H)
    buf[p:p + Lq] = gy / (adjoint_envelope(cfg, L) if env is None else env)
    idx = np.arange(n_fft)[None, :] + H * np.arange(T)[:, None]
    Z = np.fft.rfft(buf[idx] * wf[None, :], axis=-1) * mask.T
    return np.fft.irfft(Z, n=n_fft, axis=-1) * wf[None, :]


def adjoint_scatter(fr, cfg, L):
    """frames^T and the trim: (T, n_fft) per-frame terms -> (L,) gradient."""
    n_fft, H = cfg["n_fft"], cfg["H"]
    p, T, _ = adjoint_geometry(cfg, L)
    assert fr.shape == (T, n_fft)
    ext = np.zeros(L + 2 * p, dtype=fr.dtype)
    for t in range(T):
        ext[t * H:t * H + n_fft] += fr[t]
    return ext[p:p + L]


def adjoint_f64(gy, mask, cfg, L):
    """The gradient of ``O.istft_torch(O.stft_torch(x) * M)`` w.r.t. one row x of L samples, M fixed, in float64 numpy.
    gy: (Lq,);  mask: (F, T) float64;  cfg: the dict ``torchgate_units`` builds (n_fft, W, H, window).  Returns (L,)."""
    return adjoint_scatter(adjoint_frames_f64(gy, mask, cfg, L), cfg, L)


def emulate_adjoint_f32(gy, mask, cfg, L, window=None):
    """``adjoint_f64`` in the kernels' arithmetic: float32 envelope sums and g_y / env, float32 window, scipy.fft's
    rfft / irfft on float32, float32 mask multiply, float32 overlap-add.  ``window``: another (n_fft,) float32 table
    than the rounded ``cfg['window']`` (the false-positive control).  Returns (L,) float32."""
    n_fft, H = cfg["n_fft"], cfg["H"]
    p, T, Lq = adjoint_geometry(cfg, L)
    wf = O._centered_window(n_fft, cfg["W"], cfg["window"]).astype(F32) if window is None else np.asarray(window, dtype=F32)
    w2 = wf * wf
    env = np.zeros(n_fft + (T - 1) * H, dtype=F32)
    for t in range(T):
        env[t * H:t * H + n_fft] += w2
    buf = np.zeros(n_fft + (T - 1) * H, dtype=F32)
    buf[p:p + Lq] = np.asarray(gy, dtype=F32) / env[p:p + Lq]
    idx = np.arange(n_fft)[None, :] + H * np.arange(T)[:, None]
    Z = scipy.fft.rfft(buf[idx] * wf[None, :], n=n_fft, axis=-1)
    assert Z.dtype == np.complex64, "scipy.fft left float32"
    fr = scipy.fft.irfft(Z * np.asarray(mask, dtype=np.float64).astype(F32).T, n=n_fft, axis=-1) * wf[None, :]
    assert fr.dtype == F32
    return adjoint_scatter(fr, cfg, L)


def adjoint_unit(gy, mask, cfg, L):
    """A unit for ``local_error`` / ``budget`` / ``local_check`` as they stand: ``want`` the float64 gradient over
    ``keep = (0, L)``, ``emu`` the float32 emulation, ``bud`` its pooled per-hop-block error -- hand it on,
    ``local_check(got, u, bud=u['bud'])``: ``emulate_f32`` is the forward's.  ``mask`` is what the reference is GIVEN --
    on the GPU the float32 mask the engine saved for the forward."""
    u = dict(gy=np.asarray(gy, dtype=np.float64), mask=np.asarray(mask, dtype=np.float64), cfg=cfg, L=L, keep=(0, L))
    u["want"] = adjoint_f64(u["gy"], u["mask"], cfg, L)
    u["emu"] = emulate_adjoint_f32(u["gy"], u["mask"], cfg, L)
    u["bud"] = budget(u, emu=u["emu"])
    return u


# The backward matrix: one cell per route of sg_process_batch_backward / sg_process_rows_backward and per transform
# family behind stage_apply_ola.  ``route``: the kernels the cell's shape and options reach (row = k_row_backward, fast = k_apply_fast, reg = the
# register apply kernels, ola = stage_apply_ola, rows = rw_backward).  ``opts``: development options by
# name (SG_OPT_<name>); ``env``: set while the handle is created.  L in hops (+ a remainder that is no multiple of H, so
# the tail [Lq, L) exists); the rows cells hold five rows of their own lengths, NaN beyond them.  The four-step sizes
# (n_fft = 16384) are left out: one cell of them costs more than the rest of the matrix, and their backward is the same
# stage_apply_ola call as 4096's with another transform behind it, which the forward matrix (CELLS) holds.
def _b(name, route, n_fft, hops, rem, **kw):
    return dict(kw, name=name, route=route, n_fft=n_fft, hops=hops, rem=rem)


B_CELLS = [
    _b("row-T64", "row", 1024, 63, 13),
    _b("row-T9", "row", 1024, 8, 0),
    _b("fast-T65", "fast", 1024, 64, 13),
    _b("fast-norowgate", "fast", 1024, 63, 13, opts=(("FORCE_NOROWGATE", 1),), like="row-T64"),     # the same input
    _b("fast-ns", "fast", 1024, 70, 5, nonstationary=True, prop=0.7),
    _b("reg-512", "reg", 512, 70, 13),
    _b("reg-256", "reg", 256, 70, 13),
    _b("reg-2048", "reg", 2048, 70, 13),
    _b("reg-512-f64", "reg", 512, 70, 13, dtype="float64"),
    _b("lds-128", "ola", 128, 40, 7),
    _b("lds-4096", "ola", 4096, 40, 7),
    _b("lds-512-w400-h101", "ola", 512, 40, 7, W=400, H=101),
    _b("lds-1024-nofast", "ola", 1024, 64, 13, opts=(("FORCE_NOFAST", 1),)),
    _b("mixed-400", "ola", 400, 40, 7),
    _b("mixed-1000", "ola", 1000, 40, 7),
    _b("czt-601", "ola", 601, 40, 7),
    _b("czt-400", "ola", 400, 40, 7, env=(("SG_NO_MIXED_RADIX", "1"),)),
    _b("rows-256", "rows", 256, 60, 13, lengths=True),
    _b("rows-1024", "rows", 1024, 60, 13, lengths=True),
    _b("rows-4096", "rows", 4096, 60, 13, lengths=True),
    _b("rows-1024-ns", "rows", 1024, 60, 13, lengths=True, nonstationary=True),
]
B_ROWS_K = 37          # the rows cells' fourth and fifth row hold H k and H k + H - 1 samples


def b_cell_id(c):
    return c["name"]


def grad_field(Lq, H, seed, impulses=True):
    """The first grad_out of a row: tone + noise of amplitude ~1, the second half 60 dB down, impulses of amplitude 1
    on both sides of the first hop seam, at the last hop and the last sample, and one in the middle of the quiet half
    (``impulses=False``: without them -- tests/test_backward_parity_host.py)."""
    rng = np.random.default_rng(seed)
    g = 0.3 * rng.standard_normal(Lq) + 0.7 * np.sin(2 * np.pi * 1234.5 * np.arange(Lq) / T_SR)
    g[Lq // 2:] *= 1e-3
    for s in (0, 1, H - 1, H, Lq - H, Lq - 1, (3 * Lq) // 4) if impulses else ():
        g[s] += 1.0
    return g.astype(F32)


def grad_impulses(Lq):
    """The second grad_out: the two ends alone."""
    g = np.zeros(Lq, dtype=F32)
    g[0] = g[Lq - 1] = 1.0
    return g


B_LOUD = ((0.0, 0.08), (0.70, 0.78), (0.91, 1.0))


def b_signal(kind, n, seed, only=None):
    """A row of x: ``signals.two_level``'s content (kind 0: tone + noise) or ``signals.dc_nyquist``'s (kind 1) in two
    levels 30 dB apart, loud over ``B_LOUD`` (shares of the row) only.  TorchGate's stationary gate takes its threshold
    from the row itself, mean + 1.5 std of each band's dB over the frames: with a share f of the frames A dB above the
    rest that is A (f + 1.5 sqrt(f (1 - f))) above the quiet level, which the loud frames only exceed for f < 0.31.
    ``two_level`` as it stands (f = 0.5, its quiet half on the -40 dB floor) and ``dc_nyquist`` (one level) leave masks
    that pass next to nothing anywhere, and a gradient that is next to zero with them.  Here f = 0.25: the mask passes
    at the start of a row, inside the quiet half of the ``grad_field`` and at the row's end (so the tail [Lq, L) gets a
    gradient), and gates between.  ``only``: one of the three loud stretches alone -- a row of a few frames (2 W samples:
    9 frames, each 4 hops wide) is loud in every frame with all three."""
    y = signals._base(n, T_SR, seed) if kind == 0 else signals.dc_nyquist(n, T_SR, seed).astype(np.float64)
    env = np.full(n, _ROWS_QUIET)
    for a, b in (B_LOUD if only is None else B_LOUD[only:only + 1]):
        env[int(a * n):int(np.ceil(b * n))] = 1.0
    return (y * env).astype(F32)


@functools.lru_cache(maxsize=None)
def _b_case(i):
    c = B_CELLS[i]
    i = [d["name"] for d in B_CELLS].index(c.get("like", c["name"]))      # (seeds)
    n_fft = c["n_fft"]
    W = c.get("W", n_fft)
    H = c.get("H", W // 4)
    L = c["hops"] * H + c["rem"]
    kw = dict(n_fft=n_fft, nonstationary=bool(c.get("nonstationary", False)), prop_decrease=c.get("prop", 1.0))
    if "W" in c:
        kw.update(win_length=W, hop_length=H)
    if n_fft not in (1024, 512):
        kw.update(freq_mask_smooth_hz=3.02 * T_SR / (n_fft / 2), time_mask_smooth_ms=2.02 * H / T_SR * 1000)
    if c.get("lengths"):
        lens = [L, 2 * W, 2 * W + 1, H * B_ROWS_K, H * B_ROWS_K + H - 1]
    else:
        lens = [L] * 3
    x = np.full((len(lens), L), np.nan, dtype=F32)
    for b, n in enumerate(lens):
        x[b, :n] = b_signal(b % 2, n, 70 * i + b, only=b % 3 if n // H < 16 else None)
    cfg = dict(n_fft=n_fft, W=W, H=H, window=tile_window(W))
    gy1, gy2 = [], []
    for b, n in enumerate(lens):
        Lq = adjoint_geometry(cfg, n)[2]
        gy1.append(grad_field(Lq, H, 7000 + 70 * i + b))
        gy2.append(grad_impulses(Lq))
    return dict(cell=c, x=x, lens=lens, lengths=np.array(lens, dtype=np.int64) if c.get("lengths") else None, kw=kw,
                W=W, H=H, L=L, cfg=cfg, gy=(gy1, gy2), dtype=c.get("dtype", "float32"))


def b_case(i):
    """Inputs of a backward cell: ``x`` (B, L) float32-valued (NaN beyond a row's own samples), ``lens`` per row,
    ``lengths`` (rows cells; else None), ``kw`` for TorchGate / ``torchgate_units``, ``cfg`` for ``adjoint_f64``,
    ``gy = (first, second)``: per row a (Lq_row,) float32 grad_out (``grad_field``, ``grad_impulses``)."""
    return _b_case(i)


@functools.lru_cache(maxsize=4)
def _b_oracle(i):
    case = _b_case(i)
    return [torchgate_units(case["x"][b:b + 1, :n].astype(np.float64), T_SR, window=case["cfg"]["window"], **case["kw"])[1][0]
            for b, n in enumerate(case["lens"])]


def b_oracle(i):
    """The forward oracle's unit of every row of a backward cell (the row gated alone)."""
    return _b_oracle(i)


def adjoint_check_rows(tag, gx, gy, mask, cfg, lens):
    """A gradient (B, L) against ``adjoint_f64`` row by row: row b holds ``lens[b]`` samples, its grad_out is
    ``gy[b][:Lq_b]``, its mask ``mask[b, :T_b, :F]`` ((B, T, FS) as the engine saves it, natural bin order).  No hop
    block of ``[0, lens[b])`` may be over its float32 bound (``local_check``); returns the largest local_error / budget."""
    gx, mask = np.asarray(gx), np.asarray(mask)
    F = cfg["n_fft"] // 2 + 1
    worst = 0.0
    for b, n in enumerate(lens):
        p, T, Lq = adjoint_geometry(cfg, n)
        u = adjoint_unit(np.asarray(gy[b])[:Lq], mask[b, :T, :F].T, cfg, n)
        bad, ratio = local_check(gx[b, :n], u, bud=u["bud"])
        worst = max(worst, ratio)
        if len(bad):
            err = local_error(gx[b, :n], u["want"], cfg["H"])
            raise AssertionError("%s row %d: hop blocks %s of %d over their bound: error %s, budget %s, largest error / budget "
                                 "in the row %.2f" % (tag, b, bad[:10].tolist(), len(err), err[bad[:10]], u["bud"][bad[:10]],
                                                      ratio))
    return worst


# ----------------------------------------------------------------------------------------------------------------
# near-threshold cells: the exact re-evaluation of ambiguous decisions (tests/test_ambiguous_cells_host.py: conditions on
# the oracle and planted defects; tests/test_gpu_ambiguous_cells.py: the kernels)
# ----------------------------------------------------------------------------------------------------------------
# Every bulk decision kernel runs a float32 transform, flags a cell AMBIGUOUS when ||X| - T| <= delta with
# delta = 2^-16 ||x w||_2 (|X|, T in the unscaled transform's units), and has the whole wave re-evaluate each flagged cell
# as one float64 DFT sum of that bin.  On random input about one cell in 1e5 is flagged, at bands and frames nobody
# chose.  The inputs here are BUILT so that chosen cells sit inside delta / 2 of their thresholds, on both sides:
#
# * the threshold comes from a separate noise clip, so it stays put while the recording is moved (the row gate's cell:
#   from the row itself, re-derived in every iteration);
# * every band of every unit (channel, chunk) holds a target, every frame of a unit holds one -- frame 0 and the last
#   frame, which read zero padding or the neighbouring chunk's samples, included -- except the three frames on each
#   side of the unit's CROWDED frame; so every frame position modulo a decision kernel's frames per workgroup is hit
#   whatever that count is, as long as a unit holds three workgroups of the largest one a route of the cell launches
#   (tests/test_ambiguous_cells_host.py reads the counts from the kernels' headers and launches).  Where a size has more
#   frames than bands (n_fft = 64, 256) a frame whose neighbours leave no band free stays empty;
# * the crowded frame holds a target on every 4th band (every 8th where 4 n_fft / W > 4), bands 0, n_fft / 4 and
#   n_fft / 2 among them: one wave retires many cells, several per lane, the Nyquist flag with the rest;
# * two targets whose frames share a sample (within a unit or across a chunk seam) lie >= 4 n_fft / W bins apart, the
#   width of the Hann main lobe, so moving one barely moves the other;
# * goals: | |X| / T - 1 | log-uniform in [5e-8, 2e-6], random sign.  T ~ 2 ||x w|| on noise, so 2e-6 is ~0.25 delta;
#   the lower end is ~5 x the float32 rounding of the samples (2^-25 ||x w|| x 0.6 in |X|, ~1e-8 T) and 50 x 1e-7 dB.
#
# The solve is a Jacobi iteration in float64: every target's complex deficit X (want / |X| - 1) is cancelled by adding the
# windowed cosine and sine of its bin over the samples the frame really reads (a 2 x 2 real system per target: at a
# unit's edge the frame is cut short); all targets at once, until every | |X| / T - 1 - goal | <= 1e-12.  Then the samples
# are rounded to the cell's dtype, and what counts is the oracle's view of the ROUNDED samples.
#
# Chirp-z, four-step and the tile core (clips, rows, streams) decide in float64 and have no ambiguity path: no cell.
# Two cells run float64 decisions all the same and hold them to the same bits: n_fft = 8192 (no float32 decision kernel
# at that size) and TorchGate with xn= (four-kernel path).  k_row_gate, which re-evaluates whole bands, only runs on rows
# that take their threshold from themselves: its cell (rowgate-1024-own) re-derives the threshold from the row in every
# iteration.  That fixed point contracts only while a band holds few targets (each drags the six overlapping frames of
# its band along), so there bands 0, n_fft / 4 and n_fft / 2 are targeted in the crowded frame alone.
A_SEP = 4              # targets in sample-overlapping frames: >= A_SEP n_fft / W bins apart
A_GOAL = (5e-8, 2e-6)
A_TOL = 1e-12
_A_REG = ("default", "force_split", "force_nofast")


def _a(name, family, n_fft, frames, routes=("default",), **kw):
    return dict(kw, name=name, family=family, n_fft=n_fft, frames=frames, routes=routes)


# frames: hops per chunk (a unit holds 3 more frames); >= 3 workgroups of the size's decision kernels
A_CELLS = [
    _a("register-1024", "register", 1024, 48, _A_REG),
    _a("register-512", "register", 512, 96, _A_REG),
    _a("register-256", "register", 256, 192, _A_REG),
    _a("register-2048", "register", 2048, 48, _A_REG),
    _a("lds-64", "lds_pow2", 64, 192),
    _a("lds-4096", "lds_pow2", 4096, 32),
    _a("lds-8192", "lds_pow2", 8192, 32),
    _a("lds-1024-w600-h151", "lds_pow2", 1024, 48, W=600, H=151),
    _a("mixed-400", "mixed_radix", 400, 48),
    _a("mixed-4000", "mixed_radix", 4000, 32),
    _a("register-1024-f64", "register", 1024, 48, dtype="float64"),
    _a("register-1024-i16", "register", 1024, 48, dtype="int16"),
    _a("torchgate-1024-xn", "torchgate", 1024, 62, xn=True),
    _a("rowgate-1024-own", "torchgate", 1024, 62),
]
_A_RESEED = {}         # name -> seed offset (tests/test_ambiguous_cells_host.py holds the conditions a seed must meet)


def a_cell_id(c):
    return c["name"]


def a_cell(name):
    return next(c for c in A_CELLS if c["name"] == name)


def _a_window(cell, W):
    """The float64 analysis window over the frame a transform reads, and that frame's length."""
    if cell["family"] == "torchgate":
        return O._centered_window(cell["n_fft"], W, tile_window(W)), cell["n_fft"]
    return O.hann_periodic(W), W


def _a_frames(row, g0, v0, v1, T, n_frame, H):
    """(T, n_frame): frame t holds row[g0 + t H + m] where v0 <= index < v1, zeros elsewhere."""
    buf = np.zeros(n_frame + (T - 1) * H)
    a, b = max(v0, g0), min(v1, g0 + len(buf))
    buf[a - g0:b - g0] = row[a:b]
    return buf[np.arange(n_frame)[None, :] + H * np.arange(T)[:, None]]


def _a_stride(A, ov, sep):
    """A stride s so that bands less than sep apart land >= ov places apart in a list of A frames."""
    for s in range(ov + 1, A):
        if all(min((s * d) % A, A - (s * d) % A) >= ov for d in range(1, sep)):
            return s
    raise ValueError("no stride for %d frames" % A)


def _a_place(geo, F, n_fft, n_frame, H, sep, rng, extras=True):
    """Targets of every unit: ``[(bands, frames)]`` and the crowded frame of each unit."""
    ov = -(-n_frame // H)
    step = 4 * -(-sep // 4)
    placed = {}            # channel -> (first sample of the frame, band) of every target so far
    lists = [([], []) for _ in geo]
    crowded = [g["T"] // 2 for g in geo]

    def free(g, f, t):
        at = placed.setdefault(g["ch"], [[], []])
        s = np.asarray(at[0]) - (g["g0"] + t * H)
        near = (np.abs(s) < n_frame) & (np.abs(np.asarray(at[1]) - f) < sep)
        return not near.any()

    def put(ui, f, t):
        g = geo[ui]
        at = placed.setdefault(g["ch"], [[], []])
        lists[ui][0].append(f)
        lists[ui][1].append(t)
        at[0].append(g["g0"] + t * H)
        at[1].append(f)

    def fill(ui, t):
        f0 = int(rng.integers(1, F - 1))
        for f in ((f0 + k) % F for k in range(F)):
            if f % step and free(geo[ui], f, t):
                put(ui, f, t)
                return True
        return False

    # first, in every unit: the crowded frame; frame 0 and the last frame (they read padding or the neighbour chunk,
    # and across a seam they share samples with the neighbour's frames); bands 0, n_fft / 4 and n_fft / 2 once more in
    # every twelfth frame, so that the bins every kernel treats apart get enough targets for a share of them to mean
    # something
    for ui, g in enumerate(geo):
        for f in range(0, F, step):
            put(ui, f, crowded[ui])
    for ui, g in enumerate(geo):
        for t in (0, g["T"] - 1):
            if not fill(ui, t):
                raise ValueError("no band left for frame %d of unit %d" % (t, ui))
    for ui, g in enumerate(geo):
        T, tc = g["T"], crowded[ui]
        allowed = [t for t in range(T) if abs(t - tc) >= ov]
        for t in allowed[2::12] if extras else ():
            for f in (0, n_fft // 4, n_fft // 2):
                if free(g, f, t):
                    put(ui, f, t)
        s = _a_stride(len(allowed), ov, sep)
        n = 0
        for f in range(F):
            if f % step == 0:
                continue
            i0 = (s * n) % len(allowed)      # (a count, not f: f skips the crowded bands, and s f would skip frames)
            n += 1
            for k in range(len(allowed)):
                t = allowed[(i0 + k) % len(allowed)]
                if free(g, f, t):
                    put(ui, f, t)
                    break
            else:
                raise ValueError("no frame left for band %d" % f)
        # frames the bands left out (more frames than bands); a frame whose neighbours leave no band free stays empty
        # (tests/test_ambiguous_cells_host.py holds what must be hit)
        hit = set(lists[ui][1])
        for t in allowed:
            if t not in hit and fill(ui, t):
                hit.add(t)
    return [(np.array(tf), np.array(tt)) for tf, tt in lists], crowded


def _a_solve(y2, geo, targets, goals, wf, n_fft, n_frame, H, tlin, max_iter=400, relax=1.0):
    """The Jacobi iteration.  y2: (rows, N) float64, changed in place; ``tlin(Xs)``: per unit the (F,) threshold in the
    unscaled transform's units (given every unit's spectrum: the row gate's own-statistics cell re-derives it).
    Returns (iterations, largest | |X| / T - 1 - goal |)."""
    w2 = wf * wf
    pre = []
    for g, (tf, tt) in zip(geo, targets):
        valid = _a_frames(np.ones(y2.shape[1]), g["g0"], g["v0"], g["v1"], g["T"], n_frame, H)
        Q = np.fft.fft(valid * w2[None, :], n=n_fft, axis=-1)
        q = Q[tt, (2 * tf) % n_fft]
        E = Q[tt, 0].real
        pre.append(dict(valid=valid, Scc=0.5 * (E + q.real), Sss=0.5 * (E - q.real), Scs=-0.5 * q.imag,
                        edge=(tf == 0) | (2 * tf == n_fft)))
    err = np.inf
    for it in range(max_iter):
        Xs = [np.fft.rfft(_a_frames(y2[g["ch"]], g["g0"], g["v0"], g["v1"], g["T"], n_frame, H) * wf[None, :], n=n_fft, axis=-1)
              for g in geo]                                                          # (T, F) each
        tl = tlin(Xs)
        err, ups = 0.0, []
        for g, (tf, tt), goal, p, X, t_lin in zip(geo, targets, goals, pre, Xs, tl):
            x = X[tt, tf]
            want = t_lin[tf] * (1.0 + goal)
            err = max(err, float(np.max(np.abs(np.abs(x) / t_lin[tf] - 1.0 - goal))))
            d = relax * x * (want / np.abs(x) - 1.0)
            det = p["Scs"] ** 2 - p["Scc"] * p["Sss"]
            with np.errstate(divide="ignore", invalid="ignore"):
                a = np.where(p["edge"], d.real / p["Scc"], (-p["Sss"] * d.real - p["Scs"] * d.imag) / det)
                b = np.where(p["edge"], 0.0, (p["Scs"] * d.real + p["Scc"] * d.imag) / det)
            spec = np.zeros(X.shape, dtype=np.complex128)
            spec[tt, tf] = np.where(p["edge"], n_fft * a, 0.5 * n_fft * (a - 1j * b))
            ups.append(np.fft.irfft(spec, n=n_fft, axis=-1)[:, :n_frame] * wf[None, :] * p["valid"])
        if err <= A_TOL:
            return it, err
        for g, up in zip(geo, ups):
            row = y2[g["ch"]]
            for t in range(g["T"]):
                a0 = g["g0"] + t * H
                lo, hi = max(a0, 0), min(a0 + n_frame, len(row))
                row[lo:hi] += up[t, lo - a0:hi - a0]
    return max_iter, err


def unit_delta(unit):
    """(T,) float64: delta = 2^-16 ||x w||_2 of every frame, from the stored samples and the float64 window, in the
    unscaled transform's units."""
    c = unit["cfg"]
    if c["variant"] == "S":
        wf, n_frame = O.hann_periodic(c["W"]), c["W"]
    else:
        wf, n_frame = O._centered_window(c["n_fft"], c["W"], c["window"]), c["n_fft"]
    T = unit["raw"].shape[1]
    x = np.asarray(unit["x"], dtype=np.float64)
    fr = _a_frames(x, -(n_frame // 2), 0, len(x), T, n_frame, c["H"]) * wf[None, :]
    return 2.0 ** -16 * np.sqrt(np.sum(fr * fr, axis=1))


def unit_margin(unit):
    """(F, T) float64: (|X| - T) / delta of every cell (positive: the cell passes)."""
    c = unit["cfg"]
    s = float(np.sum(O.hann_periodic(c["W"]))) if c["variant"] == "S" else 1.0
    t_lin = (10.0 ** (unit["thresh"] / 20.0) - O.EPS64) * s
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.abs(unit["Z"]) * s - t_lin[:, None]) / unit_delta(unit)[None, :]


@functools.lru_cache(maxsize=None)
def _near_threshold_case(name):
    c = a_cell(name)
    n_fft = c["n_fft"]
    W = c.get("W", n_fft)
    H = c.get("H", W // 4)
    F = n_fft // 2 + 1
    dtype = c.get("dtype", "float32")
    rows = c["family"] == "torchgate"
    seed = 4100 + 37 * [d["name"] for d in A_CELLS].index(name) + _A_RESEED.get(name, 0)
    rng = np.random.default_rng(seed)
    wf, n_frame = _a_window(c, W)
    sep = -(-A_SEP * n_fft // W)
    level = 8000.0 if dtype == "int16" else 0.1
    if rows:
        sr, Cn, N = T_SR, 3, c["frames"] * H + 128
        kw = dict(n_fft=n_fft)
        geo = [dict(ch=b, chunk=0, g0=-(n_fft // 2), v0=0, v1=N, T=1 + N // H) for b in range(Cn)]
        noise = (level * rng.standard_normal((1, 30 * H))).astype(F32) if c.get("xn") else None
    else:
        sr, Cn = SR, 2
        cs, pad = c["frames"] * H + 5, H + 3
        N = 2 * cs - 7
        kw = dict(stationary=True, n_fft=n_fft, chunk_size=cs, padding=pad, prop_decrease=1.0)
        if "W" in c:
            kw.update(win_length=W, hop_length=H)
        if n_fft not in (1024, 512, 256, 2048) or "W" in c:
            kw.update(freq_mask_smooth_hz=3.02 * SR / (n_fft / 2), time_mask_smooth_ms=2.02 * H / SR * 1000)
        geo = [dict(ch=ci, chunk=k, g0=k * cs - pad - W // 2, v0=max(0, k * cs - pad), v1=min(N, (k + 1) * cs + pad),
                    T=(cs + 2 * pad + 2 * (W // 2) - W) // H + 1) for ci in range(Cn) for k in range(2)]
        noise = level * rng.standard_normal(max(24 * H, 2 * W))
        noise = np.clip(np.rint(noise), -32768, 32767).astype(np.int16) if dtype == "int16" else noise.astype(F32)
    y2 = level * rng.standard_normal((Cn, N))
    # (own statistics: a band's threshold moves with every cell of the band, and each target drags the six frames that
    # overlap it along; six more targets in one band make that map expanding, so bands 0, n_fft / 4 and n_fft / 2 keep to
    # the crowded frame there)
    targets, crowded = _a_place(geo, F, n_fft, n_frame, H, sep, rng, extras=not (rows and noise is None))
    goals = [rng.choice([-1.0, 1.0], len(tf)) * np.exp(rng.uniform(np.log(A_GOAL[0]), np.log(A_GOAL[1]), len(tf)))
             for tf, _ in targets]
    def cap_goals(t_lins):
        # a frame cut short at a unit's edge holds little of the window: delta shrinks with ||x w||, T does not, so the
        # goal there is capped at 0.4 delta (delta of the recording as drawn; the solve only adds to it)
        for g, (tf, tt), goal, t_lin in zip(geo, targets, goals, t_lins):
            fr = _a_frames(y2[g["ch"]], g["g0"], g["v0"], g["v1"], g["T"], n_frame, H) * wf[None, :]
            cap = 0.4 * 2.0 ** -16 * np.sqrt(np.sum(fr * fr, axis=1))[tt] / t_lin[tf]
            goal[:] = np.sign(goal) * np.minimum(np.abs(goal), np.maximum(cap, A_GOAL[0]))

    if rows and noise is None:
        def tlin(Xs):                           # the row's own mean + 1.5 std (ddof = 1) of its floored dB field
            out = []
            for X in Xs:
                db = O.amp_to_db(X.T, 40.0)
                out.append(10.0 ** ((np.mean(db, axis=-1) + 1.5 * np.std(db, axis=-1, ddof=1)) / 20.0) - O.EPS64)
            return out
    elif rows:
        db = O.amp_to_db(O.stft_torch(noise.astype(np.float64), n_fft, W, H, tile_window(W))[0], 40.0)
        fixed = 10.0 ** ((np.mean(db, axis=-1) + 1.5 * np.std(db, axis=-1, ddof=1)) / 20.0) - O.EPS64
        tlin = lambda Xs: [fixed] * len(Xs)     # noqa: E731
    else:
        th, _, _ = O.noise_threshold_S(noise.astype(np.float64)[None, :], n_fft, W, H, 1.5, kw["chunk_size"], True)
        fixed = (10.0 ** (th / 20.0) - O.EPS64) * float(np.sum(wf))
        tlin = lambda Xs: [fixed] * len(Xs)     # noqa: E731
    cap_goals(tlin([np.fft.rfft(_a_frames(y2[g["ch"]], g["g0"], g["v0"], g["v1"], g["T"], n_frame, H) * wf[None, :], n=n_fft,
                                axis=-1) for g in geo]))

    def stored(v):
        return np.clip(np.rint(v), -32768, 32767).astype(np.int16) if dtype == "int16" else v.astype(dtype)

    # (the own-statistics threshold moves with the row: quarter steps keep the fixed point from overshooting)
    relax = 0.25 if rows and noise is None else 1.0
    its, err = _a_solve(y2, geo, targets, goals, wf, n_fft, n_frame, H, tlin, relax=relax, max_iter=int(400 / relax))
    # rounding the samples moves |X| by ~1e-8 T (int16: by several delta), and now and then a target lands within
    # bit_diff's reach of its threshold: such a target's goal is moved outwards by half and the solve taken up again
    for _ in range(12):
        y = stored(y2)
        y64 = y.astype(np.float64)
        Xs = [np.fft.rfft(_a_frames(y64[g["ch"]], g["g0"], g["v0"], g["v1"], g["T"], n_frame, H) * wf[None, :], n=n_fft,
                          axis=-1) for g in geo]
        again = False
        for (tf, tt), goal, X, t_lin in zip(targets, goals, Xs, tlin(Xs)):
            close = np.abs(20.0 * np.log10(np.abs(X[tt, tf]) / t_lin[tf])) < 4e-7
            if dtype == "int16":
                close &= np.abs(goal) < 1.0      # (once: the cell then leaves delta / 2 and is no target)
                goal[close] = np.where(goal[close] > 0, 2.0, -0.5)
            else:
                goal[close] *= 1.5
            again |= bool(close.any())
        if not again:
            break
        its += _a_solve(y2, geo, targets, goals, wf, n_fft, n_frame, H, tlin, relax=relax)[0]
    # the oracle's view of the stored samples
    if rows:
        out, units = torchgate_units(y.astype(np.float64), sr, xn=None if noise is None else noise.astype(np.float64),
                                     window=tile_window(W), **kw)
    else:
        out, units = oracle_units(y.astype(np.float64), sr, y_noise=noise.astype(np.float64), **kw)
    assert [(u["ch"], u["chunk"]) for u in units] == [(g["ch"], g["chunk"]) for g in geo]
    margins = []
    for ui, u in enumerate(units):
        assert u["raw"].shape == (F, geo[ui]["T"]), (u["raw"].shape, F, geo[ui]["T"])
        tf, tt = targets[ui]
        m = unit_margin(u)[tf, tt]
        if dtype == "int16":     # rounding to integers moves |X| by several delta: the targets are those that stayed
            keep = np.abs(m) <= 0.5
            targets[ui], goals[ui], m = (tf[keep], tt[keep]), goals[ui][keep], m[keep]
        margins.append(m)
    return dict(cell=c, y=y, y_noise=noise, xn=noise if rows else None, kw=kw, dtype=dtype, precision=None, sr=sr, W=W, H=H,
                targets=targets, goals=goals, margins=margins, crowded=crowded, step=4 * -(-sep // 4), sep=sep,
                iterations=its, residual=err, out=out, units=units, geo=geo)


def near_threshold_case(cell):
    """A near-threshold cell: ``y`` (2, N) in the cell's dtype (row gate: ``y`` is x (3, L) float32), ``y_noise`` the
    noise clip the threshold comes from (``xn`` for the row gate; None: the row's own statistics), ``kw`` for
    reduce_noise / ``oracle_units`` (TorchGate / ``torchgate_units``), and the oracle's view of the STORED samples:
    ``out``, ``units``; per unit ``targets[ui] = (bands, frames)``, ``goals[ui]`` (|X| / T - 1 before rounding),
    ``margins[ui]`` ((|X| - T) / delta after rounding), ``crowded[ui]`` the crowded frame, ``geo[ui]['g0']`` the sample of the
    recording frame 0 starts at; ``iterations`` / ``residual``
    of the solve."""
    return _near_threshold_case(cell["name"])


# ----------------------------------------------------------------------------------------------------------------
# the -80 dB floor, band by band (tests/test_floor_host.py: conditions on the oracle and planted defects;
# tests/test_gpu_floor.py: the kernels)
# ----------------------------------------------------------------------------------------------------------------
# _amp_to_db floors a band's dB at (its maximum over the padded chunk) - 80.  In the gate a band whose maximum exceeds
# thresh[f] + 80 dB passes whole (a LIFTED band); in the noise statistics cells more than 80 dB under their band's maximum
# enter mean and std at the floor.  The inputs here engage both band by band, near the switch:
#
# gate (``floor_gate_case``): five units of 56 frames (chunk_size 37 H + 11, padding 9 H + 5, N = 4 chunk_size + 300) of
# white noise 10 dB under a white noise clip (all amplitudes below are set from the clip's thresholds, so every n_fft
# and window meets the same margins), plus
#   * a tone on bin n_fft / 8 over 6 hops in the middle of chunk 1 (no other unit's window holds it);
#   * an alternating-sign burst (band F - 1) in the LAST W samples of unit 0's padded window: unit 0's only lifting
#     frames lie wholly in its right padding; unit 1 holds the burst in its body;
#   * a constant level (band 0) over the FIRST W samples of unit 3's padded window -- a whole frame -- so unit 3's
#     only lifting frames lie wholly in its left padding; unit 2 holds it in its body;
#   * a tone on bin 63.5 in the middle of chunk 2 (bands 63 | 64, both sides of the 64-band seam; F > 66 only) and, where
#     the last 64-band block holds more than four bands, a tone in the middle of that block;
#   * unit 4 lifts nothing.  (``switch="dc"``: a second constant level early in chunk 2, see ``_f_build``.)
# The SWITCH band -- band n_fft / 8 + 3 of unit 1, or band 0 of unit 3 (``switch="dc"``) -- is placed at +g and at -g dB
# from its switch by bisecting its content's amplitude in float64 (g log-uniform in [1e-5, 1e-3]; int16: [3e-4, 1e-3],
# whole sample values move |X| by ~3e-5 dB); then the samples are rounded to the cell's dtype and the margins re-read.
#
# statistics (``floor_stats_case``): noise clips of 150 - 300 frames with zero runs of W + (m - 1) H samples aligned to
# the frames (exactly m zero-power frames in every band), a steady tone over the middle third above noise 80 dB down
# (floored cells in the tone's main-lobe bands only), and a plain clip.
F_GAIN = (1e-5, 1e-3)
F_GAIN_I16 = (3e-4, 1e-3)
F_OVER_DB = dict(tone=14.0, nyq=8.0, dc=8.0, seam=10.0, last=10.0)     # a content's peak band over its switch
_F_REG = ("default", "force_split", "force_nofast", "force_unfused", "floor_test_1", "floor_test_2")


def _f(name, family, n_fft, routes=("default",), **kw):
    return dict(kw, name=name, family=family, n_fft=n_fft, routes=routes)


F_CELLS = [
    _f("register-1024", "register", 1024, _F_REG, switch="dc"),
    _f("register-512", "register", 512, _F_REG),
    _f("register-256", "register", 256, _F_REG),
    _f("register-2048", "register", 2048, _F_REG),
    _f("lds-64", "lds_pow2", 64),
    _f("lds-4096", "lds_pow2", 4096),
    _f("lds-1024-w600-h151", "lds_pow2", 1024, W=600, H=151),
    _f("lds-8192", "lds_pow2", 8192),
    _f("mixed-400", "mixed_radix", 400),
    _f("czt-777", "chirp_z", 777),
    _f("register-1024-f64", "register", 1024, dtype="float64", precision="float64"),
    _f("register-1024-i16", "register", 1024, dtype="int16", sw_off=2),
    _f("register-1024-p07", "register", 1024, ("default", "force_split"), prop=0.7),
    _f("batch-1024", "clips", 1024, batch=True),
]
_F_RESEED = {"register-1024": 1}         # name -> seed offset (tests/test_floor_host.py holds the conditions a seed must meet)


def f_cell_id(c):
    return c["name"]


def f_cell(name):
    return next(c for c in F_CELLS if c["name"] == name)


def switch_margin(unit):
    """(F,) float64: m[f] = max_t dB - 80 - thresh[f] of a stationary unit (positive: the band is lifted)."""
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(np.abs(unit["Z"]) + O.EPS64)
    return db.max(axis=1) - 80.0 - unit["thresh"]


def _f_store(v, dtype):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16) if dtype == "int16" else np.asarray(v).astype(dtype)


def _f_geometry(c):
    n_fft = c["n_fft"]
    W = c.get("W", n_fft)
    H = c.get("H", W // 4)
    cs, pad = 37 * H + 11, 9 * H + 5
    return n_fft, W, H, cs, pad, 4 * cs + 300


def _f_kw(c):
    n_fft, W, H, cs, pad, N = _f_geometry(c)
    kw = dict(stationary=True, n_fft=n_fft, chunk_size=cs, padding=pad, prop_decrease=c.get("prop", 1.0))
    if "W" in c:
        kw.update(win_length=W, hop_length=H)
    if n_fft not in (1024, 512, 256, 2048) or "W" in c:
        kw.update(freq_mask_smooth_hz=3.02 * SR / (n_fft / 2), time_mask_smooth_ms=2.02 * H / SR * 1000)
    return kw


def _f_unit_window(y64, k, cs, pad):
    return O.read_chunk(y64[None, :], k * cs - pad, (k + 1) * cs + pad)[0]


def _f_build(c, sign):
    """One build of a gate cell: the switch band at sign x g."""
    n_fft, W, H, cs, pad, N = _f_geometry(c)
    F = n_fft // 2 + 1
    dtype = c.get("dtype", "float32")
    i16 = dtype == "int16"
    seed = 5200 + 41 * [d["name"] for d in F_CELLS].index(c["name"]) + _F_RESEED.get(c["name"], 0)
    rng = np.random.default_rng(seed)
    # the clip's level follows sqrt(W), so the thresholds -- and with them every amplitude below -- are those of W = 1024
    # at every size; int16: the base noise is 1 LSB RMS, the clip 3
    level = (1e5 if i16 else 1.0) * np.sqrt(W / 1024.0)
    base = level * 1e-5 * rng.standard_normal(N)
    noise = level * 3e-5 * rng.standard_normal(40 * H)
    sw_kind = c.get("switch", "tone")
    if sw_kind == "dc":
        # band 0 must hold the MINIMUM threshold: the clip loses its running mean over W / 4 samples
        noise = noise - np.convolve(noise, np.ones(W // 4) / (W // 4), mode="same")
    noise = _f_store(noise, dtype)
    kw = _f_kw(c)
    thresh, _, _ = O.noise_threshold_S(noise.astype(np.float64)[None, :], n_fft, W, H, 1.5, cs, True)
    sw_lin = 10.0 ** ((thresh + 80.0) / 20.0)         # |X| (oracle's scale) at which a band's floor reaches its threshold
    lo, hi = F_GAIN_I16 if i16 else F_GAIN
    g = float(np.exp(rng.uniform(np.log(lo), np.log(hi))))
    i = np.arange(N, dtype=np.float64)
    over = {k: 10.0 ** (v / 20.0) for k, v in F_OVER_DB.items()}
    kt = n_fft // 8
    parts = {}

    def span(a, b):
        e = np.zeros(N)
        e[a:b] = 1.0
        return e
    mid1 = cs + 15 * H
    parts["tone"] = (2.0 * sw_lin[kt] * over["tone"], span(mid1, mid1 + 6 * H) * np.sin(2 * np.pi * kt * (i - mid1) / n_fft))
    parts["nyq"] = (sw_lin[F - 1] * over["nyq"], span(cs + pad - W, cs + pad) * (1.0 - 2.0 * (i % 2)))
    parts["dc"] = (sw_lin[0] * over["dc"], span(3 * cs - pad, 3 * cs - pad + W))
    mid2 = 2 * cs + 14 * H
    if sw_kind == "dc":
        # unit 2 holds the switch burst in its body, 11 samples off unit 3's frame grid: its band 0 would sit next to the
        # switch too.  A second level early in chunk 2 (unit 1 sees it in its right padding, unit 3 not at all) lifts it
        parts["dc2"] = (sw_lin[0] * over["dc"], span(2 * cs + 2 * H, 2 * cs + 2 * H + W))
    if F > 66:
        parts["seam"] = (2.0 * sw_lin[63] * over["seam"], span(mid2, mid2 + 8 * H) * np.sin(2 * np.pi * 63.5 * (i - mid2) / n_fft))
    rem = (F - 1) % 64
    if rem >= 4:
        kl = F - 1 - rem // 2
        parts["last"] = (2.0 * sw_lin[kl] * over["last"],
                         span(mid2 + H, mid2 + 7 * H) * np.sin(2 * np.pi * kl * (i - mid2) / n_fft + 0.4))
    sw_part, sw_unit, sw_band = ("dc", 3, 0) if sw_kind == "dc" else ("tone", 1, kt + c.get("sw_off", 3))
    rest = base + sum(a * s for k, (a, s) in parts.items() if k != sw_part)
    shape = parts[sw_part][1]
    w = O.hann_periodic(W)

    def margin(A, stored=False):
        y = rest + A * shape
        if stored:
            y = _f_store(y, dtype).astype(np.float64)
        x = _f_unit_window(y, sw_unit, cs, pad)
        ext = np.concatenate([np.zeros(W // 2), x, np.zeros(W // 2)])
        T = (len(ext) - W) // H + 1
        fr = ext[np.arange(W)[None, :] + H * np.arange(T)[:, None]] * w[None, :]
        if sw_band == 0:
            mag = np.abs(fr.sum(axis=1))
        else:
            mag = np.abs(fr @ np.exp(-2j * np.pi * sw_band * np.arange(W) / n_fft))
        return 20.0 * np.log10(mag.max() / w.sum() + O.EPS64) - 80.0 - thresh[sw_band]

    goal = sign * g
    a_lo, a_hi = 0.0, (32000.0 if i16 else 0.95)
    assert margin(a_lo) < goal < margin(a_hi), (c["name"], margin(a_lo), margin(a_hi))
    for _ in range(200):
        a_mid = 0.5 * (a_lo + a_hi)
        if margin(a_mid) < goal:
            a_lo = a_mid
        else:
            a_hi = a_mid
        if a_hi - a_lo <= 1e-15 * a_hi:
            break
    A = 0.5 * (a_lo + a_hi)
    y = _f_store(rest + A * shape, dtype)
    return dict(y=y, y_plain=_f_store(base, dtype), y_noise=noise, kw=kw, dtype=dtype, precision=c.get("precision"), g=g, goal=goal, amplitude=A,
                switch=(sw_unit, sw_band), placed=margin(A), stored=margin(A, stored=True), seed=seed)


@functools.lru_cache(maxsize=None)
def _floor_gate_case(name, sign):
    c = f_cell(name)
    case = _f_build(c, sign)
    out, units = oracle_units(case["y"].astype(np.float64), SR, y_noise=case["y_noise"].astype(np.float64), **case["kw"])
    case.update(cell=c, out=out, units=units, margins=[switch_margin(u) for u in units])
    return case


def floor_gate_case(cell, sign=+1):
    """A floor cell's gate input, the switch band at ``sign`` x g: ``y`` (N,) and ``y_noise`` in the cell's dtype, ``kw``
    for reduce_noise / ``oracle_units``, the oracle's view of the STORED samples (``out``, ``units``) and per unit the
    switch margin ``margins[ui][f] = max_t dB - 80 - thresh[f]``; ``switch = (unit, band)``, ``g``, ``amplitude``,
    ``placed`` / ``stored``: the switch band's margin before / after rounding to the dtype; ``y_plain``: the same
    recording without the added content (no band lifts: ``floor_plain_oracle``)."""
    return _floor_gate_case(cell["name"], int(sign))


@functools.lru_cache(maxsize=4)
def _floor_plain_oracle(name):
    case = _floor_gate_case(name, 1)
    return oracle_units(case["y_plain"].astype(np.float64), SR, y_noise=case["y_noise"].astype(np.float64), **case["kw"])


def floor_plain_oracle(cell):
    """``(out, units)`` of the cell's recording without the added content."""
    return _floor_plain_oracle(cell["name"])


def floor_batch_case(cell):
    """``reduce_noise_batch``: three clips of different length over one shared noise clip -- the +g build (lifts bands),
    the start of its first chunk alone (cut before the burst: lifts nothing) and a stretch of the -g build from inside
    chunk 1 on (its chunk grid is another one: the tone and both bursts lie elsewhere in its units)."""
    a, b = floor_gate_case(cell, +1), floor_gate_case(cell, -1)
    n_fft, W, H, cs, pad, N = _f_geometry(cell)
    ys = [a["y"], a["y"][:cs - 2 * n_fft].copy(), b["y"][cs + 7:3 * cs - 2 * H].copy()]
    return dict(ys=ys, y_noise=a["y_noise"], kw=a["kw"], dtype=a["dtype"])


@functools.lru_cache(maxsize=2)
def _floor_batch_oracle(name):
    case = floor_batch_case(f_cell(name))
    yn = case["y_noise"].astype(np.float64)
    return [oracle_units(y.astype(np.float64), SR, y_noise=yn, **case["kw"])[1] for y in case["ys"]]


def floor_batch_oracle(cell):
    return _floor_batch_oracle(cell["name"])


# ---- statistics ----
S_CLIPS = [
    dict(name="runs-1024", n_fft=1024, frames=221, kind="runs"),
    dict(name="runs-256", n_fft=256, frames=263, kind="runs"),
    dict(name="tone-mid-1024", n_fft=1024, frames=190, kind="tone", bin=32.0),
    dict(name="tone-seam-1024", n_fft=1024, frames=190, kind="tone", bin=63.5),
    dict(name="tone-seam-256", n_fft=256, frames=290, kind="tone", bin=63.5),
    dict(name="plain-1024", n_fft=1024, frames=160, kind="plain"),
]


def s_clip_id(c):
    return c["name"]


def stats_slices(T, F, frames_per_slice, slices_max, maxs, tg):
    """The slice count of the single-pass statistics of one unit of T frames (api.hip: stat_slices and stage_stats),
    and the slice boundaries (kernels.hpp: k_colstats1)."""
    blocks = (F + 63) // 64
    nts = max(1, min(-(-2048 // blocks), slices_max, max(1, T // 16)))
    nts = max(1, min(nts, tg * maxs, T // frames_per_slice))
    return nts, [T * s // nts for s in range(nts + 1)]


@functools.lru_cache(maxsize=None)
def _floor_stats_case(name, nts):
    c = next(d for d in S_CLIPS if d["name"] == name)
    n_fft, T = c["n_fft"], c["frames"]
    W, H = n_fft, n_fft // 4
    N = (T - 1) * H + 3
    rng = np.random.default_rng(6100 + [d["name"] for d in S_CLIPS].index(name))
    y = 0.1 * rng.standard_normal(N)
    runs = []
    if c["kind"] == "runs":
        b = [T * s // nts for s in range(nts + 1)]
        assert nts >= 5, nts
        # (first frame, m): frame 0 alone (the pivot; slice 0 holds one floored frame), two inside slice 1, three inside
        # slice 2, a pair straddling the boundary of slices 3 | 4, five up to the last frame
        runs = [(0, 1), (b[1] + 9, 2), (b[2] + 11, 3), (b[4] - 1, 2), (T - 5, 5)]
        for t0, m in runs:
            y[max(0, t0 * H - W // 2):(t0 + m - 1) * H + W // 2] = 0.0
    elif c["kind"] == "tone":
        i = np.arange(N, dtype=np.float64)
        a, e = N // 3, (2 * N) // 3
        # noise 80 dB under the tone in the tone's band: |X| of white noise is ~1.1 sigma sqrt(0.375 W) / (0.5 W)
        y = 0.25e-4 * np.sqrt(W) / 1.3 * rng.standard_normal(N)
        # (switched on and off over 4 W samples each: a hard edge spreads the tone over every band of the edge frames)
        ramp = np.clip(np.minimum(i - a, e - i) / (4.0 * W), 0.0, 1.0)
        y += 0.5 * np.sin(0.5 * np.pi * ramp) ** 2 * np.sin(2 * np.pi * c["bin"] * i / n_fft)
    y = y.astype(F32)
    kw = dict(stationary=True, n_fft=n_fft, chunk_size=N + 1, padding=0, prop_decrease=1.0)
    return dict(clip=c, y_noise=y, runs=runs, kw=kw, T=T, W=W, H=H, nts=nts)


def floor_stats_case(clip, nts):
    """A statistics clip: ``y_noise`` (float32), ``runs`` [(first zero-power frame, m)], ``T`` frames; ``nts``: the slice
    count the engine uses for it (the zero runs are placed against its slice boundaries)."""
    return _floor_stats_case(clip["name"], int(nts))


def engine_stats_constants():
    """``(frames_per_slice, slices_max, maxs, tg)`` of the single-pass noise statistics, read from the sources
    (csrc/api.hip: SG_STAT_FRAMES_PER_SLICE, SG_STAT_SLICES_MAX and the expressions ``stats_slices`` restates;
    csrc/kernels.hpp: STAT1_MAXS, STAT_TG and k_colstats1's slice boundaries)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "noisereduce_amd", "csrc")
    with open(os.path.join(csrc, "api.hip")) as f:
        api = f.read()
    with open(os.path.join(csrc, "kernels.hpp")) as f:
        ker = f.read()

    def num(text, pattern):
        m = re.search(pattern, text)
        assert m, pattern
        return int(m.group(1))
    # the expressions restated in stats_slices
    assert "int64_t nts = (2048 + blocks - 1) / blocks;" in api
    assert "std::min<int64_t>(SG_STAT_SLICES_MAX, std::max<int64_t>(1, g.T / 16))" in api
    assert "std::min(stat_slices(g, ub), STAT_TG * STAT1_MAXS), g.T / SG_STAT_FRAMES_PER_SLICE)" in api
    assert "const int64_t tb = g.T * ts / nts, te = g.T * (ts + 1) / nts;" in ker
    return (num(api, r"#define SG_STAT_FRAMES_PER_SLICE (\d+)"), num(api, r"#define SG_STAT_SLICES_MAX (\d+)"),
            num(ker, r"constexpr int STAT1_MAXS = (\d+);"), num(ker, r"constexpr int STAT_TG = (\d+);"))


def stats_clip_slices(clip):
    """``(nts, boundaries)`` the engine uses for a statistics clip."""
    return stats_slices(clip["frames"], clip["n_fft"] // 2 + 1, *engine_stats_constants())


def amp_db_bits(unit, thresh):
    """The decision bits of a stationary unit under another threshold (F,)."""
    return O.amp_to_db(unit["Z"], 80.0) > np.asarray(thresh)[:, None]


# ----------------------------------------------------------------------------------------------------------------
# the route matrix of TorchGate.forward without lengths= (csrc/api.hip: sg_process_batch), shared by
# tests/test_torchgate_routes_host.py (conditions on the oracle, planted defects) and tests/test_gpu_torchgate_routes.py
# ----------------------------------------------------------------------------------------------------------------
# sg_process_batch picks its kernels from the rows of a unit batch (below 16 / from 16 on), the frames of a row (up to
# 64 with 160 rows: the row gate; up to 128: k_row_decide; beyond: k_t2_rows + k_decide_bits_t2), where the thresholds
# come from (the rows, one noise row, one noise row per row) and the number of unit batches the workspace budget allows.
# T_CELLS above never varies any of them.  Every row of an R cell differs from every other row in level, colour, tone and
# (some) in floor and DC / Nyquist content, so that a threshold, band maximum or mask taken from another row or another
# batch changes hundreds of decisions (tests/test_torchgate_routes_host.py holds that).
#
# ``batches``: the rows per unit batch the cell means to run in; a cell with more than one gets a workspace budget
# (``r_budget``) and the GPU test asserts the split from what the handle reports, not from the budget.
# ``route``: what decides -- row_gate (k_row_gate), row_decide (k_row_decide: statistics + constants + bits of a tile),
# t2 (k_t2_rows + k_decide_bits_t2), float (k_decide, float raw mask + float smoothing), box (k_box_mask), ns_raw
# (k_boxcar_sigmoid + the general smoothing kernels).  ``apply``: fast (k_apply_fast), reg (a register geometry's apply
# kernel), ola (k_apply_istft + k_ola).  ``xn``: None, "one" (one noise row: ustride = 0), "rows" (a noise row per row:
# ustride = FS, vn.unit0 = u0 per batch), ``xnT`` its frames.
# (nt96 / wide-nt: 241 frames, not 240 -- 4 rows of 240 frames get 15 statistics slices, and 240 is a multiple of 15.
# nt96 is wide-nt's other side: the widest time smoothing that stays on the bit-mask path.  Both switch the frequency
# smoothing off: with the default 500 Hz, (nf + 1)^2 (nt + 1)^2 exceeds 65535 and the path is left through ktot instead.)
R_SR = 16000
_NT97_MS = 97.02 * 256 / R_SR * 1000       # time_mask_smooth_ms of n_grad_time = 97 at hop 256
_NT96_MS = 96.02 * 256 / R_SR * 1000


def _r(name, n_fft, B, T, route, apply="fast", xn=None, xnT=None, batches=None, kw=None, **more):
    return dict(name=name, n_fft=n_fft, B=B, T=T, route=route, apply=apply, xn=xn, xnT=xnT,
                batches=list(batches) if batches else [B], kw=dict(kw or {}), **more)


R_CELLS = [
    _r("t128", 1024, 5, 128, "row_decide"),
    _r("t129", 1024, 5, 129, "t2"),
    _r("b15", 1024, 15, 150, "t2"),
    _r("b16", 1024, 16, 150, "t2"),
    _r("b16-nofast", 1024, 16, 150, "float", apply="ola", nofast=True),
    _r("xnB-15", 1024, 15, 100, "row_decide", xn="rows", xnT=41),
    _r("xnB-16", 1024, 16, 100, "row_decide", xn="rows", xnT=41),
    _r("xnB-long", 1024, 17, 200, "t2", xn="rows", xnT=260),
    _r("xn1-long", 1024, 6, 200, "t2", xn="one", xnT=260),
    _r("split", 1024, 37, 129, "t2", batches=(16, 16, 5)),
    _r("split-xnB", 1024, 37, 100, "row_decide", xn="rows", xnT=41, batches=(16, 16, 5)),
    _r("split-rowgate", 1024, 200, 64, "row_gate", batches=(80, 80, 40)),
    _r("rg-64", 1024, 160, 64, "row_gate"),
    _r("rg-65", 1024, 160, 65, "row_decide"),
    _r("rg-159", 1024, 159, 64, "row_decide"),
    _r("prop07", 1024, 16, 150, "float", kw=dict(prop_decrease=0.7)),
    _r("nt96", 1024, 4, 241, "t2", kw=dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=_NT96_MS)),
    _r("wide-nt", 1024, 4, 241, "float", kw=dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=_NT97_MS)),
    _r("n512", 512, 16, 150, "float", apply="reg"),
    _r("n2048", 2048, 16, 150, "float", apply="reg",
       kw=dict(freq_mask_smooth_hz=3.02 * R_SR / 1024, time_mask_smooth_ms=2.02 * 512 / R_SR * 1000)),
    _r("n512-win", 512, 5, 150, "float", apply="ola", xn="one", xnT=77, kw=dict(win_length=400, hop_length=101)),
    _r("n400", 400, 17, 140, "float", apply="ola", xn="rows", xnT=61,
       kw=dict(freq_mask_smooth_hz=3.02 * R_SR / 200, time_mask_smooth_ms=2.02 * 100 / R_SR * 1000)),
    _r("f64", 1024, 16, 129, "t2", dtype="float64"),
    _r("ns-box", 1024, 20, 150, "box", batches=(8, 8, 4), kw=dict(nonstationary=True)),
    _r("ns-raw", 1024, 20, 150, "ns_raw", batches=(8, 8, 4),
       kw=dict(nonstationary=True, n_movemean_nonstationary=7)),
]
R_FLOOR_EVERY = 4            # rows b with b % 4 == 3: second half 60 dB down, plus a steady hum that keeps its bands unlifted
R_DCNY_ROWS = (1, 2)         # rows with DC + Nyquist content (signals.dc_nyquist's)
_R_RESEED = {}               # name -> seed offset (tests/test_torchgate_routes_host.py holds the conditions a seed must meet)


def r_cell_id(c):
    return c["name"]


def r_cell(name):
    return next(c for c in R_CELLS if c["name"] == name)


def r_geometry(c):
    """(n_fft, W, H) of a route cell."""
    return O.resolve_stft_params(c["n_fft"], c["kw"].get("win_length"), c["kw"].get("hop_length"))


def _one_pole(rng, n, pole):
    """Unit-variance noise through y[i] = pole y[i - 1] + w[i]."""
    import scipy.signal
    w = rng.standard_normal(n + 64)
    return scipy.signal.lfilter([1.0], [1.0, -pole], w)[64:] * np.sqrt(1.0 - pole * pole)


def r_row_pole(b):
    """Row b's colour: low-pass and high-pass alternate, the pole's size walks over 17 values."""
    return (1.0 if b % 2 == 0 else -1.0) * (0.1 + 0.8 * ((5 * b) % 17) / 17.0)


def r_row_level(b):
    """Row b's level: 3 dB steps over 24 dB."""
    return 10.0 ** (-3.0 * (b % 9) / 20.0)


def route_rows(B, L, seed, sr=R_SR):
    """(B, L) float32: row b = 0.1 x level_b x one-pole noise (pole_b) + a 0.5 x level_b tone of its own frequency that is
    on for 30 % of the row from a row-dependent sample on.  Rows b % 4 == 3: everything after L / 2 scaled by 1e-3, plus a
    steady 0.05 x level_b hum at a quarter of the sampling rate (its bands stay within 40 dB of their maximum, every other
    band of the row is lifted by the floor).  Rows 1 and 2: + 0.01 DC + 0.02 (-1)^n, scaled by the row's level."""
    i = np.arange(L, dtype=np.float64)
    x = np.empty((B, L), dtype=F32)
    for b in range(B):
        rng = np.random.default_rng(seed + 101 * b)
        lev = r_row_level(b)
        hz = sr * (0.05 + 0.4 * ((7 * b + 3) % 31) / 31.0) + 3.7 * b
        on = int(L * (0.15 + 0.5 * ((3 * b) % 11) / 11.0))
        y = 0.1 * _one_pole(rng, L, r_row_pole(b))
        y[on:on + (3 * L) // 10] += 0.5 * np.sin(2 * np.pi * hz * i[on:on + (3 * L) // 10] / sr)
        y *= lev
        if b % R_FLOOR_EVERY == R_FLOOR_EVERY - 1:
            y[L // 2:] *= 1e-3
            y += 0.05 * lev * np.sin(2 * np.pi * (0.25 * sr + 7.3) * i / sr)
        if b in R_DCNY_ROWS:
            y += lev * (0.01 + 0.02 * (1.0 - 2.0 * (np.arange(L) % 2)))
        x[b] = y.astype(F32)
    return x


def route_noise(Bn, Ln, seed):
    """(Bn, Ln) float32 noise rows, no tone.  Bn > 1: row b coloured and levelled like row b of ``route_rows``, 6 dB under
    its noise.  Bn == 1: nearly white (pole 0.1) at -14 dB of row 0's noise, the middle of the rows' 24 dB of levels, so
    that the loudest row is not all-pass and the quietest not all-gated."""
    xn = np.empty((Bn, Ln), dtype=F32)
    for b in range(Bn):
        rng = np.random.default_rng(seed + 7919 + 101 * b)
        if Bn == 1:
            xn[b] = (0.1 * 10.0 ** (-14.0 / 20.0) * _one_pole(rng, Ln, 0.1)).astype(F32)
        else:
            xn[b] = (0.05 * r_row_level(b) * _one_pole(rng, Ln, r_row_pole(b))).astype(F32)
    return xn


@functools.lru_cache(maxsize=None)
def _r_case(name):
    c = r_cell(name)
    n_fft, W, H = r_geometry(c)
    L = (c["T"] - 1) * H + 13
    seed = 4000 + 37 * [d["name"] for d in R_CELLS].index(name) + _R_RESEED.get(name, 0)
    x = route_rows(c["B"], L, seed)
    xn = None
    if c["xn"]:
        xn = route_noise(c["B"] if c["xn"] == "rows" else 1, (c["xnT"] - 1) * H + 13, seed)
    kw = dict(c["kw"], n_fft=n_fft)
    return dict(cell=c, x=x, xn=xn, kw=kw, L=L, W=W, H=H, dtype=c.get("dtype", "float32"),
                stationary=not kw.get("nonstationary", False))


def r_case(c):
    """Inputs of a route cell: ``x`` (B, L) and ``xn`` (None, (1, Ln) or (B, Ln)), float32-valued; ``kw`` for TorchGate /
    ``torchgate_units`` (sr = R_SR); ``dtype`` what the call is given."""
    return _r_case(c["name"])


@functools.lru_cache(maxsize=3)
def _r_oracle(name):
    case = _r_case(name)
    xn = None if case["xn"] is None else case["xn"].astype(np.float64)
    return torchgate_units(case["x"].astype(np.float64), R_SR, xn=xn, window=tile_window(case["W"]), **case["kw"])[1]


def r_oracle(c):
    """The oracle's units of a route cell, one per row."""
    return _r_oracle(c["name"])


def r_unit_bytes(n_fft, T):
    """Workspace bytes of one unit of T frames as csrc/api.hip's ``unit_bytes`` (not lean) has them; the expressions are
    checked against the source."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "noisereduce_amd", "csrc")
    with open(os.path.join(csrc, "api.hip")) as f:
        api = f.read()
    with open(os.path.join(csrc, "nonstat_mask.hpp")) as f:
        ns = f.read()
    assert "return cells * (8 + 4 + 4 + 2) + (size_t)g.T * g.n * 4 + (size_t)g.FS * 16 +" in api
    assert "(size_t)(g.T / NS_TT + 1) * 2 * g.FS * 8 * 2 +" in api
    assert "(size_t)(g.T / 8 + 1) * 2 * g.FS * 8;" in api
    assert "int64_t ub = ws_budget(h) / (int64_t)unit_bytes(h, g, lean);" in api
    assert "constexpr int NS_TT = 64;" in ns
    FS = (n_fft // 2 + 1 + 15) // 16 * 16
    cells = T * FS
    return cells * 18 + T * n_fft * 4 + FS * 16 + (T // 64 + 1) * 2 * FS * 8 * 2 + (T // 8 + 1) * 2 * FS * 8


def r_budget(c):
    """``max_workspace_bytes`` for the cell's split (0: the default budget, one batch): room for batches[0] units of the
    larger of the two geometries (rows, noise rows) and half a unit more."""
    if len(c["batches"]) == 1:
        return 0
    per = r_unit_bytes(c["n_fft"], max(c["T"], c["xnT"] or 0))
    return per * c["batches"][0] + per // 2


def r_stat_slices(c, T, nb, single_pass):
    """Slice count of the column statistics over a batch of nb units of T frames (api.hip: stat_slices; stage_stats for
    the single-pass kernels), re-derived from the sources as ``engine_stats_constants`` does."""
    fps, smax, maxs, tg = engine_stats_constants()
    blocks = ((c["n_fft"] // 2 + 1 + 63) // 64) * nb
    nts = max(1, min(-(-2048 // blocks), smax, max(1, T // 16)))
    if single_pass:
        nts = max(1, min(nts, tg * maxs, T // fps))
    return nts


def r_stats_launches(c):
    """[(what, T, nb, single_pass)] of a stationary cell: every launch of the column statistics / column maxima that slices
    the frames (sg_process_batch: stage_stats on the noise, stage_power's k_colmax below 16 rows and stage_colstats on
    the rows where k_row_decide and k_row_gate do not take them)."""
    out = []
    if c["xn"] == "one":
        out.append(("noise", c["xnT"], 1, True))
    for nb in c["batches"]:
        if c["xn"] == "rows":
            out.append(("noise", c["xnT"], nb, nb < 16))
        if c["route"] in ("t2", "float"):
            out.append(("rows", c["T"], nb, False))
    return out


def torchgate_gate_kwargs(tg, **extra):
    """Keyword arguments of ``_ffi.Gate`` for the handle a TorchGate module creates (torchgate.py: _gate_for), for tests
    that need a handle of their own (a workspace budget)."""
    import torch
    from noisereduce_amd import _ffi
    nf, nt = tg._n_grad
    kw = dict(variant=_ffi.SG_VARIANT_T, stationary=not tg.nonstationary, n_fft=tg.n_fft, win_length=tg.win_length,
              hop_length=tg.hop_length, n_grad_freq=nf, n_grad_time=nt, smooth_mask=tg.smoothing_filter is not None,
              prop_decrease=tg.prop_decrease, n_std_thresh=tg.n_std_thresh_stationary, top_db=40.0, ddof=1,
              n_movemean=tg.n_movemean_nonstationary, nonstat_thresh=tg.n_thresh_nonstationary,
              nonstat_slope=1.0 / tg.temp_coeff_nonstationary, window=torch.hann_window(tg.win_length).double().numpy())
    kw.update(extra)
    return kw


# ----------------------------------------------------------------------------------------------------------------
# the width matrix: mask smoothing half-widths (n_grad_freq, n_grad_time) on both sides of every edge the engine routes
# on, shared by tests/test_smoothing_widths_host.py (conditions on the oracle, the routing restated) and
# tests/test_gpu_smoothing_widths.py
# ----------------------------------------------------------------------------------------------------------------
# A cell: gate ("S": stationary, "NS": non-stationary, both variant S), n_fft (window = n_fft, hop = n_fft / 4 --
# resolve_stft_params), the half-widths, the routes it runs, and
#   none=True          a half-width of 1 is spelled None (the reference's other spelling of it), else 1.02 bins / frames
#   small=True         a single unpadded unit of 34 frames: the field is smaller than the filter on both axes
#   tc=...             time_constant_s (non-stationary)
#   precision="float64"
# Shapes: a unit holds 2 nt + 70 frames -- two edge tiles and an interior 64-frame tile of every smoothing kernel, whose
# tiles are at most 64 frames wherever the filter is wide -- in two chunks with under one hop of padding, so that the
# first and the last frame of a unit reach kept samples; one channel.
W_LDS_CAP = 150 * 1024                 # the dynamic LDS every smoothing launch may ask for (api.hip)
_W_REG = ("default", "force_split", "force_nofast")
_W_CORNER = _W_REG + ("force_unfused",)


def _w(gate, n_fft, nf, nt, routes=("default",), **kw):
    name = "%s-%d-f%d-t%d" % (gate, n_fft, nf, nt) + "".join("-%s" % k if v is True else "-%s%s" % (k, v)
                                                            for k, v in sorted(kw.items()) if k != "precision")
    if kw.get("precision") == "float64":
        name += "-f64"
    if routes == ("force_unfused",):
        name += "-unfused"
    return dict(name=name, gate=gate, n_fft=n_fft, nf=nf, nt=nt, routes=tuple(routes), **kw)


# ---- byte counts, from the constants of the headers ----
def sm2_pitch(F):
    """fused.hpp smooth2_pitch: LDS row pitch of k_smooth_bits2's phase-1 counts."""
    return ((F + 3) & ~3) + 4 * ((F + 31) // 32) + 4


def sm2_tile(F, nf, nt, tt_max=None):
    """api.hip fit_sm2_tile: the tile height (frames) k_smooth_bits2 settles on, or None when no tile of >= 16 frames fits:
    (tt + 2 nt + 2) rows of counts (1 byte while (nf + 1)^2 <= 255, else 2) + (tt + 2 nt) bit rows of ceil(F / 64) + 2
    words + the 8 KiB lookup table <= 150 KiB; tt from smooth2_tt_max(F) = 256 / 128 / 64 (F <= 160 / <= 320 / above) down
    by halves."""
    ct = 1 if (nf + 1) ** 2 <= 255 else 2
    wpr = (F + 63) // 64
    tt = (256 if F <= 160 else 128 if F <= 320 else 64) if tt_max is None else tt_max
    while tt >= 16:
        rows = tt + 2 * nt
        cf = ((rows + 2) * sm2_pitch(F) * ct + 15) & ~15
        if cf + rows * (wpr + 2) * 8 + 8192 <= W_LDS_CAP:
            return tt
        tt >>= 1
    return None


def smf_lds_bytes(nf, nt):
    """api.hip stage_smooth: k_smooth_tiled's tile, SMF_TT = SMF_FB = 64, SMF_KT = 192."""
    rows, cols = 64 + 2 * nt, 64 + 2 * nf
    return ((rows + 3) * (cols | 1) + (rows + 3) * 65 + 8 + 64 + 192 + 64 + 64) * 4


def smooth_tiled_ok(nf, nt):
    return smf_lds_bytes(nf, nt) <= W_LDS_CAP and nf <= 30 and 2 * nt + 4 <= 192 and 64 + 2 * nf <= 192


def xsm_lds_bytes(nf, nt):
    """exact.hpp xsm_lds_bytes: kx_smooth_tiled's tile, XSM_TT = 32, XSM_FB = 64, XSM_KMAX = 192."""
    rows, cols = 32 + 2 * nt + 3, 64 + 2 * nf + 3
    return (rows * (cols | 1) + rows * 65 + 2 * 192 + 64 + 32) * 8


def x_tiled_ok(nf, nt):
    return xsm_lds_bytes(nf, nt) <= W_LDS_CAP and 2 * nf < 192 and 2 * nt < 192


def _last_nt(ok):
    """The largest nt >= 1 with ok(nt) (ok is monotone)."""
    nt = 1
    while ok(nt + 1):
        nt += 1
    return nt


def _mixed_radix(n_fft):
    m = n_fft // 2
    for p in (2, 3, 5, 7, 11, 13):
        while m % p == 0:
            m //= p
    return n_fft % 2 == 0 and n_fft >= 8 and m == 1


# one-pass gates: (max nf, max nt, frames per tile) -- api.hip OP1024 / REG512 / REG256 / REG2048 (abutting tiles)
W_ONEPASS = {1024: (8, 16, 16), 512: (8, 24, 32), 256: (8, 40, 64), 2048: (24, 8, 8)}
NS_IIR_NT = tuple(range(1, 21)) + (25, 34, 37)          # nonstat_mask.hpp: instantiated k_iir_mask<nt>
NS_MAX_NF = 24


def w_geometry(c):
    return O.resolve_stft_params(c["n_fft"], None, None)


def w_smooth(c):
    """Whether the reference smooths at all: (1, 1) switches the filter off (base.py:111)."""
    return not (c["nf"] == 1 and c["nt"] == 1)


def w_iir_b(c):
    n_fft, W, H = w_geometry(c)
    return float(O.iir_coefficient(c.get("tc", 2.0), SR, H))


def w_route(c, route):
    """The routing predicates of csrc/api.hip restated: ``(smoothing kernel, bytes of its cell, frames per tile)`` as
    ``Gate.smooth_route()`` reports it after the cell ran ``route``."""
    n_fft, W, H = w_geometry(c)
    F = n_fft // 2 + 1
    nf, nt, smooth = c["nf"], c["nt"], w_smooth(c)
    general = ("off", 4, 0) if not smooth else ("k_smooth_tiled", 4, 64) if smooth_tiled_ok(nf, nt) else \
        ("k_smooth_f+k_smooth_t", 4, 0)
    if c.get("precision") == "float64":
        # the n_fft = 1024 stationary gate keeps the bit-mask stages and applies in float64 (exact_fused_ok); everything
        # else is run_S_exact
        if not (c["gate"] == "S" and n_fft == 1024 and w_fused_ok(c)):
            return ("off", 8, 0) if not smooth else ("kx_smooth_tiled", 8, 32) if x_tiled_ok(nf, nt) else \
                ("kx_smooth_f+kx_smooth_t", 8, 0)
        return ("k_smooth_bits2", 1 if (nf + 1) ** 2 <= 255 else 2, sm2_tile(F, nf, nt)) if smooth else ("off", 2, 0)
    if c["gate"] == "NS":
        b = w_iir_b(c)
        chain = route != "force_unfused" and 0.0 < b < 1.0 and (1.0 - b) ** (64 + 2 * 20) >= 1e-3
        one = chain and smooth and (nt <= 20 or (1.0 - b) ** (64 + 2 * nt) >= 1e-3) and nf <= NS_MAX_NF and nt in NS_IIR_NT
        return ("k_iir_mask<nt>", 4, 64) if one else general
    if route == "force_unfused" or not w_fused_ok(c):
        return general
    if route == "default" and smooth and n_fft in W_ONEPASS:
        mf, mt, frames = W_ONEPASS[n_fft]
        if nf <= mf and nt <= mt:
            return ("k_gate_onepass" if n_fft == 1024 else "k_gate_onepass_reg", 1, frames)
    if not smooth:
        return ("off", 2, 0)
    return ("k_smooth_bits2", 1 if (nf + 1) ** 2 <= 255 else 2, sm2_tile(F, nf, nt))


def w_fused_ok(c):
    """api.hip fused_ok: the bit-mask path of the stationary gate -- integer sums in uint16, a power of two or a
    mixed-radix size up to 4096, nt <= 96, nf <= 30, and a tile of k_smooth_bits2 that fits."""
    n_fft, W, H = w_geometry(c)
    nf, nt, smooth = c["nf"], c["nt"], w_smooth(c)
    ktot = (nf + 1) ** 2 * (nt + 1) ** 2 if smooth else 1
    pow2 = n_fft & (n_fft - 1) == 0
    if not (ktot <= 65535 and (pow2 or _mixed_radix(n_fft)) and n_fft <= 4096):
        return False
    return not smooth or (nt <= 96 and nf <= 30 and sm2_tile(n_fft // 2 + 1, nf, nt) is not None)


def _w_cells():
    S, NS = "S", "NS"
    cells = []
    # ---- stationary, register geometries ----
    cells += [_w(S, 1024, 1, 1, _W_CORNER, none=True),                 # no smoothing at all
              _w(S, 1024, 1, 1, _W_REG),                               # ... spelled as numbers
              _w(S, 1024, 1, 2, _W_REG, none=True), _w(S, 1024, 2, 1, _W_REG),
              _w(S, 1024, 8, 8, _W_REG), _w(S, 1024, 8, 9, _W_REG),   # 2 nt > 16: the third row block (onepass.hpp)
              _w(S, 1024, 8, 16, _W_CORNER), _w(S, 1024, 8, 17, _W_REG), _w(S, 1024, 9, 16, _W_REG)]
    cells += [_w(S, 512, 8, 24, _W_CORNER), _w(S, 512, 8, 25, _W_REG), _w(S, 512, 9, 24, _W_REG),
              # the operand table holds the time weights wt(32 b + row - nt - j) of k-block b = 0, 1 for the 16 output
              # frames j of a product: 16 + 2 nt = 32 rows fill block 0 exactly at nt = 8, nt = 9 is the first to have
              # non-zero weights in block 1 (and nt = 24 the last whose 64 rows fit both)
              _w(S, 512, 3, 8, _W_REG), _w(S, 512, 3, 9, _W_REG)]
    cells += [_w(S, 256, 8, 24, _W_REG), _w(S, 256, 8, 25, _W_REG),   # 2 nt > 48: the third k-block (onepass256.hpp)
              _w(S, 256, 8, 27, _W_REG), _w(S, 256, 8, 28, _W_REG),   # ktot 63504 | 68121
              _w(S, 256, 5, 40, _W_CORNER), _w(S, 256, 5, 41, _W_REG),   # ktot 60516 | 63504, past the gate's 40
              _w(S, 256, 6, 40, _W_REG)]                                 # ktot 82369
    cells += [_w(S, 2048, 8, 8, _W_REG), _w(S, 2048, 16, 8, _W_REG), _w(S, 2048, 24, 8, _W_CORNER),
              _w(S, 2048, 25, 8, _W_REG), _w(S, 2048, 24, 9, _W_REG)]
    # ---- stationary, general bit-mask path ----
    for n_fft in (128, 400, 4096):
        cells += [_w(S, n_fft, 5, 2), _w(S, n_fft, 6, 2),             # the 18-bit lookup table: 8 + 2 nf <= 18
                  _w(S, n_fft, 14, 3), _w(S, n_fft, 15, 3),           # (nf + 1)^2 <= 255: uint8 | uint16 cells
                  _w(S, n_fft, 30, 6), _w(S, n_fft, 31, 6),           # nf <= 30
                  _w(S, n_fft, 14, 16), _w(S, n_fft, 15, 15),         # ktot 65025 | 65536
                  _w(S, n_fft, 1, 96, none=True), _w(S, n_fft, 1, 97)]
    # n_fft = 4096 (F = 2049, tiles from 64 frames down): the last nt of every tile height sm2_tile settles on at nf = 2,
    # and the first nt no tile fits
    seen = set()
    for nt in range(1, 97):
        tt = sm2_tile(2049, 2, nt)
        if tt not in seen and tt is not None:
            seen.add(tt)
            cells.append(_w(S, 4096, 2, _last_nt(lambda t, tt=tt: sm2_tile(2049, 2, t) == tt or
                                                 (sm2_tile(2049, 2, t) or 0) > tt)))
    cells.append(_w(S, 4096, 2, _last_nt(lambda t: sm2_tile(2049, 2, t) is not None) + 1))
    cells.append(_w(S, 64, 30, 30, small=True))
    # ---- materialised float kernels: the chirp-z size 601, and SG_OPT_FORCE_UNFUSED at 1024 ----
    nt30 = _last_nt(lambda t: smooth_tiled_ok(30, t))       # smf_lds_bytes(30, nt) <= 150 KiB
    for n_fft, routes in ((601, ("default",)), (1024, ("force_unfused",))):
        cells += [_w(S, n_fft, 30, nt30, routes), _w(S, n_fft, 30, nt30 + 1, routes),
                  _w(S, n_fft, 2, 94, routes), _w(S, n_fft, 2, 95, routes),       # 2 nt + 4 <= SMF_KT = 192
                  _w(S, n_fft, 31, 4, routes)]
    # ---- non-stationary ----
    for n_fft in (1024, 400):
        cells += [_w(NS, n_fft, 2, nt) for nt in (20, 21, 24, 25, 26, 34, 37, 38)]
        cells += [_w(NS, n_fft, 24, 9), _w(NS, n_fft, 25, 9),
                  # c = 1 - b at a time constant of 18 frames is 0.946: c^(64 + 40) = 3.1e-3 keeps the tile-parallel
                  # recurrence, c^(64 + 74) = 4.7e-4 < 1e-3 refuses k_iir_mask<37>
                  _w(NS, n_fft, 2, 37, tc=18.0 * (n_fft // 4) / SR)]
    # ---- precision="float64": the float64 pipeline's own smoothing kernels (n_fft = 512: run_S_exact) ----
    # (2 nt < XSM_KMAX = 192 never decides: xsm_lds_bytes passes 150 KiB first at every nf -- nf = 3: from nt = 53 on.
    # (3, 95) | (3, 96) therefore both run the two separate passes; the edge that exists at nf = 3 is the byte count's)
    xnt30 = _last_nt(lambda t: x_tiled_ok(30, t))           # xsm_lds_bytes(30, nt) <= 150 KiB
    xnt3 = _last_nt(lambda t: x_tiled_ok(3, t))
    for gate in (S, NS):
        cells += [_w(gate, 512, 3, 95, precision="float64"), _w(gate, 512, 3, 96, precision="float64"),
                  _w(gate, 512, 3, xnt3, precision="float64"), _w(gate, 512, 3, xnt3 + 1, precision="float64"),
                  _w(gate, 512, 30, xnt30, precision="float64"), _w(gate, 512, 30, xnt30 + 1, precision="float64"),
                  _w(gate, 64, 30, 30, small=True, precision="float64")]
    names = [c["name"] for c in cells]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cells


W_CELLS = _w_cells()
W_SIGMA = 0.25 * 10.0 ** (-40.0 / 20.0)        # the noise clip: 40 dB under the loud block (signals.dappled)
# name -> seed offset: a seed that lands a stationary decision within 1e-6 dB of its threshold, leaves the sparse block
# outside [0.02, 0.3] ones, or a non-stationary unit without cells below 0.1 / above 0.9 is changed
# (tests/test_smoothing_widths_host.py holds the conditions)
_W_RESEED = {}


def w_cell_id(c):
    return c["name"]


def w_cell(name):
    return next(c for c in W_CELLS if c["name"] == name)


def w_blocks(c):
    """``(N, chunk_size, padding, blocks)``: the recording of a width cell.  Two chunks; the loud block straddles the seam
    (the last frames of unit 0 and the first of unit 1 lie inside it, and each unit sees 2 nt + 2 hops of it plus the
    padding: a full filter footprint of ones), a sparse block of 48 hops on either side, quiet ends.  ``small``: loud,
    sparse, quiet, loud in 9 + 10 + 6 + 8 hops of one unpadded unit.  Non-stationary cells: every chunk starts quiet (the
    recurrence starts from its first frame: a unit that starts loud keeps its floor at that level and its sigmoid at 0
    throughout) and holds a steady block of 2 nt + 4 hops between two sparse ones; the recording ends in three hops of
    ``steady``, so that the last unit's last frame holds a sigmoid near 1 (its floor is the slow forward pass's last value)
    and zero padding beyond the field differs from replication there.  No input does that at a unit's FIRST frame: the
    forward pass starts at A[0] and the backward pass adds b sum (1 - b)^k fwd[k] with fwd[k] >= (1 - b)^k A[0], so
    S[0] >= A[0] / (2 - b), (A - S) / S <= 1 - b and the sigmoid stays under sigmoid(-10) = 4.5e-5 -- replication of
    frame 0 IS zero padding to that order."""
    n_fft, W, H = w_geometry(c)
    nt = c["nt"]
    # (small: 34 frames, not 20 -- with fewer than nt + 1 frames the taps at |dt| = nt only ever meet the zero padding, and
    # an implementation without them is not wrong on such a field; 34 frames and 33 bins are still under the 61 taps)
    if c.get("small") and c["gate"] == "NS":
        N = 33 * H + 5
        return N, N + 9, 0, [(0, 6 * H, "quiet"), (6 * H, 14 * H, "sparse"), (14 * H, 24 * H, "steady"), (24 * H, N, "sparse"),
                             (N - 3 * H, N, "steady")]
    if c.get("small"):
        N = 33 * H + 5
        return N, N + 9, 0, [(0, 9 * H, "loud"), (9 * H, 19 * H, "sparse"), (19 * H, 25 * H, "quiet"), (25 * H, N, "loud")]
    cs = (2 * nt + 68) * H + 5
    pad = H // 2 + 3
    N = 2 * cs - 7
    if c["gate"] == "NS":
        blocks = []
        for s0 in (0, cs):
            a, b = s0 + 12 * H, s0 + 36 * H
            blocks += [(s0, a, "quiet"), (a, b, "sparse"), (b, b + (2 * nt + 4) * H, "steady"),
                       (b + (2 * nt + 4) * H, min(N, s0 + cs), "sparse")]
        blocks.append((N - 3 * H, N, "steady"))       # (an onset in the last frames of the last unit: below)
        return N, cs, pad, blocks
    half = (2 * nt + 2) * H + W
    q = 12 * H
    return N, cs, pad, [(0, q, "quiet"), (q, cs - half, "sparse"), (cs - half, cs + half, "loud"),
                        (cs + half, N - q, "sparse"), (N - q, N, "quiet")]


def w_block_frames(c, unit, kind):
    """Frames of ``unit`` whose whole window lies inside a block of ``kind``: a boolean (T,) array."""
    n_fft, W, H = w_geometry(c)
    N, cs, pad, blocks = w_blocks(c)
    T = unit["raw"].shape[1]
    in_unit = -(W // 2) + H * np.arange(T)                     # first sample of frame t in the unit; the unit's ends are
    whole = (in_unit >= 0) & (in_unit + W <= len(unit["x"]))   # zero-extended by W / 2: those frames are in no block
    start = unit["dst"][0] - unit["keep"][0] + in_unit         # ... and in the recording
    inside = np.zeros(T, dtype=bool)
    for a, b, k in blocks:
        if k == kind:
            inside |= whole & (start >= a) & (start + W <= b)
    return inside


@functools.lru_cache(maxsize=None)
def _w_case(name):
    c = w_cell(name)
    n_fft, W, H = w_geometry(c)
    nf, nt = c["nf"], c["nt"]
    N, cs, pad, blocks = w_blocks(c)
    seed = 31000 + 7 * n_fft % 1009 + 101 * nf + nt + _W_RESEED.get(name, 0)
    spell = lambda m, unit: None if (m == 1 and c.get("none")) else (m + 0.02) * unit   # noqa: E731
    stationary = c["gate"] == "S"
    kw = dict(stationary=stationary, n_fft=n_fft, chunk_size=cs, padding=pad, prop_decrease=1.0,
              freq_mask_smooth_hz=spell(nf, SR / (n_fft / 2)), time_mask_smooth_ms=spell(nt, 1000.0 * H / SR))
    if "tc" in c:
        kw["time_constant_s"] = c["tc"]
    y = signals.dappled(N, n_fft, blocks, W_SIGMA, seed)
    y_noise = None
    if stationary:
        y_noise = (W_SIGMA * np.random.default_rng(seed + 5).standard_normal(max(64 * H, 2 * W))).astype(F32)
    f64 = c.get("precision") == "float64"
    return dict(cell=c, y=y, y_noise=y_noise, kw=kw, dtype="float64" if f64 else "float32", precision=c.get("precision"))


def w_case(c):
    """Input and keyword arguments of a width cell, laid out like ``cell_case``'s."""
    return _w_case(c["name"])


@functools.lru_cache(maxsize=4)
def _w_oracle(name):
    case = _w_case(name)
    out, units = oracle_units(case["y"].astype(np.float64), SR, separable=True,
                              y_noise=None if case["y_noise"] is None else case["y_noise"].astype(np.float64), **case["kw"])
    c = case["cell"]
    for u in units:
        assert (u["cfg"]["nf"], u["cfg"]["nt"], u["cfg"]["filt"] is not None) == (c["nf"], c["nt"], w_smooth(c)), name
    return out, units


def w_oracle(c):
    return _w_oracle(c["name"])


# ---- TorchGate.forward (n_fft = 1024, float32) at the widths sg_process_batch routes on ----
# rowgate=True: SG_OPT_FORCE_NOROWGATE = 2 (the row gate whenever the shape is eligible), rows of 64 frames, thresholds
# from the rows themselves (the row gate takes no noise row).  Own statistics bound the loud block: with a share p of loud
# frames D dB over the rest, mean + 1.5 std of the row's dB lies D (1.5 sqrt(p (1 - p)) - (1 - p)) over the loud level,
# which is negative only for p < 0.31 -- and D is at most the 40 dB of TorchGate's floor.  A footprint of 2 nt + 1 WHOLE
# loud frames costs more than that many frames of the statistics: a frame is four hops long, so three more frames on each
# open side are partly loud (at the row's start the two reflected frames instead).  nt = 16 / 17: 33 / 35 frames, out of
# the question; nt = 7 / 8 (the nf = 30 pair): 15 / 17 whole + 5 .. 6 partial = 20 .. 23 of 64 frames, p = 0.31 .. 0.36 --
# the threshold lies AT or over the loud level, whatever the rest of the row holds.  So no row-gate cell sums its full
# ktot anywhere (a sum next to the uint16 edge is made in full by k_smooth_bits2 instead: 65025 at (14, 16), variant S); a
# 64-frame row holds 13 loud-touched frames here, p = 0.2, where the threshold is only 8 dB under the loud level, less than ``loud``'s bins move from frame to
# frame: the row-gate rows take ``steady`` blocks (every fourth bin, the same level in every frame).  Every other stationary cell takes its thresholds from a noise row at W_SIGMA
# and holds rows of 2 nt + 70 frames with the full footprint of ones.
def _tw(gate, nf, nt, **kw):
    name = "%s-f%d-t%d" % (gate, nf, nt) + "".join("-%s" % k for k, v in sorted(kw.items()) if v is True)
    return dict(name=name, gate=gate, n_fft=1024, nf=nf, nt=nt, T=64 if kw.get("rowgate") else 2 * nt + 70, **kw)


_TW_NT64 = _last_nt(lambda t: sm2_tile(513, 2, t, tt_max=64) == 64)
_TW_NT32 = _last_nt(lambda t: sm2_tile(513, 2, t, tt_max=64) >= 32)
TW_CELLS = [
    _tw("T", 14, 16, rowgate=True), _tw("T", 14, 17, rowgate=True),      # ktot 65025 | 72900 (and nt <= 16)
    _tw("T", 13, 17, rowgate=True),                                      # ktot 63504: nt <= RG_NTMAX = 16 alone
    _tw("T", 30, 7, rowgate=True), _tw("T", 30, 8, rowgate=True),        # ktot 61504 | 77841
    _tw("T", 2, 81), _tw("T", 2, 82),                 # the tile search from 64 frames (the launch failed here once)
    _tw("T", 2, _TW_NT64), _tw("T", 2, _TW_NT64 + 1),  # ... whose 64-frame tile is left here (sm2_tile: 74 | 75)
    _tw("T", 1, _TW_NT32), _tw("T", 1, _TW_NT32 + 1),  # ... and whose 32-frame tile here (90 | 91; nf = 1: ktot <= 65535)
    _tw("T", 1, 96, none=True), _tw("T", 1, 97),
    _tw("T", 30, 6), _tw("T", 31, 6),
    _tw("TNS", 2, 12), _tw("TNS", 2, 13),             # k_box_mask<nt> is instantiated for nt = 0 .. 12
    _tw("TNS", 2, 19), _tw("TNS", 2, 20), _tw("TNS", 2, 21),
    _tw("TNS", 24, 9), _tw("TNS", 25, 9),
]


def tw_cell_id(c):
    return c["name"]


def tw_route(c):
    """sg_process_batch's routing on the widths (csrc/api.hip), as ``Gate.smooth_route()`` reports it."""
    nf, nt, smooth = c["nf"], c["nt"], w_smooth(c)
    ktot = (nf + 1) ** 2 * (nt + 1) ** 2 if smooth else 1
    general = ("off", 4, 0) if not smooth else ("k_smooth_tiled", 4, 64) if smooth_tiled_ok(nf, nt) else \
        ("k_smooth_f+k_smooth_t", 4, 0)
    if c["gate"] == "TNS":
        box = c.get("kbox", 20) == 20 and (not smooth or (nf <= NS_MAX_NF and 1 <= nt <= 12))
        return ("k_box_mask", 4, 64) if box else general
    if c.get("rowgate") and smooth and ktot <= 65535 and c["T"] <= 64 and 1 <= nf <= 30 and 1 <= nt <= 16:
        return ("k_row_gate", 1, 64)
    if not smooth:
        return ("off", 2, 0)
    if not (nt <= 96 and ktot <= 65535):
        return general
    ct = 1 if (nf + 1) ** 2 <= 255 else 2
    if nf > 30:
        # the tile search is only made for nf <= 30 (t_sm2_ok keeps its default), and stage_smooth_bits hands nf > 30 to
        # the first-generation k_smooth_bits: 64-frame tiles, (64 + 2 nt) rows of F counts -- (nf + 1)^2 >= 1024, so
        # ktot <= 65535 leaves (nt + 1)^2 <= 63, nt <= 6: 76 rows, 82 KiB at most.  This is the only way into that kernel (variant S leaves the bit-mask path at nf > 30).
        return ("k_smooth_bits", ct, 64)
    tt = sm2_tile(513, nf, nt, tt_max=64)
    return ("k_smooth_bits2", ct, tt) if tt else general


def _tw_rows(c, B, seed):
    H, W, T = 256, 1024, c["T"]
    L = (T - 1) * H + 7
    if c["gate"] == "TNS":
        # (two hops of steady at either end: the moving mean over 20 frames, zero beyond the row, leaves the first and the
        # last frame a sigmoid near 1, so that zero padding of the smoothing differs from replication at both ends)
        blocks = [(0, 2 * H, "steady"), (2 * H, 10 * H, "quiet"), (10 * H, 30 * H, "sparse"), (30 * H, (34 + 2 * c["nt"]) * H, "steady"),
                  ((34 + 2 * c["nt"]) * H, L - 2 * H, "sparse"), (L - 2 * H, L, "steady")]
    elif c.get("rowgate"):
        blocks = [(0, 10 * H, "steady"), (10 * H, 40 * H, "sparse"), (40 * H, L - 2 * H, "quiet"), (L - 2 * H, L, "steady")]
    else:
        a = (2 * c["nt"] + 2) * H + W // 2
        blocks = [(0, a, "loud"), (a, a + 44 * H, "sparse"), (a + 44 * H, L - 6 * H, "quiet"), (L - 6 * H, L, "loud")]
    return np.stack([signals.dappled(L, 1024, blocks, W_SIGMA, seed + 13 * b) for b in range(B)]), blocks


@functools.lru_cache(maxsize=None)
def _tw_case(name):
    c = next(c for c in TW_CELLS if c["name"] == name)
    H = 256
    seed = 47000 + 101 * c["nf"] + c["nt"] + _W_RESEED.get(name, 0)
    x, blocks = _tw_rows(c, 3 if c.get("rowgate") else 2, seed)
    spell = lambda m, unit: None if (m == 1 and c.get("none")) else (m + 0.02) * unit   # noqa: E731
    kw = dict(n_fft=1024, nonstationary=c["gate"] == "TNS", freq_mask_smooth_hz=spell(c["nf"], SR / 512.0),
              time_mask_smooth_ms=spell(c["nt"], 1000.0 * H / SR))
    xn = None
    if c["gate"] == "T" and not c.get("rowgate"):
        xn = (W_SIGMA * np.random.default_rng(seed + 5).standard_normal((1, 64 * H))).astype(F32)
    return dict(cell=c, x=x, xn=xn, kw=kw, blocks=blocks)


def tw_case(c):
    return _tw_case(c["name"])


@functools.lru_cache(maxsize=4)
def _tw_oracle(name):
    case = _tw_case(name)
    xn = None if case["xn"] is None else case["xn"].astype(np.float64)
    return torchgate_units(case["x"].astype(np.float64), SR, xn=xn, window=tile_window(1024), separable=True, **case["kw"])[1]


def tw_oracle(c):
    return _tw_oracle(c["name"])


# ---- the moving mean of TorchGate's non-stationary gate (n_movemean_nonstationary), n_fft = 1024 ----
# forward: k_boxcar_sigmoid (32-frame blocks; k_box_mask only knows the default 20) on rows of M_T frames; lengths=: the
# moving mean of csrc/rows.hip (left = (kbox - 1) / 2).  padding="same" puts (k - 1) // 2 zeros on the left and k / 2 on the
# right: asymmetric for even k.
M_T = 40
M_CELLS = [dict(name="mm%d" % k, kbox=k, lengths=False) for k in (1, 2, 3, 19, 21, 32, 33, M_T - 1, M_T, M_T + 5, 2 * M_T + 1)] + \
          [dict(name="mm%d-lengths" % k, kbox=k, lengths=True) for k in (1, 2, 21, 30)]      # (the shortest row: 24 frames)
M_LENGTHS = (M_T, 24, 33)       # frames per row of the lengths= cells


def m_cell_id(c):
    return c["name"]


@functools.lru_cache(maxsize=None)
def _m_case(name):
    c = next(c for c in M_CELLS if c["name"] == name)
    H = 256
    frames = M_LENGTHS if c["lengths"] else (M_T, M_T)
    L = (M_T - 1) * H + 7
    x = np.full((len(frames), L), np.nan, dtype=F32) if c["lengths"] else np.zeros((len(frames), L), dtype=F32)
    lens = []
    for b, T in enumerate(frames):
        n = (T - 1) * H + 7
        blocks = [(0, 5 * H, "quiet"), (5 * H, 14 * H, "sparse"), (14 * H, 22 * H, "steady"), (22 * H, n, "sparse")]
        x[b, :n] = signals.dappled(n, 1024, blocks, W_SIGMA, 53000 + 17 * c["kbox"] + b)
        lens.append(n)
    kw = dict(n_fft=1024, nonstationary=True, n_movemean_nonstationary=c["kbox"],
              freq_mask_smooth_hz=2.02 * SR / 512.0, time_mask_smooth_ms=2.02 * 1000.0 * H / SR)
    return dict(cell=c, x=x, lengths=np.array(lens, dtype=np.int64) if c["lengths"] else None, kw=kw)


def m_case(c):
    return _m_case(c["name"])


@functools.lru_cache(maxsize=4)
def _m_oracle(name):
    case = _m_case(name)
    window = tile_window(1024)
    if case["lengths"] is None:
        return torchgate_units(case["x"].astype(np.float64), SR, window=window, **case["kw"])[1]
    return [torchgate_units(case["x"][b:b + 1, :int(n)].astype(np.float64), SR, window=window, **case["kw"])[1][0]
            for b, n in enumerate(case["lengths"])]


def m_oracle(c):
    return _m_oracle(c["name"])
