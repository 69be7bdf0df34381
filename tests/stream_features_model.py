"""Float64 model of the feature steps of a stream bank (a helper, not a test): the yardstick of
tests/test_stream_features_host.py and tests/test_gpu_stream_features.py, built on tests/stream_spectrum_model.py -- ``Y``
from the oracle, then the formula in numpy:

    lin[m, t] = sum_k fb[k, m] * |r * Y[k, t]| ** power        feat = ln(lin + eps) if log else lin

``Y = Z * mask`` is scipy.signal.stft's scaling (1 / sum(window)), so ``r = 1`` for ``scale="scipy"`` and ``r = sum(window)``
for ``scale="torch"`` (s = 1 on the unscaled transform).  The model sums in extended precision (its own error is nothing
against the bounds); ``lin_sequential`` is the float64 sum in the engine's stated order, for the one case where the order
itself shows (partial sums that overflow).

The bounds are derived, not measured.  With ``b_t`` what a frame's ``Y`` may be off by (stream_spectrum_model.frame_bound,
times r), ``a_k = |fb[k, m]|``, ``y_k = |r Y|``, ``n_m`` the width of filter m's hull and ``g = (n_m + 3) * 2**-53``:

    power 2:  E = sum_k a_k (2 y_k b_t + b_t**2) + g * sum_k a_k y_k**2
    power 1:  E = sum_k a_k b_t                  + g * sum_k a_k y_k

(first term: the spectrum's error carried through the power; second: the power of a bin is two roundings, its product with
the weight and the running sum one each -- n_m + 2 in all, plus one of slack).  A float32 result adds ``2**-24 |value|``; the
log turns E into ``E / (lin + eps - E)`` plus four ulp of the result type, which needs ``E < lin + eps``."""
import numpy as np

from noisereduce_amd.torchgate.filterbank import mel_filterbank, support_tables
from oracle import spectralgate_oracle as O
from tests import parity_budget as PB
from tests import stream_spectrum_model as SM

U = 2.0 ** -53
LD = np.longdouble
BANKS = ("mel40", "one", "wide300", "dense_signed", "zero_nyq")
DEFECTS = ("descending_k", "hull_short_lo", "hull_short_hi", "nyquist_dropped", "column_plus_one", "scale_after_power",
           "mask_float32")


def bank(name, n_fft, sr=PB.SR):
    """(F, M) float32 filterbanks, small and chosen to reach every branch of the filter sum."""
    F = n_fft // 2 + 1
    rng = np.random.default_rng(n_fft + 17 * BANKS.index(name))
    if name == "mel40":
        return mel_filterbank(sr, n_fft, 40).numpy()
    if name == "one":                    # M = 1: a ramp over 37 bins with a zero inside its hull
        fb = np.zeros((F, 1), np.float32)
        fb[F // 4:F // 4 + 37, 0] = np.linspace(0.1, 1.0, 37, dtype=np.float32)
        fb[F // 4 + 5, 0] = 0.0
        return fb
    if name == "wide300":                # more filters than a workgroup has threads; hulls of 1 .. 19 bins (8-blocks and tails)
        fb = np.zeros((F, 300), np.float32)
        for m in range(300):
            w = 1 + m % 19
            lo = (m * (F - w)) // 299
            fb[lo:lo + w, m] = rng.uniform(0.05, 1.0, w).astype(np.float32)
        assert fb[F - 1, 299] != 0 and fb[0, 0] != 0
        return fb
    if name == "dense_signed":           # every hull is [0, F): the Nyquist term of the sum; signed weights (log=False only)
        fb = rng.standard_normal((F, 5)).astype(np.float32)
        fb[fb == 0] = 0.5
        return fb
    if name == "zero_nyq":               # an all-zero filter and one supported at bin F - 1 alone
        fb = np.zeros((F, 4), np.float32)
        fb[3:12, 0] = rng.uniform(0.1, 1.0, 9).astype(np.float32)
        fb[F - 1, 2] = 0.75
        fb[0:3, 3] = (1.0, 0.5, 0.25)
        return fb
    raise KeyError(name)


def scale_ratio(scale, W):
    """r of the module docstring: what the scipy-scaled Y is multiplied with before the power."""
    return 1.0 if scale == "scipy" else float(O.hann_periodic(W).sum())


def engine_scale(W):
    """The engine's own 1 / sum(window) of its periodic Hann window, bit for bit: the same libm cosine in the same
    expression, summed in index order (csrc/api.hip).  Check 2 divides the engine's Y by it to get back the unscaled
    product: any other sum(window) differs from it by roundings of its own, which is all that check allows."""
    import math
    S = 0.0
    for k in range(W):
        S += 0.5 - 0.5 * math.cos(2.0 * math.pi * k / W)
    return 1.0 / S


def _weights(fb, defect=None):
    """The (F, M) weights the sum really uses, in extended precision, with a planted defect."""
    w = np.asarray(fb, dtype=np.float32).astype(LD)
    F, M = w.shape
    khull, _ = support_tables(fb)
    if defect == "hull_short_lo":
        for m in range(M):
            if khull[m, 1] > khull[m, 0]:
                w[khull[m, 0], m] = 0
    elif defect == "hull_short_hi":
        for m in range(M):
            if khull[m, 1] > khull[m, 0]:
                w[khull[m, 1] - 1, m] = 0
    elif defect == "nyquist_dropped":
        w[F - 1, :] = 0
    elif defect == "column_plus_one":
        w = np.roll(w, -1, axis=1)
    return w


def powers(Y, power, r, defect=None):
    """p[k, t] = |r Y|**power in extended precision (real and imaginary parts scaled first, as the engine scales them)."""
    Y = np.asarray(Y)
    re, im = Y.real.astype(LD), Y.imag.astype(LD)
    r = LD(r)
    if defect == "scale_after_power":
        s = re * re + im * im
        return (s if power == 2 else np.sqrt(s)) * r
    re, im = re * r, im * r
    s = re * re + im * im
    return s if power == 2 else np.sqrt(s)


def linear(Y, fb, power, r, defect=None):
    """lin (M, T) in extended precision."""
    return _weights(fb, defect).T @ powers(Y, power, r, defect)


def finish(lin, log, eps):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.log(lin + LD(eps)) if log else lin


def features(Z, mask, fb, power, r, log, eps, defect=None):
    """The model's feat (M, T), extended precision, of Y = Z * mask."""
    m = np.asarray(mask, dtype=np.float64)
    if defect == "mask_float32":
        m = m.astype(np.float32).astype(np.float64)
    return finish(linear(np.asarray(Z) * m, fb, power, r, defect), log, eps)


def lin_sequential(p, fb, descending=False):
    """The float64 sum of every filter over its hull, one addition per bin in ascending k (the engine's order) or, the
    planted defect, descending: (M, T) float64.  p: (F, T) float64 powers."""
    fb = np.asarray(fb, dtype=np.float32).astype(np.float64)
    khull, _ = support_tables(fb)
    out = np.zeros((fb.shape[1], p.shape[1]))
    with np.errstate(over="ignore", invalid="ignore"):
        for m in range(fb.shape[1]):
            ks = range(khull[m, 0], khull[m, 1])
            for k in (reversed(ks) if descending else ks):
                out[m] = out[m] + fb[k, m] * p[k]
    return out


def frame_bounds(Y, Z, r):
    """b_t (T,): what the spectrum test holds a frame of the float64 Y to, in the scaling of the powers."""
    return r * SM.frame_bound(np.asarray(Y), np.asarray(Z), False, PB.F64_REL, PB.EPS32, PB.POOL)


def budget(Y, fb, power, r, b_t=None, extra_u=0.0):
    """E (M, T) of the module docstring for lin; b_t None: the summation terms alone (Y is the engine's own, exact).
    extra_u: further roundings per term that the REFERENCE carries (a Y that was itself rounded after scaling)."""
    a = np.abs(np.asarray(fb, dtype=np.float32).astype(np.float64))
    y = np.abs(np.asarray(Y)) * r
    khull, _ = support_tables(fb)
    g = ((khull[:, 1] - khull[:, 0] + 3 + extra_u) * U)[:, None]
    E = g * (a.T @ (y ** power))
    if b_t is not None:
        b = np.asarray(b_t, dtype=np.float64)[None, :]
        E = E + (a.T @ (2 * y * b + b * b) if power == 2 else a.sum(axis=0)[:, None] * b)
    return E


def tolerance(lin, E, log, eps, dtype):
    """What feat may be off by, cell by cell; inf where the log bound does not exist (E >= lin + eps)."""
    lin = np.asarray(lin, dtype=np.float64)
    narrow = np.dtype(dtype) == np.float32
    if not log:
        return E + (2.0 ** -24 * np.abs(lin) if narrow else 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        room = lin + eps - E
        val = np.abs(np.log(lin + eps))
        return np.where(room > 0, E / room, np.inf) + 4 * (2.0 ** -23 if narrow else 2.0 ** -52) * val


def bad_cells(feat, want, tol):
    """(m, t) of the cells over their tolerance; a NaN on one side only counts."""
    feat = np.asarray(feat).astype(LD)
    assert feat.shape == want.shape == tol.shape, (feat.shape, want.shape, tol.shape)
    with np.errstate(invalid="ignore"):
        d = np.abs(feat - want)
        same = (np.isnan(feat) & np.isnan(want)) | (np.isinf(feat) & (feat == want))
    return np.argwhere(~same & ~(d <= tol))


def check(tag, feat, Z, mask, fb, power, scale, log, eps, W, engine_Y=None):
    """The check of tests/test_gpu_stream_features.py: feat (M, T) of one channel against the model of Y = Z * mask with
    the oracle bound -- or, engine_Y given (the complex128 Y of push_spectrum on a twin bank), against the formula on that Y
    with the summation terms alone.  Returns the bad cells."""
    r = scale_ratio(scale, W)
    if engine_Y is None:
        Y = np.asarray(Z) * np.asarray(mask, dtype=np.float64)
        E = budget(Y, fb, power, r, frame_bounds(Y, Z, r))
    else:
        # (under scale="torch" the reference is Y / engine_scale: Y carries the rounding of its own scale product, which the
        # engine's powers never saw -- one more rounding per factor of the power)
        Y = np.asarray(engine_Y)
        if scale == "torch":
            r = LD(1.0) / LD(engine_scale(W))
        E = budget(Y, fb, power, float(r), None, extra_u=0.0 if scale == "scipy" else float(power))
    lin = linear(Y, fb, power, r)
    want = finish(lin, log, eps)
    tol = tolerance(lin, E, log, eps, np.asarray(feat).dtype)
    assert np.isfinite(tol[~np.isnan(np.asarray(want, dtype=np.float64))]).all(), tag      # no cell is left out
    bad = bad_cells(feat, want, tol)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(np.asarray(feat).astype(LD) - want) / tol
    print("%s: largest error / tolerance %.3g over %d cells" % (tag, float(np.nanmax(ratio)) if ratio.size else 0.0, ratio.size))
    return bad


# ---- the cases of the oracle test (GPU) and of the host test's conditions --------------------------------------------------
def _cases():
    picks = {("stream-S", 256, True): ("mel40", 2, "scipy", True), ("stream-S", 256, False): ("wide300", 1, "torch", True),
             ("stream-NS", 256, True): ("dense_signed", 2, "torch", False), ("stream-NS", 256, False): ("zero_nyq", 1, "scipy", True),
             ("stream-S", 1024, True): ("zero_nyq", 2, "torch", True), ("stream-S", 1024, False): ("dense_signed", 1, "scipy", False),
             ("stream-NS", 1024, True): ("mel40", 1, "torch", True), ("stream-NS", 1024, False): ("one", 2, "scipy", True),
             ("stream-S", 4096, True): ("wide300", 2, "scipy", True), ("stream-S", 4096, False): ("dense_signed", 2, "scipy", False),
             ("stream-NS", 4096, True): ("one", 1, "torch", False), ("stream-NS", 4096, False): ("mel40", 2, "torch", True)}
    out = []
    for c in PB.TILE_CELLS:
        key = (c["path"], c["n_fft"], c["col"] == 0)
        if key in picks:
            b, power, scale, log = picks[key]
            # (eps: each convention's default -- push_features' 1e-10 under the scipy scaling, gated_filterbank's 1e-6 on
            # the unscaled transform, where b_t is sum(window) times larger and 1e-10 would leave a gated cell no log bound)
            out.append(dict(cell=c, bank=b, power=power, scale=scale, log=log, eps=1e-10 if scale == "scipy" else 1e-6))
    return out


CASES = _cases()


def case_id(c):
    return "%s-%s-p%d-%s-%s" % (PB.tile_cell_id(c["cell"]), c["bank"], c["power"], c["scale"], "log" if c["log"] else "lin")


# ---- the order case: partial sums that overflow in ascending order and not in descending -----------------------------------
def order_case():
    """A bin-centred tone so loud that, unscaled (scale="torch"), its three Hann bins have powers q, 4q, q with
    5q > DBL_MAX > 4q, and a filter (+1, +1, -1) on them: ascending k gives q + 4q = inf, descending -q + 4q + q stays
    finite.  Returns dict(y float64 (N,), n_fft, W, H, fb, k0)."""
    n_fft = W = 256
    H = 64
    k0 = 40
    N = W + 24 * H
    q = 0.22 * np.finfo(np.float64).max                     # the side bins' power |A W / 8|**2: 4q = 0.88, 5q = 1.1 DBL_MAX
    A = np.sqrt(q) * 8.0 / W
    y = A * np.cos(2 * np.pi * k0 * np.arange(N) / n_fft)
    fb = np.zeros((n_fft // 2 + 1, 2), np.float32)
    fb[k0 - 1:k0 + 2, 0] = (1.0, 1.0, -1.0)
    fb[k0 - 1:k0 + 2, 1] = (-1.0, 1.0, 1.0)                 # the mirror image: finite ascending, inf descending
    return dict(y=y, n_fft=n_fft, W=W, H=H, fb=fb, k0=k0)


def order_bad(feat, Z, mask, oc):
    """The check of the order case: on the frames that lie wholly inside the tone, feat (2, T) is infinite exactly where
    the ascending float64 sum is, and elsewhere within 1e-11 of it (Y is held to 1e-12 of the frame's peak, so the three
    comparable powers to 2e-12 each and their sum, 6q against a result of 4q, to 3e-12).  Returns the bad (m, t)."""
    W, H, N = oc["W"], oc["H"], len(oc["y"])
    t = np.arange(Z.shape[1])
    inside = (t * H - W // 2 >= 0) & (t * H - W // 2 + W <= N)
    p = powers(np.asarray(Z) * np.asarray(mask, dtype=np.float64), 2, scale_ratio("torch", W)).astype(np.float64)
    want = lin_sequential(p, oc["fb"])
    feat = np.asarray(feat, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.where(np.isinf(want), feat == want, np.abs(feat - want) <= 1e-11 * np.abs(want))
    return np.argwhere(~ok & inside[None, :]), want, inside
