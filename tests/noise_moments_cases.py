"""Noise clips for the two-launch noise statistics (k_noise_moments + k_colstats1_final; csrc/api.hip: stage_stats),
shared by tests/test_noise_moments_host.py (what every clip does, held on the oracle) and tests/test_gpu_noise_moments.py.

A k_noise_moments workgroup owns one slice of ``FPS[n_fft]`` consecutive frames (its teams minus the one that transforms
the pivot frame 0); the route takes clips of at least 512 frames and at most 256 slices.  Clips are ``(T - 1) hop + 3``
samples, like parity_budget's: T frames, the last one mostly padding."""
import numpy as np

from oracle import spectralgate_oracle as O

SR = 48000
FPS = {256: 63, 512: 31, 1024: 15, 2048: 3}     # frames per slice: 1024 threads / threads per frame - 1
MIN_FRAMES, MAX_SLICES = 512, 256
SIGMA = 1e-3                                    # noise level of every clip

# (n_fft, T): n_fft = 1024 at the route's lower bound, one frame over it, a whole number of slices (525 = 35 * 15), two
# frames into the last slice, and a clip of 70 slices; the other geometries at the smallest T >= 512 that is no multiple
# of their slice (512 at all three)
GEOMS = [(1024, 512), (1024, 513), (1024, 525), (1024, 527), (1024, 1041), (256, 512), (512, 512), (2048, 512)]
VARIANT_GEOM = (1024, 527)   # every kind of clip runs here; the other cells run "noise" and "zeros_straddle"
KINDS = ["noise", "zeros_frame0", "zeros_inside", "zeros_straddle", "zeros_last5", "tone", "stereo", "int16", "float64",
         "nan"]


def case_ids():
    out = []
    for n_fft, T in GEOMS:
        kinds = KINDS if (n_fft, T) == VARIANT_GEOM else ["noise", "zeros_straddle"]
        out += [(n_fft, T, k) for k in kinds]
    return out


def case_name(c):
    return "nfft%d-T%d-%s" % c


def zero_run(n_fft, T, kind):
    """Frames [t0, t1] of the clip's zero-power run, or None."""
    fps = FPS[n_fft]
    if kind == "zeros_frame0":
        return 0, 0
    if kind == "zeros_inside":       # inside slice 3, touching neither of its ends
        return 3 * fps + 1, 3 * fps + max(1, min(fps - 2, 4))
    if kind == "zeros_straddle":     # the last frame of slice 4 and the first two of slice 5
        return 5 * fps - 1, 5 * fps + 1
    if kind == "zeros_last5":
        return T - 5, T - 1
    return None


def tone_band(n_fft):
    return n_fft // 8        # bin-centred: 6 kHz at every n_fft


def build(n_fft, T, kind):
    """The clip as the array handed to the engine, (C, L); ``float64(clip)`` is what the oracle gets."""
    H = n_fft // 4
    L = (T - 1) * H + 3
    rng = np.random.default_rng([n_fft, T, KINDS.index(kind)])
    y = SIGMA * rng.standard_normal((2 if kind == "stereo" else 1, L))
    run = zero_run(n_fft, T, kind)
    if run is not None:
        # frame t reads samples [t H - n_fft / 2, t H + n_fft / 2)
        y[:, max(0, run[0] * H - n_fft // 2):min(L, run[1] * H + n_fft // 2)] = 0.0
    if kind == "tone":
        # a Hann-windowed bin holds sigma sqrt(1.5 / n_fft) of noise (rms) and A / 2 of a bin-centred tone: 80 dB apart
        A = 2e4 * SIGMA * np.sqrt(1.5 / n_fft)
        t = np.arange(L)
        on = (t // (4 * n_fft)) % 2 == 1
        y[0] += np.where(on, A * np.sin(2 * np.pi * tone_band(n_fft) * t / n_fft), 0.0)
    if kind == "nan":
        y[0, L // 2] = np.nan
    if kind == "int16":
        return np.round(y * (3000.0 / SIGMA)).astype(np.int16)
    if kind == "float64":
        return y
    return y.astype(np.float32)


def oracle(n_fft, clip):
    """(thresh[F], raw dB [F, T], floor [F, 1], |Z| [F, T]) of a clip on the float64 oracle."""
    H = n_fft // 4
    y = np.asarray(clip, dtype=np.float64)
    thr, _, _ = O.noise_threshold_S(y, n_fft, n_fft, H, 1.5, 10 ** 9, True)
    with np.errstate(invalid="ignore"):
        Z = np.abs(O.stft_scipy(np.mean(y, axis=0), n_fft, n_fft, H))
        db = 20.0 * np.log10(Z + O.EPS64)
        floor = np.max(db, axis=-1, keepdims=True) - 80.0
    return thr, db, floor, Z
