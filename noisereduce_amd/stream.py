"""``StreamBank`` / ``StreamGate`` -- the gate for live audio: streams gated block by block on the GPU, with the
stationary gate (a fixed noise profile, or one learnt from the stream itself) or the non-stationary one (no profile, a
bounded lookahead).

Everything else in the package needs the last sample of a recording before the first one comes out.  A ``StreamBank``
holds many independent streams with a fixed noise profile; each step takes whatever block every stream received (0
samples, 1 sample, a second -- different streams different lengths) and returns the samples that became final, in a fixed
number of kernel launches per step (sg_stream_push, include/mi355gate.h).

With ``W`` = win_length, ``H`` = hop_length, ``h = W // 2``, ``nt`` = the time half width of the mask smoothing (0 with
smoothing off) and ``n`` samples received, a stream has emitted ``emitted(n, W, H, nt) = max(0, (t_dec(n) - nt + 1) * H - h)``
samples, ``t_dec(n) = floor((n + h - W) / H)``: every sample whose frames all have their final mask.  The delay is below
``latency_samples = W + (nt + 1) * H`` samples (3 584 at the 48 kHz defaults: 75 ms).  ``flush`` ends a stream: the
remaining frames see zeros after the last sample and the remaining samples come out.

The concatenated output of a stream equals ``reduce_noise(y, sr, y_noise=..., stationary=True, chunk_size=None,
padding=0)`` of the whole signal, whatever the block split, with one designed difference: the -top_db floor is causal.
Offline a band's floor is its maximum over the whole recording minus 80 dB; here it is the maximum over the frames up
to and including the current one.  The two agree wherever no band's maximum exceeds its threshold by more than 80 dB.
A NaN / Inf sample gates every band from its first frame on until the slot is flushed or reset; the NaN itself survives.
A stream's output does not depend, bitwise, on how it was cut into blocks, on its slot, or on the other streams of a step.

``stationary=False`` streams the non-stationary gate (``reduce_noise``'s default) and takes no noise profile.  Offline its
smoother runs forward and then backward over the whole recording; here the forward pass ``fwd[f, t] = b A[f, t] + (1 - b)
fwd[f, t - 1]`` (``fwd[f, -1] = A[f, 0]``, ``A = |X|``, ``b`` from ``time_constant_s``) is carried per band, and the level of
frame ``t`` is the same forward-backward smoother of the signal as known ``L = lookahead_frames`` frames later: with ``e =
min(t + L, T - 1)``, ``s = fwd[f, e]``, then ``s = b fwd[f, k] + (1 - b) s`` for ``k = e, ..., t``.  The mask is the offline
one from there on.  ``L = int(lookahead_ms / (H / sr * 1000))`` adds to ``nt`` everywhere above: ``emitted(n, W, H, nt +
L)``, ``latency_samples = W + (nt + L + 1) * H``.  With ``L >= T - 1`` the output is ``reduce_noise(y, sr, stationary=False,
chunk_size=None, padding=0)`` of the whole signal; the distance shrinks with ``L`` (16 kHz, n_fft 512 / 400 / 160,
``time_constant_s=0.1``: 0.45 of the offline output's peak at ``L = 0``, 2.7e-3 at 32, 2.9e-7 at 128).  With a long time
constant and a small ``L`` -- the default ``time_constant_s=2`` at ``L`` up to 64 -- the level lags the signal as any
causal smoother does and the output differs from the offline one by more than its peak: by design, as the causal floor is.
Digital silence gives ``0 / 0`` = NaN as offline; a NaN / Inf sample keeps the band levels NaN until the slot is flushed or
reset.

``noise_from_stream=True`` is the stationary gate without a noise clip, as ``reduce_noise(y, sr, stationary=True)`` is
offline: there a band's threshold is the mean plus ``n_std_thresh_stationary`` standard deviations of the band's floored dB
values over the whole recording; here the two are a running estimate per (stream, channel) and band.  The recurrence is the
definition.  For frames ``t = 0, 1, ...`` in order::

    db = 20 log10(|X[f, t]| + eps);  rmax = max(rmax, db);  x = max(db, rmax - top_db)     (the causal floor; NaN-sticky)
    if t < learn_frames (or learning is unlimited):
        Wn = lam * Wn + 1;  d = x - mu;  mu = mu + d / Wn;  M2 = lam * M2 + d * (x - mu)
    thr = mu + n_std_thresh_stationary * sqrt(M2 / Wn);  the cell passes when x > thr

from ``Wn = mu = M2 = 0``.  ``noise_memory_s=None`` is ``lam = 1``: the cumulative mean and standard deviation (``ddof = 0``,
as the reference's ``np.std``) of frames ``0 .. t``; otherwise ``lam = exp(-H / (sr * noise_memory_s))`` forgets
exponentially.  ``noise_learn_s`` holds the profile after ``learn_frames = int(noise_learn_s * sr / H)`` frames (``None``:
it keeps learning).  Frame ``t`` is part of its own threshold, as every frame of a recording is offline.  What follows from
the definition: frame 0 has ``M2 = 0`` and ``thr = x``, so it is gated whole; a band whose dB value is exactly constant
(leading digital silence) has ``d = 0`` exactly and stays exactly gated; a NaN / Inf sample gates every band until the slot
is flushed or reset, forgetting or not; a memory of less than about three hops gates EVERYTHING -- frame ``t`` has the
share ``1 / Wn`` of its own statistics, a cell can lie at most ``sqrt(Wn - 1)`` deviations above its own mean, and ``Wn``
stays below ``1 / (1 - lam)``: with ``n_std_thresh_stationary = 1.5`` nothing passes for ``lam <= 0.69``
(``noise_memory_s <= 2.7 H / sr``; in general ``lam <= 1 - 1 / (1 + n_std^2)``).  Every channel of a multichannel stream has its own statistics -- the reference
takes one threshold from the channel mean; the two are the same thing for one channel.  With ``lam = 1``, unlimited learning
and no band ranging over more than ``top_db``, ``noise_profile`` just before the flush is the reference's threshold of the
whole signal.  Everything else -- frames, ``emitted``, ``latency_samples``, flush, launches per step, bitwise independence
of the block split, the slot and the other streams -- is the fixed-profile bank's.

``precision="float64"`` makes the bank exact: its streams are the gate above at the block's own sample type.  The default
bank stores every frame's segment as float32 and rounds every sample to float32 before it leaves the device (a
non-stationary one also keeps its sigmoid and smoothed mask rows as float32), so a float64 block comes back float32-accurate
in a float64 array and integer blocks are refused.  The exact bank keeps all of that in float64 -- the transforms, the ring
and the overlap-add carry are float64 in both -- and takes float32, float64, int16 and int32 blocks, every slot getting its
own block's type back:

* float64 blocks come back float64-accurate (1e-12 of peak against the float64 model instead of 1e-7);
* float32 blocks are that float64 result rounded once;
* int16 / int32 blocks are ``trunc(float64 result)``, as ``ndarray.astype`` truncates and as ``reduce_noise`` returns integer
  recordings offline: where the causal floor is not live, ``reduce_noise(y_int, sr, ..., chunk_size=None, padding=0)`` of the
  whole recording.  The caveat is the offline one: a float64 value within rounding noise of an integer may truncate to either
  neighbour.  NaN (digital silence in a non-stationary bank is ``0 / 0``) becomes integer 0 -- what ``astype`` makes of NaN
  differs from platform to platform, so 0 is the stated choice.  Values outside the integer range are as unspecified as
  ``astype``'s.

A step whose blocks all share one sample type travels in that type both ways (an int16 step uploads and downloads 2 bytes
per sample); a step of mixed types travels as float64, which holds all four types exactly, and every slot's result is
converted on arrival with the same rounding / truncation / NaN rule.  Either way a slot's samples are bitwise those of the
same stream pushed alone.  Everything else -- frames, ``emitted``, ``latency_samples``, flush, four launches per step,
bitwise independence of the block split, the slot and the other streams -- is unchanged; the cost is a scratch twice as wide
and, non-stationary, mask rows of 8 bytes (``state_bytes(..., exact=True)``).

A stream is not tied to the bank it started in.  ``snapshot(slots)`` reads out what a stream needs to go on -- the samples
no applied frame has covered yet, the open overlap-add sums, the mask rows later frames smooth over, the running band maxima,
the learnt noise statistics or the forward level and the rows still ahead of the lookahead, the slot's threshold -- as a
``StreamState``, and ``restore({slot: state})`` writes it into any slot of any bank of the same gate (same geometry, kind,
smoothing, lookahead, precision and gate parameters; another ``n_streams``, ``max_block``, device or, through
``to_bytes`` / ``from_bytes``, process).  The stream goes on there bit for bit as it would have without the move; restoring
one state twice forks a stream.  One launch per call, no host synchronisation for device states.

``push_spectrum`` / ``flush_spectrum`` are ``push`` / ``flush`` that also hand out the gated spectrogram ``Y = Z * mask``, frame
by frame: the product the step inverts, stored on its way to the inverse transform (sg_stream_push_spectrum; DESIGN section
13e).  With ``lag = nt + lookahead_frames`` a stream has applied ``frames_applied(n, W, H, lag) = max(0, t_dec(n) - lag + 1)``
frames after ``n`` samples (``emitted == max(0, frames * H - h)``); a step reports the newly applied ones, a flush all
remaining ones up to ``T = (N + 2 h - W) // H + 1``.  The contract:

* after any sequence of steps a stream's reported frames, concatenated, are frames ``0 .. A(n) - 1`` (``0 .. T - 1`` after the
  flush); frame ``t`` is the frame of samples ``[t H - h, t H - h + W)``;
* each frame is the offline ``Z * mask`` of the whole signal for ``padding=0`` -- ``Z`` scaled as ``scipy.signal.stft`` scales
  it (``1 / sum(window)``), the mask evaluated once per band in float64, ``Y`` the float64 product rounded once to its type,
  bins 0 and ``n_fft / 2`` with an imaginary part of exactly ``+0.0`` -- with the causal ``-top_db`` floor as the one designed
  difference and a non-stationary bank's bounded lookahead exactly as for the audio; ``scipy.signal.istft`` of the concatenated
  ``Y`` is the concatenated audio;
* ``Y`` and ``mask`` are bitwise independent of the block split, the slot, the other streams of the step and their sample
  types, and of whether earlier steps were ``push`` or ``push_spectrum`` (frames that pass in a ``push`` step are simply not
  reported); the audio of a ``push_spectrum`` step is bitwise the audio of ``push``;
* ``snapshot`` / ``restore`` between spectrum steps continues ``Y`` bit for bit; the payload does not change.

``Y`` is complex64 for a float32 block and complex128 for a float64 / int16 / int32 one, on any bank kind: the transforms and
the masks are float64 in every bank.  Same four launches per step, no host synchronisation for device tensors.

``set_filterbank(fb)`` and ``push_features`` / ``flush_features`` are the same steps with every applied frame reduced to
filterbank (log-mel) features on the device, ``sum_k fb[k, m] |s Z mask| ** power`` or its ``ln(. + eps)``, instead of
stored as ``F`` complex bins (sg_stream_set_filterbank / sg_stream_push_features): the frames, the audio
and the mask of ``push_spectrum``, float64 sums in a fixed order rounded once, bitwise independent of the block split, the
slot, the other streams and the kind of the earlier steps.  The filterbank belongs to the bank, not to a stream's state.

``algorithm="torchgate"`` (with ``stationary=False``; or ``StreamBank.from_torchgate(tg, n_streams)``) streams the other gate
of the package, ``TorchGate(nonstationary=True)``, and this one EQUALS the offline gate: there is no designed difference.  Its
level is a moving mean over ``K = n_movemean_nonstationary`` frames that reads ``lo = (K - 1) // 2`` frames behind a frame and
``L = K - 1 - lo`` ahead of it and nothing else, so a lookahead of ``L`` frames is all it needs.  The definition, with the
float32 Hann table ``TorchGate`` hands the engine and ``A = |X|`` of the unscaled transform:

* frame ``t`` is the frame of samples ``[t H - h, t H - h + W)``, ``W`` even: the samples ``torch.stft(center=True)`` windows
  (for ``W < n_fft`` torch centres the window in the ``n_fft`` frame and the bank puts it first: another phase, which audio,
  mask and features do not see);
* ``S[f, t] = (1 / K) * sum of A[f, q]`` over ``q`` in ``[t - lo, t - lo + K)`` cut to ``[0, T)``, every sum taken afresh in
  ascending ``q`` in float64, ``T - 1`` the stream's last frame; ``raw = sigmoid(((A - S) / S - n_thresh_nonstationary) /
  temp_coeff_nonstationary)``, ``0 / 0`` = NaN as offline;
* the mask is ``prop_decrease * (raw - 1) + 1`` smoothed with the zero-padded triangle over the stream's own ``(F, T)`` field
  -- ``prop_decrease`` FIRST, the value outside the field 0: TorchGate's order, not the scipy gate's;
* a frame is decided once frame ``t + L`` is in, or at the flush: ``lookahead_frames == L``, ``emitted(n, W, H, nt + L)``,
  ``latency_samples = W + (nt + L + 1) * H`` (``K = 20``, n_fft 1024 at 16 kHz: 14 frames, 288 ms);
* after the flush a stream of ``N >= 2 W`` samples has emitted ``N`` samples: the first ``H * (N // H)`` are
  ``TorchGate(...)(x[None])[0]``, the other ``N mod H`` the same overlap-add over the window envelope continued (no zero tail);
* ``push_features(..., scale="torch")`` / ``flush_features`` return, frame by frame, ``TorchGate.gated_filterbank(x, fb, power,
  log, eps)`` of the whole signal, and ``return_mask=True`` the mask above (``scale="scipy"``: ``ValueError``);
* output, mask and features are bitwise independent of the block split, the slot, the other streams and the kind of the
  earlier steps; ``precision="float64"`` works as for the non-stationary bank (float64 mask rows, all four sample types).

Such a bank takes no noise profile, no ``lookahead_ms`` and none of the scipy gate's ``time_constant_s`` /
``thresh_n_mult_nonstationary`` / ``sigmoid_slope_nonstationary``; ``snapshot`` / ``restore`` (a state header of kind 1 could
not tell the two non-stationary gates apart, and its format is pinned) and ``push_spectrum`` (it would have to take
``torch.stft``'s phase and scale) raise ``ValueError`` before any device work.

Out of scope: spectrum-only steps that skip the inverse transform, gradients through a stream, ``TorchGate``'s stationary gate
(its statistics need ``xn`` or the whole recording) and ``push_spectrum`` / snapshots of its non-stationary one, collectives
between GPUs (a state's bytes are the transport), and ``n_fft`` other than a power of two from 256 to 4096 (``ValueError``).
"""
import ctypes

import numpy as np
import torch

from noisereduce_amd import _ffi
from noisereduce_amd.torchgate.filterbank import check_filterbank

_NONE_CHUNK = 1 << 62
_N_FFTS = (256, 512, 1024, 2048, 4096)
_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
_EXACT_TYPES = _FLOATS + (np.dtype(np.int16), np.dtype(np.int32))      # what a precision="float64" bank takes
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int16): torch.int16,
          np.dtype(np.int32): torch.int32}
MAX_STATE_BYTES = 32 << 30      # default bound on a bank's device state (``max_state_bytes=``)
MAX_LOOKAHEAD_FRAMES = 4096     # SG_STREAM_MAX_LOOKAHEAD (include/mi355gate.h)


def t_decided(n, W, H):
    """Last frame that lies inside the first ``n`` samples (-1: none)."""
    a = n + W // 2 - W
    return -1 if a < 0 else a // H


def emitted(n, W, H, nt):
    """Samples a stream has emitted after receiving ``n`` (host arithmetic; no GPU)."""
    return max(0, (t_decided(n, W, H) - nt + 1) * H - W // 2)


def frames_applied(n, W, H, lag):
    """Frames a stream has applied -- gated, inverted and, in a spectrum step, reported -- after receiving ``n`` samples:
    ``A(n) = max(0, t_dec(n) - lag + 1)``, ``lag`` = nt + lookahead_frames (host arithmetic; no GPU).  ``emitted(n, W, H,
    lag) == max(0, A(n) * H - W // 2)``."""
    return max(0, t_decided(n, W, H) - lag + 1)


def iir_coefficient(time_constant_s, sr, H):
    """One-pole coefficient of the reference's get_time_smoothed_representation."""
    t_frames = time_constant_s * sr / float(H)
    return (np.sqrt(1 + 4 * t_frames ** 2) - 1) / (2 * t_frames ** 2)


def box_frames(K):
    """``(lo, L)`` of TorchGate's moving mean over ``K`` frames, frames ``t - lo .. t + L`` (``conv1d(padding="same")``
    puts the shorter half of an even ``K`` behind the frame)."""
    lo = (K - 1) // 2
    return lo, K - 1 - lo


def state_bytes(n_units, n_fft, W, H, nt, L, max_block, stationary, noise_from_stream=False, exact=False, movemean=0):
    """Device memory a bank holds between steps (sg_stream_state_bytes_ex's arithmetic; DESIGN section 13's state table).
    ``noise_from_stream``: the three float64 rows of noise statistics per unit of an adaptive bank.  ``exact``: the
    sigmoid rows of a non-stationary bank at 8 bytes (nothing else of the state differs).  ``movemean``: ``K`` of an
    ``algorithm="torchgate"`` bank (``stationary=False``; ``L`` must be ``box_frames(K)[1]``): its ``|X|`` rows reach
    ``(K - 1) // 2`` frames further back, and it keeps neither a forward level nor the forward rows."""
    F = n_fft // 2 + 1
    FS = (F + 15) // 16 * 16
    mf = (max_block + W // 2) // H + 3
    per = (W + (nt + L + 1) * H) * 8 + 2 * W * 8
    RB = 2 * nt + 1 + L + mf
    if stationary:
        per += FS * 8 + RB * ((F + 63) // 64) * 8
    elif movemean:
        per += (L + box_frames(movemean)[0] + 1 + mf) * FS * 8 + RB * FS * (8 if exact else 4)
    else:
        per += FS * 8 + (L + 1 + mf) * 2 * FS * 8 + RB * FS * (8 if exact else 4)
    if noise_from_stream:
        per += 3 * FS * 8
    return n_units * per


def state_payload_bytes(n, n_fft, W, H, nt, L, channels, kind, exact=False):
    """Bytes of one slot's ``StreamState`` payload after ``n`` samples (sg_stream_export_bytes' arithmetic; DESIGN section
    13d's layout table).  ``kind``: "fixed", "nonstationary" or "adaptive"; ``nt``: 0 with the smoothing off.  Does not
    depend on ``max_block``: the payload holds the live rows in index order, not the bank's rings."""
    F = n_fft // 2 + 1
    FS = (F + 15) // 16 * 16
    wpr = (F + 63) // 64
    L = L if kind == "nonstationary" else 0
    RC = W + (nt + L + 1) * H
    td = t_decided(n, W, H)
    ts = max(-1, td - L)
    ta = max(-1, ts - nt)
    E = max(0, (ta + 1) * H - W // 2)
    words = min(n, RC)                                                  # ring: samples [max(0, n - RC), n)
    words += max(0, ta * H - W // 2 + W - E) if ta >= 0 else 0          # the live carry: [E, ta H - h + W)
    row_lo = max(0, ta + 1 - nt)
    if kind == "nonstationary":
        words += FS                                                     # fst
        words += (td - ts) * 2 * FS                                     # fa: frames (ts, td]
        words += (ts - row_lo + 1) * (FS if exact else FS // 2)         # mk: frames [row_lo, ts]
    else:
        words += FS + (td - row_lo + 1) * wpr                           # rmax; bits: frames [row_lo, td]
    if kind == "adaptive":
        words += 3 * FS                                                 # nst
    return 8 * ((2 * FS if kind == "fixed" else 0) + channels * words)  # thr, T2 once per slot


_KINDS = ("fixed", "nonstationary", "adaptive")      # SG_STREAM_FIXED / _NONSTATIONARY / _ADAPTIVE
_DTYPE_CODES = (np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int16), np.dtype(np.int32))   # SG_F32 ...
_HEAD_BYTES = ctypes.sizeof(_ffi.SgStreamHead)


class StreamState:
    """One stream's state as ``StreamBank.snapshot`` took it: a header (``head``, an ``_ffi.SgStreamHead``: format version,
    the signature a bank must share to take it, the stream's counters, what kind of block it was last fed with) and the
    payload (``payload``, a uint8 tensor: a view into the snapshot's one device buffer, or host memory for a state built
    ``from_bytes``).  ``received`` / ``emitted``: the stream's samples in and out so far."""

    def __init__(self, head, payload):
        self.head, self.payload = head, payload
        self.received, self.emitted = int(head.n), int(head.E)

    def to_bytes(self):
        """Header + payload as self-contained bytes (synchronises and copies to the host)."""
        return bytes(self.head) + self.payload.detach().cpu().numpy().tobytes()

    @classmethod
    def from_bytes(cls, blob):
        blob = bytes(blob)
        if len(blob) < _HEAD_BYTES:
            raise ValueError(f"StreamState: {len(blob)} bytes are fewer than a header ({_HEAD_BYTES})")
        head = _ffi.SgStreamHead.from_buffer_copy(blob[:_HEAD_BYTES])
        if head.magic != _ffi.SG_STREAM_HEAD_MAGIC:
            raise ValueError(f"StreamState: not a stream state (magic {head.magic & 0xffffffff:#x})")
        if head.version != _ffi.SG_STREAM_HEAD_VERSION:
            raise ValueError(f"StreamState: format version {head.version} (this library reads "
                             f"{_ffi.SG_STREAM_HEAD_VERSION})")
        if head.payload_bytes < 0 or len(blob) != _HEAD_BYTES + head.payload_bytes:
            raise ValueError(f"StreamState: {len(blob)} bytes, the header announces {_HEAD_BYTES} + {head.payload_bytes}")
        payload = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8, offset=_HEAD_BYTES).copy())
        return cls(head, payload)


class _Default:
    """A default that can be told from the same value given explicitly (it shows as the value in a signature)."""

    def __init__(self, value):
        self.value = value

    def __repr__(self):
        return repr(self.value)


def _widths(sr, n_fft, H, freq_mask_smooth_hz, time_mask_smooth_ms):
    """(n_grad_freq, n_grad_time, smooth) with the reference's errors (SpectralGate._generate_mask_smoothing_filter)."""
    if freq_mask_smooth_hz is None and time_mask_smooth_ms is None:
        return 1, 1, False
    nf = nt = 1
    if freq_mask_smooth_hz is not None:
        nf = int(freq_mask_smooth_hz / (sr / (n_fft / 2)))
        if nf < 1:
            raise ValueError("freq_mask_smooth_hz needs to be at least {}Hz".format(int((sr / (n_fft / 2)))))
    if time_mask_smooth_ms is not None:
        nt = int(time_mask_smooth_ms / ((H / sr) * 1000))
        if nt < 1:
            raise ValueError("time_mask_smooth_ms needs to be at least {}ms".format(int((H / sr) * 1000)))
    return nf, nt, not (nf == 1 and nt == 1)


class StreamBank:
    """``n_streams`` live streams of ``channels`` channels each, gated with the stationary gate or, ``stationary=False``,
    the non-stationary one with ``lookahead_ms`` of lookahead (module docstring; no noise profile then, and
    ``time_constant_s``, ``thresh_n_mult_nonstationary``, ``sigmoid_slope_nonstationary`` as ``reduce_noise``).  ``algorithm="torchgate", stationary=False`` streams ``TorchGate``'s non-stationary gate instead,
    exactly (``n_movemean_nonstationary``, ``n_thresh_nonstationary``, ``temp_coeff_nonstationary`` as ``TorchGate``;
    ``from_torchgate`` reads them from a module; module docstring for what such a bank refuses).

    The noise profile is fixed per stream: ``y_noise`` (a noise clip, ``(n,)`` or ``(C, n)``; channel mean, whole clip,
    the float64 statistics ``reduce_noise`` uses) or ``thresholds_db`` (``n_fft // 2 + 1`` dB values) sets it for every
    slot; ``set_noise(slots, ...)`` overrides it per stream.  ``max_block`` is the longest block a step may push to one
    stream (default: one second).

    ``push({slot: block})`` -> ``{slot: out}``: blocks are ``(n,)`` or ``(C, n)`` float32 / float64 numpy arrays or
    device tensors (``precision="float64"``: int16 / int32 too, every slot gets its block's type back, each sample the
    float64 result at that type -- module docstring); device tensors in give device tensors out with no host synchronisation (output lengths are host
    arithmetic); numpy in gives numpy out.  ``flush(slots)`` -> ``{slot: tail}`` ends streams (fewer than ``win_length``
    samples in all: ``ValueError``) and leaves the slots empty; ``reset(slots)`` drops their state.

    ``push_spectrum(blocks, return_mask=False)`` / ``flush_spectrum(slots, blocks=None, return_mask=False)`` are the same
    steps -- bitwise the same samples, the same four launches -- that also report the gated spectrogram of the newly applied
    frames: ``{slot: (samples, Y)}`` or ``{slot: (samples, Y, mask)}``, ``Y`` ``(F, k)`` complex for a flat mono stream and
    ``(C, F, k)`` otherwise, ``k = frames(slot)`` after minus before (possibly 0), the bins contiguous in memory
    (``torch.stft``'s layout).  Each frame is the offline ``Z * mask`` of the whole signal (``scipy.signal.stft``'s scaling,
    ``padding=0``; the causal floor and the lookahead as for the audio), ``scipy.signal.istft`` of the concatenated frames is
    the concatenated audio, and ``Y`` / ``mask`` are bitwise independent of the block split, the slot, the other streams and
    of whether earlier steps were ``push`` or ``push_spectrum`` (module docstring: the contract).

    ``noise_from_stream=True`` takes no profile: every (stream, channel) learns its own from the frames it has seen, a
    running mean and standard deviation of the floored dB values per band (the recurrence in the module docstring),
    cumulative or, ``noise_memory_s``, forgetting exponentially with that time constant, and held after ``noise_learn_s``
    seconds if given (a ``noise_memory_s`` of less than about three hops gates everything: module docstring).  The
    statistics are per channel (the reference thresholds on the channel mean; the same for
    ``channels=1``).  ``noise_profile(slot)`` reads the current threshold; ``set_noise`` and ``thresholds`` raise."""

    def __init__(self, sr, n_streams, channels=1, y_noise=None, thresholds_db=None, prop_decrease=1.0,
                 n_std_thresh_stationary=1.5, freq_mask_smooth_hz=500, time_mask_smooth_ms=50, n_fft=1024,
                 win_length=None, hop_length=None, max_block=None, device="cuda", stationary=True, lookahead_ms=0.0,
                 time_constant_s=_Default(2.0), thresh_n_mult_nonstationary=_Default(2),
                 sigmoid_slope_nonstationary=_Default(10),
                 max_state_bytes=MAX_STATE_BYTES, noise_from_stream=False, noise_memory_s=None, noise_learn_s=None,
                 precision=None, algorithm="scipy", n_movemean_nonstationary=20, n_thresh_nonstationary=1.3,
                 temp_coeff_nonstationary=0.1):
        if precision not in (None, "float32", "float64"):
            raise ValueError(f"StreamBank: precision must be None, 'float32' or 'float64' (got {precision!r})")
        self.exact = precision == "float64"
        if algorithm not in ("scipy", "torchgate"):
            raise ValueError(f"StreamBank: algorithm must be 'scipy' or 'torchgate' (got {algorithm!r})")
        self.algorithm = algorithm
        stationary = bool(stationary)
        noise_from_stream = bool(noise_from_stream)
        # (the scipy gate's parameters: given explicitly they are an error for algorithm="torchgate", which has its own)
        scipy_only = dict(time_constant_s=time_constant_s, thresh_n_mult_nonstationary=thresh_n_mult_nonstationary,
                          sigmoid_slope_nonstationary=sigmoid_slope_nonstationary)
        time_constant_s, thresh_n_mult_nonstationary, sigmoid_slope_nonstationary = (
            v.value if isinstance(v, _Default) else v for v in scipy_only.values())
        self.movemean = 0
        if algorithm == "torchgate":
            if stationary:
                raise ValueError("StreamBank: algorithm='torchgate' streams TorchGate's non-stationary gate: pass "
                                 "stationary=False (its stationary gate needs the whole recording's statistics or xn)")
            if y_noise is not None or thresholds_db is not None or noise_from_stream:
                raise ValueError("StreamBank: algorithm='torchgate' takes no noise profile (y_noise / thresholds_db / "
                                 "noise_from_stream)")
            if lookahead_ms:
                raise ValueError("StreamBank: algorithm='torchgate' takes no lookahead_ms: n_movemean_nonstationary decides "
                                 "the lookahead, K - 1 - (K - 1) // 2 frames")
            given = [k for k, v in scipy_only.items() if not isinstance(v, _Default)]
            if given:
                raise ValueError(f"StreamBank: {', '.join(given)} belong to algorithm='scipy' (TorchGate's gate takes "
                                 f"n_movemean_nonstationary, n_thresh_nonstationary, temp_coeff_nonstationary)")
            if isinstance(n_movemean_nonstationary, bool) or int(n_movemean_nonstationary) != n_movemean_nonstationary or \
                    not 1 <= n_movemean_nonstationary <= MAX_LOOKAHEAD_FRAMES:
                raise ValueError(f"StreamBank: n_movemean_nonstationary must be an integer from 1 to {MAX_LOOKAHEAD_FRAMES} "
                                 f"(got {n_movemean_nonstationary!r})")
            if not temp_coeff_nonstationary > 0:
                raise ValueError("StreamBank: temp_coeff_nonstationary must be positive")
            if win_length is not None and int(win_length) % 2:
                raise ValueError(f"StreamBank: algorithm='torchgate' needs an even win_length (got {win_length}): the "
                                 f"stream's frames would not be the samples torch.stft windows")
            self.movemean = int(n_movemean_nonstationary)
        elif (n_movemean_nonstationary, n_thresh_nonstationary, temp_coeff_nonstationary) != (20, 1.3, 0.1):
            raise ValueError("StreamBank: n_movemean_nonstationary, n_thresh_nonstationary and temp_coeff_nonstationary "
                             "belong to algorithm='torchgate'")
        if noise_from_stream and (y_noise is not None or thresholds_db is not None):
            raise ValueError("StreamBank: noise_from_stream learns the profile; give no y_noise / thresholds_db with it")
        if noise_from_stream and not stationary:
            raise ValueError("StreamBank: noise_from_stream belongs to the stationary gate (stationary=True)")
        if not noise_from_stream and (noise_memory_s is not None or noise_learn_s is not None):
            raise ValueError("StreamBank: noise_memory_s / noise_learn_s need noise_from_stream=True")
        if noise_memory_s is not None and not (np.isfinite(noise_memory_s) and noise_memory_s > 0):
            raise ValueError(f"StreamBank: noise_memory_s must be finite and positive (got {noise_memory_s!r})")
        if noise_learn_s is not None and not (np.isfinite(noise_learn_s) and noise_learn_s > 0):
            raise ValueError(f"StreamBank: noise_learn_s must be finite and positive (got {noise_learn_s!r})")
        if not stationary and (y_noise is not None or thresholds_db is not None):
            raise ValueError("StreamBank: the non-stationary gate takes no noise profile (y_noise / thresholds_db)")
        if stationary and lookahead_ms:
            raise ValueError("StreamBank: lookahead_ms belongs to the non-stationary gate (stationary=False)")
        if not (lookahead_ms >= 0 and np.isfinite(lookahead_ms)):
            raise ValueError("StreamBank: lookahead_ms must be finite and at least 0")
        if not stationary and not time_constant_s > 0:
            raise ValueError("StreamBank: time_constant_s must be positive")
        n_fft = int(n_fft)
        if n_fft not in _N_FFTS:
            raise ValueError("StreamBank: n_fft must be a power of two from 256 to 4096")
        W = n_fft if win_length is None else int(win_length)
        H = W // 4 if hop_length is None else int(hop_length)
        if W > n_fft or W < 2 or H < 1:
            raise ValueError("StreamBank: needs 2 <= win_length <= n_fft and hop_length >= 1")
        if int(n_streams) < 1 or int(channels) < 1:
            raise ValueError("StreamBank: n_streams and channels must be at least 1")
        if y_noise is not None and thresholds_db is not None:
            raise ValueError("StreamBank: give y_noise or thresholds_db, not both")
        nf, nt, smooth = _widths(sr, n_fft, H, freq_mask_smooth_hz, time_mask_smooth_ms)
        self.sr, self.n_fft, self.win_length, self.hop_length = sr, n_fft, W, H
        self.n_streams, self.channels = int(n_streams), int(channels)
        self.nt = nt if smooth else 0
        self.max_block = int(sr) if max_block is None else int(max_block)
        if self.max_block < 1:
            raise ValueError("StreamBank: max_block must be at least 1")
        self.stationary = stationary
        self.noise_from_stream = noise_from_stream
        self.noise_forget, self.noise_learn_frames = 1.0, -1      # lam per frame; frames that learn (-1: all)
        if noise_memory_s is not None:
            self.noise_forget = float(np.exp(-H / (sr * float(noise_memory_s))))
            if not self.noise_forget > 0.0:
                raise ValueError(f"StreamBank: noise_memory_s={noise_memory_s!r} is too short against one hop "
                                 f"({H / sr:g} s): the forgetting factor underflows")
        if noise_learn_s is not None:
            self.noise_learn_frames = int(noise_learn_s * sr / H)
            if self.noise_learn_frames < 1:
                raise ValueError(f"StreamBank: noise_learn_s={noise_learn_s!r} is shorter than one hop ({H / sr:g} s)")
        self.lookahead_frames = 0 if stationary else int(lookahead_ms / ((H / sr) * 1000))
        if self.movemean:      # the part of the moving mean ahead of the frame
            self.lookahead_frames = box_frames(self.movemean)[1]
        self._lag = self.nt + self.lookahead_frames      # frames between the last one inside the audio and the last applied
        self.latency_samples = W + (self._lag + 1) * H
        self.state_bytes = state_bytes(self.n_streams * self.channels, n_fft, W, H, self.nt, self.lookahead_frames,
                                       self.max_block, stationary, noise_from_stream, self.exact, self.movemean)
        if not stationary and self.state_bytes > max_state_bytes:
            raise ValueError(f"StreamBank: {self.n_streams} x {self.channels} streams with lookahead_frames="
                             f"{self.lookahead_frames} and max_block={self.max_block} need {self.state_bytes} bytes of "
                             f"device state (max_state_bytes={max_state_bytes})")
        if self.lookahead_frames > MAX_LOOKAHEAD_FRAMES:
            raise ValueError(f"StreamBank: lookahead_ms={lookahead_ms} is {self.lookahead_frames} frames; at most "
                             f"{MAX_LOOKAHEAD_FRAMES} (the backward pass of a frame is that many dependent steps per band)")
        self._n = [0] * self.n_streams        # samples received / emitted per slot (mirrors of the library's counters)
        self._e = [0] * self.n_streams
        self._has_noise = [not stationary or noise_from_stream] * self.n_streams
        self._kind = [(False, np.dtype(np.float32), True)] * self.n_streams   # (tensor I/O, dtype, flat) of the last block
        self._bank = self._gate = None
        self._pending = []                    # noise profiles set before the first device call
        self._fb = None                       # the filterbank (set_filterbank): (F, M) float32, validated
        self._fb_pending = False              # ... set before the first device call: uploaded by _ensure
        self._device_arg = device
        self._gate_kw = dict(variant=_ffi.SG_VARIANT_S, stationary=stationary, n_fft=n_fft, win_length=W, hop_length=H,
                             n_grad_freq=nf if smooth else 1, n_grad_time=nt if smooth else 1, smooth_mask=smooth,
                             chunk_size=_NONE_CHUNK, padding=0, prop_decrease=prop_decrease,
                             n_std_thresh=n_std_thresh_stationary, top_db=80.0, ddof=0)
        if self.movemean:      # the handle TorchGate._gate_for makes: variant T, the float32 Hann table, 1 / temp as slope
            self._gate_kw = dict(variant=_ffi.SG_VARIANT_T, stationary=False, n_fft=n_fft, win_length=W, hop_length=H,
                                 n_grad_freq=nf if smooth else 1, n_grad_time=nt if smooth else 1, smooth_mask=smooth,
                                 prop_decrease=prop_decrease, n_std_thresh=n_std_thresh_stationary, top_db=40.0, ddof=1,
                                 n_movemean=self.movemean, nonstat_thresh=n_thresh_nonstationary,
                                 nonstat_slope=1.0 / temp_coeff_nonstationary,
                                 window=torch.hann_window(W).double().numpy())
        elif not stationary:
            self._gate_kw.update(iir_b=float(iir_coefficient(time_constant_s, sr, H)),
                                 nonstat_thresh=thresh_n_mult_nonstationary, nonstat_slope=sigmoid_slope_nonstationary)
        if y_noise is not None or thresholds_db is not None:
            self.set_noise(range(self.n_streams), y_noise=y_noise, thresholds_db=thresholds_db)

    @classmethod
    def from_torchgate(cls, tg, n_streams, channels=1, max_block=None, precision=None, device="cuda"):
        """The bank that streams ``tg``, a ``TorchGate(nonstationary=True)`` module: every gate parameter is read from the
        module (a stationary one: ``ValueError``).  The concatenated output of a stream is ``tg(x[None])[0]``."""
        if not getattr(tg, "nonstationary", False):
            raise ValueError("StreamBank.from_torchgate: the module is stationary; only TorchGate(nonstationary=True) "
                             "can be streamed")
        return cls(tg.sr, n_streams, channels=channels, max_block=max_block, precision=precision, device=device,
                   algorithm="torchgate", stationary=False, prop_decrease=tg.prop_decrease, n_fft=tg.n_fft,
                   win_length=tg.win_length, hop_length=tg.hop_length, freq_mask_smooth_hz=tg.freq_mask_smooth_hz,
                   time_mask_smooth_ms=tg.time_mask_smooth_ms, n_movemean_nonstationary=tg.n_movemean_nonstationary,
                   n_thresh_nonstationary=tg.n_thresh_nonstationary, temp_coeff_nonstationary=tg.temp_coeff_nonstationary)

    def _ensure(self):
        """The engine handle and the bank's device state, created at the first call that needs the GPU (arguments are
        checked before that); then the noise profiles set so far."""
        if self._bank is None:
            self._gate = _ffi.Gate(self._device_arg, **self._gate_kw)
            self.device = self._gate.device
            if self.movemean:      # (the handle's n_movemean decides the lookahead: the descriptor's stays 0)
                self._bank = self._gate.stream_create_ex(_ffi.Gate.stream_desc(
                    self.n_streams, self.channels, self.max_block, _ffi.SG_STREAM_NONSTATIONARY, 0, exact=self.exact))
            elif self.exact:
                kind = (_ffi.SG_STREAM_ADAPTIVE if self.noise_from_stream else
                        _ffi.SG_STREAM_FIXED if self.stationary else _ffi.SG_STREAM_NONSTATIONARY)
                self._bank = self._gate.stream_create_ex(_ffi.Gate.stream_desc(
                    self.n_streams, self.channels, self.max_block, kind, self.lookahead_frames, self.noise_forget,
                    self.noise_learn_frames, exact=True))
            elif self.noise_from_stream:
                self._bank = self._gate.stream_create_adaptive(self.n_streams, self.channels, self.max_block,
                                                               self.noise_forget, self.noise_learn_frames)
            elif self.stationary:
                self._bank = self._gate.stream_create(self.n_streams, self.channels, self.max_block)
            else:
                self._bank = self._gate.stream_create_nonstationary(self.n_streams, self.channels, self.max_block,
                                                                    self.lookahead_frames)
        if self._fb_pending:
            self._fb_pending = False
            self._gate.stream_set_filterbank(self._bank, self._fb)
        pending, self._pending = self._pending, []
        for slots, kind, val in pending:
            if kind == "db":
                self._gate.stream_set_threshold(self._bank, slots, val)
            else:
                with torch.cuda.device(self.device):
                    self._gate.noise_stats(val.to(self.device, torch.float64))
                    self._gate.stream_set_threshold(self._bank, slots, None)

    # -- plumbing ----------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_bank", None) is not None:
            self._gate.stream_destroy(self._bank)
            self._bank = None
            self._gate.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _slots(self, slots):
        out = [slots] if isinstance(slots, (int, np.integer)) else list(slots)
        for s in out:
            if not isinstance(s, (int, np.integer)) or s < 0 or s >= self.n_streams:
                raise ValueError(f"StreamBank: unknown slot {s!r} (the bank has {self.n_streams})")
        return [int(s) for s in out]

    @property
    def gate(self):
        """The engine handle (per-kernel timing: ``gate.profile_enable()`` / ``profile_read()``)."""
        self._ensure()
        return self._gate

    def received(self, slot):
        return self._n[self._slots(slot)[0]]

    def thresholds(self):
        """The dB threshold the handle computed last (``set_noise(..., y_noise=)``), as a numpy array (synchronises)."""
        if not self.stationary:
            raise ValueError("StreamBank: the non-stationary gate has no thresholds")
        if self.noise_from_stream:
            raise ValueError("StreamBank: a noise_from_stream bank computes no threshold on the handle; "
                             "noise_profile(slot) reads the one a stream has learnt")
        return self.gate.get_noise_threshold()

    def noise_profile(self, slot):
        """``noise_from_stream`` banks: the dB threshold of every band after the last frame decided on ``slot``, a
        ``(channels, n_fft // 2 + 1)`` float64 numpy array; NaN before the first frame.  Synchronises."""
        if not self.noise_from_stream:
            raise ValueError("StreamBank: noise_profile belongs to noise_from_stream=True (thresholds() otherwise)")
        s = self._slots(slot)[0]
        self._ensure()
        return self._gate.stream_noise_profile(self._bank, s, self.channels)

    # -- noise profile -----------------------------------------------------------------------------------------
    def set_noise(self, slots, y_noise=None, thresholds_db=None):
        if not self.stationary:
            raise ValueError("set_noise: the non-stationary gate takes no noise profile")
        if self.noise_from_stream:
            raise ValueError("set_noise: a noise_from_stream bank learns its profile from the stream")
        slots = self._slots(slots)
        if (y_noise is None) == (thresholds_db is None):
            raise ValueError("set_noise: give y_noise or thresholds_db")
        if thresholds_db is not None:
            t = np.asarray(thresholds_db, dtype=np.float64).reshape(-1)
            if t.shape[0] != self.n_fft // 2 + 1:
                raise ValueError(f"thresholds_db must hold n_fft // 2 + 1 = {self.n_fft // 2 + 1} values")
            self._pending.append((slots, "db", t))
        else:
            a = y_noise.detach() if isinstance(y_noise, torch.Tensor) else np.asarray(y_noise)
            if a.ndim == 1:
                a = a[None, :]
            if a.ndim != 2:
                raise ValueError("noise waveform must be in shape (# frames, # channels)")
            if a.shape[1] < self.win_length:
                raise ValueError(f"noise clip of {a.shape[1]} samples is shorter than win_length={self.win_length}")
            if not isinstance(a, torch.Tensor):
                a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
            self._pending.append((slots, "clip", a))
        for s in slots:
            self._has_noise[s] = True
        if self._bank is not None:
            self._ensure()

    # -- filterbank --------------------------------------------------------------------------------------------
    def set_filterbank(self, fb):
        """The bank's filterbank for ``push_features`` / ``flush_features``: any real ``(n_fft // 2 + 1, M)`` array or tensor,
        ``1 <= M <= 1024``, finite entries (negative ones are fine for ``log=False``); a constant, validated with
        ``torchgate.filterbank.check_filterbank`` (``ValueError``; the bank then keeps the filterbank it had).
        ``noisereduce_amd.torchgate.mel_filterbank(sr, n_fft, n_mels)`` is the common case.  Before the first device call it
        is kept pending, like ``set_noise``; replacing a filterbank synchronises the device.  The filterbank belongs to the
        bank, not to a stream: ``snapshot`` / ``restore`` do not carry it, and a moved stream continues its features where
        the destination bank holds the same filterbank."""
        a = check_filterbank(fb, self.n_fft // 2 + 1)
        if self._bank is not None:
            self._gate.stream_set_filterbank(self._bank, a)      # (raises before self._fb changes)
            self._fb, self._fb_pending = a, False
        else:
            self._fb, self._fb_pending = a, True

    def _feature_args(self, power, log, eps, scale):
        """(power, log, eps, the C ABI's scale) of a feature step, or ValueError -- before any device work."""
        if isinstance(power, bool) or power not in (1, 2):
            raise ValueError(f"StreamBank: power must be 1 or 2 (got {power!r})")
        eps = float(eps)
        if eps != eps:
            raise ValueError("StreamBank: eps is NaN")
        if scale not in ("scipy", "torch"):
            raise ValueError(f"StreamBank: scale must be 'scipy' or 'torch' (got {scale!r})")
        if self.movemean and scale != "torch":
            raise ValueError("StreamBank: an algorithm='torchgate' bank has torch.stft's unscaled transform only: pass "
                             "scale='torch'")
        if self._fb is None:
            raise ValueError("StreamBank: no filterbank set (set_filterbank)")
        # (0.0: the bank's own 1 / sum(window), the very factor push_spectrum applies; 1.0: the unscaled transform)
        return int(power), bool(log), eps, 0.0 if scale == "scipy" else 1.0

    # -- steps -------------------------------------------------------------------------------------------------
    def _step(self, blocks, flush, spectrum=False, return_mask=False, features=None):
        """blocks: {slot: block or None}; every argument is checked before any device work.  ``spectrum``: a spectrum
        step (sg_stream_push_spectrum), every result a tuple (samples, Y[, mask]).  ``features``: ``_feature_args``'
        result, a feature step (sg_stream_push_features), every result a tuple (samples, feat[, mask])."""
        C, W = self.channels, self.win_length
        items, tensor_io = [], None
        for s, blk in blocks.items():
            s = self._slots(s)[0]
            if not self._has_noise[s]:
                raise ValueError(f"StreamBank: slot {s} has no noise profile (y_noise / thresholds_db / set_noise)")
            if blk is None:
                items.append((s, None, 0, self._kind[s][2]))
                continue
            is_t = isinstance(blk, torch.Tensor)
            a = blk.detach() if is_t else np.asarray(blk)
            if tensor_io is None:
                tensor_io = is_t
            elif tensor_io != is_t:
                raise ValueError("StreamBank: the blocks of a step must be all numpy arrays or all device tensors")
            dt = np.dtype(str(a.dtype).replace("torch.", ""))
            if self.exact and dt not in _EXACT_TYPES:
                raise ValueError(f"StreamBank: blocks are float32, float64, int16 or int32 (got {dt})")
            if not self.exact and dt not in _FLOATS:
                raise ValueError(f"StreamBank: blocks are float32 or float64 (got {dt}; precision=\"float64\" takes "
                                 f"int16 / int32 blocks too)")
            if is_t and a.device.type != "cuda":
                raise ValueError("StreamBank: block tensors must live on the GPU")
            flat = a.ndim == 1
            if a.ndim not in (1, 2) or (flat and C != 1) or (not flat and a.shape[0] != C):
                raise ValueError(f"StreamBank: slot {s}: a block is (n,) or ({C}, n), got {tuple(a.shape)}")
            n = int(a.shape[-1])
            if n > self.max_block:
                raise ValueError(f"StreamBank: slot {s}: block of {n} samples is longer than max_block={self.max_block}")
            items.append((s, a, n, flat))
        if len({it[0] for it in items}) != len(items):
            raise ValueError("StreamBank: a slot appears twice in one step")
        if flush:
            for s, a, n, flat in items:
                if self._n[s] + n < W:
                    raise ValueError(f"StreamBank: slot {s}: a stream of {self._n[s] + n} samples is shorter than "
                                     f"win_length={W}")
        if tensor_io is None:      # a flush without a last block: what the streams were fed with
            tensor_io = bool(items) and all(self._kind[s][0] for s, _, _, _ in items)
        self._ensure()
        if self.exact:      # one sample type: the step travels in it; several: in float64, which holds every one exactly
            kinds = {np.dtype(str(a.dtype).replace("torch.", "")) if a is not None else self._kind[s][1]
                     for s, a, _, _ in items}
            travel = kinds.pop() if len(kinds) == 1 else np.dtype(np.float64)
        else:
            wide = any(a is not None and str(a.dtype).endswith("float64") for _, a, _, _ in items)
            travel = np.dtype(np.float64 if wide else np.float32)
        tdt = _TORCH[travel]
        recs, outs, in_off, out_off = [], [], 0, 0
        srecs, frames, sp_off = [], [], 0      # spectrum steps: where every record's newly applied frames go
        ft_off = 0                             # feature steps: the feature rows (M wide) next to the mask rows (F wide)
        F, H = self.n_fft // 2 + 1, self.hop_length
        M = self._fb.shape[1] if features else 0
        for s, a, n, flat in items:
            n1 = self._n[s] + n
            k = (n1 if flush else emitted(n1, W, self.hop_length, self._lag)) - self._e[s]
            recs.append(_ffi.SgStreamRec(slot=s, flush=int(flush), n_samples=n, in_offset=in_off, in_stride=n,
                                         out_offset=out_off, out_stride=k))
            outs.append((s, a, k, flat, out_off))
            in_off += C * n
            out_off += C * k
            if spectrum or features:
                kf = ((n1 + 2 * (W // 2) - W) // H + 1 if flush else frames_applied(n1, W, H, self._lag)) - \
                    frames_applied(self._n[s], W, H, self._lag)
                if features:
                    srecs.append(_ffi.SgStreamFeatRec(feat_offset=ft_off, feat_stride=kf * M, mask_offset=sp_off,
                                                      mask_stride=kf * F))
                else:
                    srecs.append(_ffi.SgStreamSpecRec(spec_offset=sp_off, mask_offset=sp_off, stride=kf * F))
                frames.append((kf, sp_off, ft_off))
                sp_off += C * kf * F
                ft_off += C * kf * M
        if spectrum or features:      # complex64 where every slot's own block is float32; else complex128, a float32 slot rounded once
            own = [np.dtype(str(a.dtype).replace("torch.", "")) if a is not None else self._kind[s][1] for s, a, _, _ in items]
            narrow = all(dt == np.dtype(np.float32) for dt in own)
            cdt, rdt = (torch.complex64, torch.float32) if narrow else (torch.complex128, torch.float64)
        with torch.cuda.device(self.device):
            parts = [a.reshape(-1) for _, a, n, _ in items if a is not None and n > 0]
            if tensor_io:
                x = torch.cat([p.to(tdt) for p in parts]) if parts else torch.empty(0, dtype=tdt, device=self.device)
            else:
                xh = torch.empty(max(in_off, 1), dtype=tdt, pin_memory=True)
                if parts:
                    xh.numpy()[:in_off] = np.concatenate([p.astype(travel, copy=False) for p in parts])
                x = xh.to(self.device, non_blocking=True)
            if x.numel() == 0:
                x = torch.empty(1, dtype=tdt, device=self.device)
            out = torch.empty(max(out_off, 1), dtype=tdt, device=self.device)
            if features:      # (feat is real: float32 where every slot's own block is float32, else float64)
                spec = torch.empty(max(ft_off, 1), dtype=rdt, device=self.device)
                mask = torch.empty(max(sp_off, 1), dtype=rdt, device=self.device) if return_mask else None
                self._gate.stream_push_features(self._bank, x, out, spec, mask, recs, srecs, *features)
            elif spectrum:
                spec = torch.empty(max(sp_off, 1), dtype=cdt, device=self.device)
                mask = torch.empty(max(sp_off, 1), dtype=rdt, device=self.device) if return_mask else None
                self._gate.stream_push_spectrum(self._bank, x, out, spec, mask, recs, srecs)
            else:
                self._gate.stream_push(self._bank, x, out, recs)
            for (s, a, n, flat), (_, _, k, _, _) in zip(items, outs):
                if flush:
                    self._n[s] = self._e[s] = 0
                else:
                    self._n[s] += n
                    self._e[s] += k
            res = {}
            host = None if tensor_io else out.cpu().numpy()
            for s, a, k, flat, off in outs:
                o = (out if tensor_io else host)[off:off + C * k].reshape(C, k)
                if a is not None:
                    dt = a.dtype
                    self._kind[s] = (tensor_io, np.dtype(str(dt).replace("torch.", "")), flat)
                else:
                    dt = self._kind[s][1]
                    if tensor_io:
                        dt = _TORCH[dt]
                if flat and C == 1:
                    o = o[0]
                if self.exact and not (dt.is_floating_point if tensor_io else dt.kind == "f"):
                    # (a mixed step arrives as float64: the kernel's integer store -- NaN -> 0, then truncation)
                    if o.dtype != dt:
                        o = torch.where(o != o, torch.zeros_like(o), o) if tensor_io else np.where(o != o, 0.0, o)
                res[s] = o.to(dt) if tensor_io else o.astype(dt, copy=True)
            if not (spectrum or features):
                return res
            fields = [spec] + ([mask] if return_mask else [])
            if not tensor_io:
                fields = [f.cpu().numpy() for f in fields]
            # (field, width of its rows -- M filters or F bins --, which of a record's two offsets places it)
            cols = [(f, M, 2) if features and i == 0 else (f, F, 1) for i, f in enumerate(fields)]
            for (s, a, k, flat, _), fr, dt in zip(outs, frames, own):
                parts, kf = [], fr[0]
                for f, R, j in cols:      # (C, kf, R) as stored, rows contiguous; handed out as the (C, R, kf) view
                    off = fr[j]
                    if tensor_io and (narrow or dt != np.dtype(np.float32)):      # (one view op per field: a step is host-bound)
                        parts.append(f.as_strided((R, kf), (1, R), off) if flat and C == 1 else
                                     f.as_strided((C, R, kf), (kf * R, 1, R), off))
                        continue
                    v = f[off:off + C * kf * R].reshape(C, kf, R)
                    if dt == np.dtype(np.float32) and not narrow:
                        if tensor_io:
                            v = v.to(torch.complex64 if v.is_complex() else torch.float32)
                        else:
                            v = v.astype(np.complex64 if np.iscomplexobj(v) else np.float32)
                    v = v.transpose(-1, -2) if tensor_io else v.swapaxes(-1, -2)
                    parts.append(v[0] if flat and C == 1 else v)
                res[s] = (res[s],) + tuple(parts)
            return res

    def push(self, blocks):
        """``{slot: block}`` -> ``{slot: newly final samples}`` (possibly empty).  No host synchronisation for device
        tensors.  Device-tensor results are views into one output buffer of the step."""
        return self._step(dict(blocks), flush=False)

    def flush(self, slots, blocks=None):
        """End the streams in ``slots``: ``{slot: remaining samples}``, of the kind and type the streams were last fed with;
        ``blocks`` may give a last block per slot.  The slots are empty and reusable afterwards."""
        slots = self._slots(slots)
        d = {s: None for s in slots}
        if blocks:
            d.update(blocks)
        return self._step(d, flush=True)

    def frames(self, slot):
        """Frames of ``slot``'s stream applied so far: reported by the spectrum steps, or passed in plain ``push`` steps
        (``frames_applied`` of ``received(slot)``; host arithmetic)."""
        return frames_applied(self._n[self._slots(slot)[0]], self.win_length, self.hop_length, self._lag)

    def _not_torchgate(self, what, why):
        """What an ``algorithm="torchgate"`` bank refuses, before any device work."""
        if self.movemean:
            raise ValueError(f"StreamBank: {what} is not available on an algorithm='torchgate' bank ({why})")

    @staticmethod
    def _block_map(blocks, who):
        """{slot: block} of a mapping or of (slot, block) pairs; a slot listed twice is an error."""
        pairs = list(blocks.items() if hasattr(blocks, "items") else blocks)
        d = dict(pairs)
        if len(d) != len(pairs):
            raise ValueError(f"StreamBank: a slot appears twice in one {who}")
        return d

    def push_spectrum(self, blocks, return_mask=False):
        """``push`` that also hands out the gated spectrogram: ``{slot: block}`` (or ``(slot, block)`` pairs) -> ``{slot:
        (samples, Y)}`` or, ``return_mask=True``, ``{slot: (samples, Y, mask)}``.  ``samples`` is exactly what ``push``
        returns.  ``Y`` holds the ``k = frames(slot) after - before`` newly applied frames (possibly 0) of ``Z * mask``, the
        product the step inverts: ``(F, k)`` for a flat mono stream, ``(C, F, k)`` otherwise, ``F = n_fft // 2 + 1``; stored
        ``(..., k, F)`` with the bins contiguous and returned as the transposed view (``torch.stft``'s layout).  complex64
        for a float32 block, complex128 for float64 / int16 / int32, whatever the other streams of the step are; ``mask``
        has ``Y``'s shape and its real type.  Same four launches, no host synchronisation for device tensors."""
        self._not_torchgate("push_spectrum", "the spectrum would need torch.stft's phase and scale")
        return self._step(self._block_map(blocks, "step"), flush=False, spectrum=True, return_mask=bool(return_mask))

    def flush_spectrum(self, slots, blocks=None, return_mask=False):
        """``flush`` that also reports every remaining frame, up to ``T = (N + 2 (W // 2) - W) // H + 1`` of a stream of
        ``N`` samples: ``{slot: (tail, Y[, mask])}``."""
        self._not_torchgate("flush_spectrum", "the spectrum would need torch.stft's phase and scale")
        slots = self._slots(slots)
        if len(set(slots)) != len(slots):
            raise ValueError("StreamBank: a slot appears twice in one flush")
        d = {s: None for s in slots}
        if blocks:
            d.update(self._block_map(blocks, "flush"))
        return self._step(d, flush=True, spectrum=True, return_mask=bool(return_mask))

    def push_features(self, blocks, power=2.0, log=False, eps=1e-10, scale="scipy", return_mask=False):
        """``push`` that also hands out filterbank (log-mel) features of the newly applied frames, reduced on the device
        while each frame is still on chip: ``{slot: block}`` (or ``(slot, block)`` pairs) -> ``{slot: (samples, feat)}`` or,
        ``return_mask=True``, ``{slot: (samples, feat, mask)}``.  ``samples`` is exactly what ``push`` returns and ``mask``
        exactly what ``push_spectrum(return_mask=True)`` returns.  ``feat`` holds the ``k`` newly applied frames
        (``push_spectrum``'s ``k``; ``frames(slot)`` counts them) of

            lin[m, t] = sum_k fb[k, m] * |s * Z[k, t] * mask[k, t]| ** power        feat = ln(lin + eps) if log else lin

        with ``fb`` the bank's filterbank (``set_filterbank``; none set: ``ValueError``) and ``power`` 1 or 2.
        ``scale="scipy"``: ``s = 1 / sum(window)``, the features of exactly the ``Y`` that ``push_spectrum`` returns;
        ``scale="torch"``: ``s = 1``, the unscaled ``torch.stft`` convention of ``TorchGate.gated_filterbank``, so that a
        model trained on offline features can read live ones.  The default ``eps`` is 1e-10, not ``gated_filterbank``'s
        1e-6: under the scipy scaling a full-scale sine has power 0.25 per bin, so 1e-6 would sit above quiet speech.

        ``(M, k)`` for a flat mono stream and ``(C, M, k)`` otherwise; stored ``(..., k, M)`` with the filters contiguous
        and returned as the transposed view, as ``gated_filterbank`` returns its result.  float32 where the slot's own
        block is float32 and float64 otherwise.  Transform, mask, powers and sums are float64, the weights float32 values
        widened; every filter sums in ascending ``k`` over the hull of its non-zero bins and the value is rounded once at
        the store.  Each frame's features are bitwise independent of the block split, the slot, the other streams and of
        whether earlier steps were ``push``, ``push_spectrum`` or ``push_features``; ``snapshot`` / ``restore`` continue
        them where the destination bank holds the same filterbank (the filterbank is not part of a stream's state).  Same
        four launches, no host synchronisation for device tensors."""
        args = self._feature_args(power, log, eps, scale)
        return self._step(self._block_map(blocks, "step"), flush=False, return_mask=bool(return_mask), features=args)

    def flush_features(self, slots, blocks=None, power=2.0, log=False, eps=1e-10, scale="scipy", return_mask=False):
        """``flush`` that also reports the features of every remaining frame, up to ``T = (N + 2 (W // 2) - W) // H + 1`` of
        a stream of ``N`` samples: ``{slot: (tail, feat[, mask])}`` (``push_features``)."""
        args = self._feature_args(power, log, eps, scale)
        slots = self._slots(slots)
        if len(set(slots)) != len(slots):
            raise ValueError("StreamBank: a slot appears twice in one flush")
        d = {s: None for s in slots}
        if blocks:
            d.update(self._block_map(blocks, "flush"))
        return self._step(d, flush=True, return_mask=bool(return_mask), features=args)

    def reset(self, slots):
        slots = self._slots(slots)
        if self._bank is not None:
            self._gate.stream_reset(self._bank, slots)
        for s in slots:
            self._n[s] = self._e[s] = 0

    # -- state transfer ----------------------------------------------------------------------------------------
    def _signature(self):
        """The fields of ``_ffi.STREAM_SIGNATURE`` as this bank has them (what sg_stream_export writes into a header)."""
        kw = self._gate_kw
        kind = 2 if self.noise_from_stream else 0 if self.stationary else 1
        return dict(n_fft=self.n_fft, win_length=self.win_length, hop_length=self.hop_length, channels=self.channels,
                    kind=kind, n_grad_freq=int(kw["n_grad_freq"]), n_grad_time=int(kw["n_grad_time"]),
                    smooth_mask=int(bool(kw["smooth_mask"])), lookahead_frames=self.lookahead_frames, exact=int(self.exact),
                    prop_decrease=float(kw["prop_decrease"]), n_std_thresh=float(kw["n_std_thresh"]),
                    top_db=float(kw["top_db"]), iir_b=float(kw.get("iir_b", 0.0)),
                    nonstat_thresh=float(kw.get("nonstat_thresh", 2.0)), nonstat_slope=float(kw.get("nonstat_slope", 10.0)),
                    noise_forget=float(self.noise_forget), noise_learn_frames=int(self.noise_learn_frames))

    def state_bytes_of(self, slot):
        """Bytes of ``slot``'s state payload right now (host arithmetic from ``received(slot)``)."""
        self._not_torchgate("state_bytes_of", "it has no snapshots")
        return state_payload_bytes(self._n[self._slots(slot)[0]], self.n_fft, self.win_length, self.hop_length, self.nt,
                                   self.lookahead_frames, self.channels, _KINDS[self._signature()["kind"]], self.exact)

    def snapshot(self, slots):
        """``{slot: StreamState}`` of the listed slots, without disturbing them: one launch on the current stream, no host
        synchronisation; the payloads are views into one uint8 device buffer.  A slot that has received nothing is valid
        (restoring it is ``reset``, plus the slot's noise profile if it had one)."""
        self._not_torchgate("snapshot", "a state header of kind 1 cannot tell the two non-stationary gates apart")
        slots = self._slots(slots)
        if len(set(slots)) != len(slots):
            raise ValueError("StreamBank: a slot appears twice in one snapshot")
        self._ensure()
        sizes = [self._gate.stream_export_bytes(self._bank, s) for s in slots]
        offsets, total = [], 0
        for b in sizes:
            offsets.append(total)
            total += (b + 255) // 256 * 256
        with torch.cuda.device(self.device):
            blob = torch.empty(max(total, 256), dtype=torch.uint8, device=self.device)
            heads = self._gate.stream_export(self._bank, slots, blob, offsets)
        out = {}
        for s, hd, off, b in zip(slots, heads, offsets, sizes):
            tensor_io, dt, flat = self._kind[s]
            hd.client0, hd.client1, hd.client2 = int(tensor_io), _DTYPE_CODES.index(dt), int(flat)
            out[s] = StreamState(hd, blob[off:off + b])
        return out

    def restore(self, states):
        """``{slot: StreamState}`` (or ``(slot, state)`` pairs): every listed slot continues the state's stream (whatever it held is dropped; its noise
        profile is the source's).  The states may come from this bank or any bank with the same signature, whatever its
        ``n_streams``, ``max_block``, device or slot, or from ``StreamState.from_bytes`` (uploaded here).  Every argument is
        checked before any device work; one launch on the current stream, no host synchronisation for device states."""
        self._not_torchgate("restore", "a state header of kind 1 cannot tell the two non-stationary gates apart")
        items = []
        for s, state in (states.items() if hasattr(states, "items") else states):      # a mapping, or (slot, state) pairs
            s = self._slots(s)[0]
            if not isinstance(state, StreamState):
                raise ValueError(f"StreamBank: slot {s}: restore takes StreamState objects (got {type(state).__name__})")
            items.append((s, state))
        if len({s for s, _ in items}) != len(items):
            raise ValueError("StreamBank: a slot appears twice in one restore")
        own = self._signature()
        for s, state in items:
            hd = state.head
            if hd.magic != _ffi.SG_STREAM_HEAD_MAGIC or hd.version != _ffi.SG_STREAM_HEAD_VERSION:
                raise ValueError(f"StreamBank: slot {s}: not a stream state of format version {_ffi.SG_STREAM_HEAD_VERSION}")
            for f in _ffi.STREAM_SIGNATURE:
                if getattr(hd, f) != own[f]:
                    raise ValueError(f"StreamBank: slot {s}: the state comes from a different kind of bank: {f} is "
                                     f"{getattr(hd, f)!r} there and {own[f]!r} here")
            td = t_decided(hd.n, self.win_length, self.hop_length)
            ts = max(-1, td - self.lookahead_frames)
            ta = max(-1, ts - self.nt)
            if hd.n < 0 or (hd.td, hd.ts, hd.ta) != (td, ts, ta) or hd.par not in (0, 1) or \
                    hd.E != emitted(hd.n, self.win_length, self.hop_length, self._lag):
                raise ValueError(f"StreamBank: slot {s}: the state's counters do not fit together (n = {hd.n})")
            want = state_payload_bytes(hd.n, self.n_fft, self.win_length, self.hop_length, self.nt, self.lookahead_frames,
                                       self.channels, _KINDS[own["kind"]], self.exact)
            if hd.payload_bytes != want or state.payload.numel() != want or state.payload.dtype != torch.uint8:
                raise ValueError(f"StreamBank: slot {s}: the state's payload is {state.payload.numel()} bytes, its counters "
                                 f"need {want}")
            if not (0 <= hd.client1 < len(_DTYPE_CODES)):
                raise ValueError(f"StreamBank: slot {s}: unknown sample type code {hd.client1} in the state")
        if not items:
            return
        self._ensure()
        with torch.cuda.device(self.device):
            blob, offsets = self._gather([st.payload for _, st in items])
            self._gate.stream_import(self._bank, [s for s, _ in items], blob, offsets, [st.head for _, st in items])
        for s, state in items:
            hd = state.head
            self._n[s], self._e[s] = int(hd.n), int(hd.E)
            self._has_noise[s] = bool(hd.has_thr) or not self.stationary or self.noise_from_stream
            self._kind[s] = (bool(hd.client0), _DTYPE_CODES[hd.client1], bool(hd.client2))

    def _gather(self, payloads):
        """(a uint8 tensor on the bank's device, byte offset of every payload from its first byte).  Contiguous payloads on
        this device at 256-byte aligned addresses (a snapshot's views) are read where they lie, offsets counted from the
        lowest one; anything else -- host states, other devices -- is packed into a new buffer, host states through one
        pinned upload."""
        if all(p.device == self.device and p.is_contiguous() and p.data_ptr() % 256 == 0 for p in payloads):
            first = min(payloads, key=lambda p: p.data_ptr())
            return first, [p.data_ptr() - first.data_ptr() for p in payloads]
        offsets, total = [], 0
        for p in payloads:
            offsets.append(total)
            total += (p.numel() + 255) // 256 * 256
        blob = torch.empty(max(total, 256), dtype=torch.uint8, device=self.device)
        host = [(o, p) for o, p in zip(offsets, payloads) if p.device.type == "cpu"]
        if len(host) == len(payloads):
            stage = torch.empty(max(total, 256), dtype=torch.uint8, pin_memory=True)
            for o, p in host:
                stage[o:o + p.numel()] = p
            blob.copy_(stage, non_blocking=True)
            return blob, offsets
        for o, p in zip(offsets, payloads):
            blob[o:o + p.numel()].copy_(p, non_blocking=True)
        return blob, offsets


class StreamGate:
    """One stream: ``push(block) -> out``, ``flush() -> tail`` (a ``StreamBank`` of one slot; same arguments,
    ``stationary=False``, ``noise_from_stream=True``, ``precision="float64"`` and ``algorithm="torchgate"`` included)."""

    def __init__(self, sr, y_noise=None, **kw):
        self.bank = StreamBank(sr, 1, y_noise=y_noise, **kw)
        self.latency_samples = self.bank.latency_samples

    def push(self, block):
        return self.bank.push({0: block})[0]

    def flush(self):
        return self.bank.flush([0])[0]

    def push_spectrum(self, block, return_mask=False):
        """``(samples, Y)`` or ``(samples, Y, mask)`` (``StreamBank.push_spectrum``)."""
        return self.bank.push_spectrum({0: block}, return_mask=return_mask)[0]

    def flush_spectrum(self, block=None, return_mask=False):
        """``(tail, Y)`` or ``(tail, Y, mask)``: the remaining samples and frames (``StreamBank.flush_spectrum``)."""
        return self.bank.flush_spectrum([0], None if block is None else {0: block}, return_mask=return_mask)[0]

    def set_filterbank(self, fb):
        self.bank.set_filterbank(fb)

    def push_features(self, block, **kw):
        """``(samples, feat)`` or ``(samples, feat, mask)`` (``StreamBank.push_features``; the same keywords)."""
        return self.bank.push_features({0: block}, **kw)[0]

    def flush_features(self, block=None, **kw):
        """``(tail, feat)`` or ``(tail, feat, mask)``: the remaining samples and frames (``StreamBank.flush_features``)."""
        return self.bank.flush_features([0], None if block is None else {0: block}, **kw)[0]

    def reset(self):
        self.bank.reset([0])

    def noise_profile(self):
        return self.bank.noise_profile(0)

    def snapshot(self):
        """The stream's ``StreamState`` (``StreamBank.snapshot``)."""
        return self.bank.snapshot([0])[0]

    def restore(self, state):
        """Continue ``state``'s stream here (``StreamBank.restore``)."""
        self.bank.restore({0: state})

    def close(self):
        self.bank.close()
