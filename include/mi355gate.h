/*
 * mi355gate.h -- C ABI of libmi355gate.so, the MI355X (gfx950) spectral-gating engine.
 *
 * This is the drop-in boundary for ONE hot path of timsainb/noisereduce: the chunk
 * filter  STFT -> per-band noise statistics -> threshold/sigmoid mask -> 2-D mask
 * smoothing -> masked complex multiply -> overlap-add ISTFT.  Nothing like this ABI
 * exists in the reference (it is pure Python); each entry point states which reference
 * interface it replaces (paths relative to /root/reference/noisereduce/).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types.  All `*_dev` pointers are DEVICE
 *     pointers (e.g. torch.Tensor.data_ptr() of a ROCm tensor); `*_host` are host pointers.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  Every call only
 *     ENQUEUES work on that stream unless documented as synchronising.
 *   - return value: 0 = success, negative = error (SG_E_*); text via sg_last_error().
 *     Nothing throws across the boundary.
 *   - a handle is not thread-safe; use one handle per (device, stream).
 *   - caller owns input/output buffers; the library owns its workspace (grown on demand,
 *     bounded by sg_params.max_workspace_bytes; large jobs are processed in unit batches).
 *   - non-finite samples: a NaN behaves as in the reference (spectralgate/stationary.py:75-106,
 *     torchgate/torchgate.py:140-160: numpy / torch maxima and means keep it): every band of the
 *     chunk / row that sees it is gated, a NaN in the noise clip gates everything, the NaN itself
 *     survives in the output.  An Inf sample is treated like a NaN.
 */
#ifndef MI355GATE_H
#define MI355GATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_VERSION 100 /* 0.1.0 */

/* The library is built with -fvisibility=hidden: only the entry points declared here are exported. */
#ifndef SG_API
#define SG_API __attribute__((visibility("default")))
#endif

/* error codes */
#define SG_OK 0
#define SG_E_INVALID (-1)     /* bad argument (maps to ValueError)            */
#define SG_E_UNSUPPORTED (-2) /* geometry outside the kernels' range          */
#define SG_E_HIP (-3)         /* HIP runtime error                            */
#define SG_E_NOMEM (-4)       /* workspace allocation failed                  */
#define SG_E_STATE (-5)       /* call order (e.g. no noise threshold yet)     */
#define SG_E_HANDOFF (-6)     /* a bounded inter-workgroup wait timed out: output invalid, re-run (sg_check_errors) */

/* sample dtypes of caller buffers */
#define SG_F32 0
#define SG_F64 1
#define SG_I16 2
#define SG_I32 3

/* algorithm variant: the reference holds two different algorithms behind one API
 *  */
#define SG_VARIANT_S 0 /* numpy/scipy "spectralgate": spectralgate/{base,stationary,nonstationary}.py */
#define SG_VARIANT_T 1 /* torch "torchgate": torchgate/torchgate.py                                   */

typedef struct sg_params {
  int32_t variant;    /* SG_VARIANT_S | SG_VARIANT_T                                        */
  int32_t stationary; /* 1: stationary (threshold) mask, 0: non-stationary (sigmoid) mask   */
  int32_t n_fft;      /* 4..32768, or a power of two up to 65536 (base.py:77; torchgate.py:55) */
  int32_t win_length; /* <= n_fft (base.py:79-82)                                           */
  int32_t hop_length; /* >= 1    (base.py:83-86)                                            */
  int32_t n_grad_freq; /* mask-smoothing half width in bins  (base.py:104), >= 1            */
  int32_t n_grad_time; /* mask-smoothing half width in frames (base.py:115), >= 1           */
  int32_t smooth_mask; /* 0: no smoothing (base.py:90-91,124-125)                           */
  int64_t chunk_size;  /* S only: base.py:66 (reduce_noise default 600000)                  */
  int64_t padding;     /* S only: base.py:67 (default 30000)                                */
  double prop_decrease;     /* base.py:88; torchgate.py:53                                  */
  double n_std_thresh;      /* stationary.py:45,79-81; torchgate.py:160                     */
  double top_db;            /* 80 (spectralgate/utils.py:11) or 40 (torchgate/utils.py:6)   */
  int32_t ddof;             /* 0: np.std (stationary.py:77); 1: torch.std_mean (torchgate.py:158) */
  int32_t n_movemean;       /* T non-stationary: boxcar length (torchgate.py:179-190)       */
  double nonstat_thresh;    /* S: thresh_n_mult_nonstationary; T: n_thresh_nonstationary     */
  double nonstat_slope;     /* S: sigmoid_slope_nonstationary; T: 1 / temp_coeff_nonstationary */
  double iir_b;             /* S non-stationary: one-pole coefficient (nonstationary.py:109-114) */
  int64_t max_workspace_bytes; /* 0 = default (8 GiB) */
} sg_params;

typedef struct sg_handle sg_handle;

SG_API int sg_version(void);

/* Last error text of a handle (or of the last failed sg_create when h == NULL). */
SG_API const char* sg_last_error(const sg_handle* h);

/* Replaces SpectralGate.__init__ parameter resolution (base.py:33-97) and
 * TorchGate.__init__ (torchgate.py:31-71): builds twiddle/window/smoothing tables on the
 * current HIP device.  `window_host`: win_length doubles, or NULL for the periodic Hann
 * window both references use (scipy get_window('hann'), torch.hann_window). */
SG_API int sg_create(const sg_params* p, const double* window_host, sg_handle** out);
SG_API int sg_destroy(sg_handle* h);

/* Geometry helpers: number of STFT frames and ISTFT output length for a length-L signal
 * (scipy/_spectral_py.py:2185-2189,1715; torch.stft/istft center=True). */
SG_API int sg_n_frames(const sg_handle* h, int64_t L, int64_t* n_frames);
SG_API int sg_output_length(const sg_handle* h, int64_t L, int64_t* out_len);

/* Workspace (bytes of HBM) the handle will own after an sg_process_chunks call on a (C, N) recording
 * (chunked as in sg_process_chunks) -- so that a caller can budget device memory next to the recording
 * (base.py:180-216 streams through a memmap instead; here units are processed in batches bounded by
 * sg_params.max_workspace_bytes).  An upper bound: it includes the exchange buffers of the fused kernels and the
 * float32 copy that a recording of another sample type (int16 / int32 / float64) costs on the default geometry --
 * C * N * 4 bytes, which a float32 recording does not pay.  The entry point does not know the sample type of the call
 * to come: unless SG_OPT_FAST_INTEGER is set (and SG_OPT_FORCE_EXACT clear) it reports the LARGER of the fused float32
 * pipeline and the float64 pipeline that integer outputs take by default (32 bytes per time-frequency cell plus float64
 * frames, batched under max_workspace_bytes / the 8 GiB default); with SG_OPT_FORCE_EXACT, the float64 figure.
 * Pure host arithmetic, no device work. */
SG_API int sg_workspace_bytes(const sg_handle* h, int64_t C, int64_t N, int32_t chunked, int64_t* bytes);

/* ---- variant S -------------------------------------------------------------------- */

/* Replaces the noise-statistics block of SpectralGateStationary.__init__
 * (stationary.py:47-81): channel mean of the (C, n) noise clip, STFT, dB with -top_db
 * floor, per-band mean/std over time, thresh = mean + n_std*std.  The caller applies
 * clip_noise_stationary (n = min(n, chunk_size)).  Result stays on the device. */
SG_API int sg_noise_stats(sg_handle* h, const void* noise_dev, int dtype, int64_t C, int64_t n,
                   int64_t row_stride, void* stream);
/* Read back / override the per-band threshold in dB (n_fft/2+1 doubles).
 * sg_get_noise_threshold synchronises the stream. */
SG_API int sg_get_noise_threshold(sg_handle* h, double* thresh_host, int32_t n_bins, void* stream);
SG_API int sg_set_noise_threshold(sg_handle* h, const double* thresh_host, int32_t n_bins, void* stream);
/* Device-to-device forms (asynchronous on `stream`, no host synchronisation): used to broadcast
 * the threshold between ranks with RCCL. */
SG_API int sg_get_noise_threshold_dev(sg_handle* h, double* thresh_dev, int32_t n_bins, void* stream);
SG_API int sg_set_noise_threshold_dev(sg_handle* h, const double* thresh_dev, int32_t n_bins, void* stream);

/* Replaces SpectralGate.get_traces + filter_chunk + _read_chunk + _do_filter for a whole
 * (C, N) planar recording that already lives in HBM (base.py:130-226): the reference's
 * chunk grid (chunk i = samples [i*cs, (i+1)*cs), filtered on a zero-padded window of
 * `padding` extra samples per side, padding discarded) is evaluated on the device, all
 * (channel, chunk) units in one set of launches.  Writes out[c][g - start_frame] for
 * g in [start_frame, end_frame); pass 0, N for everything.  `chunked` = 0 reproduces the
 * single-window branch (base.py:222), 1 the chunk grid (base.py:175-216).
 * `halo_left` / `halo_right`: number of valid samples stored BEFORE index 0 / AFTER index N-1
 * of every row (0 for a plain recording).  A rank that holds one time shard of a longer
 * recording passes its neighbours' seam samples this way so that chunk windows read real
 * data instead of zeros across the shard boundary. */
SG_API int sg_process_chunks(sg_handle* h, const void* in_dev, int in_dtype, void* out_dev,
                      int out_dtype, int64_t C, int64_t N, int64_t in_stride,
                      int64_t out_stride, int64_t start_frame, int64_t end_frame,
                      int32_t chunked, int64_t halo_left, int64_t halo_right, void* stream);

/* Replaces SpectralGate._do_filter(chunk) (base.py:158-160; stationary.py:129-133;
 * nonstationary.py:99-103): (C, Lp) padded chunk in, (C, Lp) filtered chunk out, the
 * last Lp - sg_output_length(Lp) samples are zero like the reference's. */
SG_API int sg_filter_padded(sg_handle* h, const void* chunk_dev, int in_dtype, void* out_dev,
                     int out_dtype, int64_t C, int64_t Lp, int64_t in_stride,
                     int64_t out_stride, void* stream);

/* ---- variant S: ragged batches of recordings --------------------------------------------- */
/* Many recordings of different lengths and channel counts in one call, each gated exactly as reduce_noise gates it
 * alone (noisereduce.py:13-185 -> base.py:167-226 per recording).  x_dev holds every recording's channels (sample type
 * in_dtype); out_dev receives every recording's output (out_dtype). */
typedef struct sg_clip {   /* one recording of the batch */
  int64_t x_offset;        /* element offset of channel 0 in x_dev; channel c at x_offset + c * x_stride */
  int64_t n;               /* samples per channel */
  int64_t x_stride;        /* elements between channels */
  int32_t channels;
  int32_t noise;           /* stationary gate: index into the noise table (ignored by the non-stationary gate) */
  int64_t out_offset;      /* element offset of channel 0 in out_dev */
  int64_t out_stride;      /* elements between output channels */
} sg_clip;
typedef struct sg_noise_src {   /* one noise clip (stationary.py:47-64: the caller applies clip_noise_stationary to n) */
  int64_t offset;          /* element offset of channel 0 */
  int64_t n;               /* samples per channel, >= win_length */
  int64_t stride;          /* elements between channels */
  int32_t channels;        /* the statistics read the channel mean (stationary.py:61) */
  int32_t in_x;            /* 1: the samples live in x_dev (sample type in_dtype), 0: in noise_dev (noise_dtype) */
} sg_noise_src;
/* Bytes of HBM workspace sg_process_clips needs to process all clips in ONE sub-batch (tables and fields, for the
 * handle's chunk_size / padding and the noise sources the clips use; host arithmetic only).  It is the figure
 * sg_process_clips compares with its budget: max_workspace_bytes >= the result runs the clips as one sub-batch, a smaller
 * budget splits them (clips in order, each sub-batch as large as fits; a clip that alone exceeds the budget is a sub-batch
 * of its own).  The handle keeps the largest workspace it has used until sg_destroy; a stationary call also keeps
 * n_noise * round_up(n_fft / 2 + 1, 16) doubles of thresholds (sg_debug_clip_thresholds). */
SG_API int sg_clips_workspace_bytes(const sg_handle* h, const sg_noise_src* noise, int32_t n_noise, const sg_clip* clips,
                                    int64_t n_clips, int64_t* bytes);
/* Replaces a loop of SpectralGate.get_traces calls (base.py:167-226) over n_clips recordings.  Every recording is cut into
 * the reference's units -- one unit [-padding, n + padding) when n <= chunk_size (or chunk_size == 0, meaning None:
 * base.py:222), else ceil(n / chunk_size) windows of chunk_size + 2 padding samples (base.py:152-156,175-216) -- and every
 * unit is gated on its own frame count: stationary gate with the threshold of its clip's noise source (stationary.py:47-127,
 * thresholds computed here from the noise table), non-stationary gate with the recurrence over the unit's frames
 * (nonstationary.py:47-115).  Kept samples are written to out_dev; nothing else is.  Clips are independent: a recording's
 * output does not depend on the other clips, their order or the sub-batch split.  max_workspace_bytes: sub-batch budget
 * (0: 4 GiB).  chunk_size / padding / window / smoothing come from the handle (variant S only).  Enqueues only. */
SG_API int sg_process_clips(sg_handle* h, const void* x_dev, int in_dtype, const void* noise_dev, int noise_dtype,
                            const sg_noise_src* noise, int32_t n_noise, const sg_clip* clips, int64_t n_clips,
                            void* out_dev, int out_dtype, int64_t max_workspace_bytes, void* stream);

/* ---- variant S: banks of live streams ------------------------------------------------------ */
/* The stationary gate with a fixed noise threshold, advanced block by block (no counterpart in the reference, which needs
 * the whole recording: base.py:130-226).  A bank holds n_slots independent streams of `channels` channels; a step pushes
 * a block of any length (0 included) to any subset of them and runs a fixed number of launches.  With h = win_length / 2,
 * nt = the time half width of the mask smoothing (0 without smoothing) and n samples received, a stream has emitted
 * E(n) = max(0, (floor((n + h - win_length) / hop) - nt + 1) * hop - h) samples (sg_stream_emitted: host arithmetic), so
 * the delay stays below win_length + (nt + 1) * hop samples.  The concatenated output is the offline gate of the whole
 * signal for padding = 0 (frames, mask smoothing and overlap-add of sg_process_clips' single window), except for the
 * -top_db floor, which is causal: a band's floor at frame t is its maximum over frames 0..t minus top_db.  A NaN / Inf
 * sample gates every band from its first frame on until the slot is flushed or reset.  The output does not depend on the
 * block split, the slot, or the other streams of a step.  Stationary handles with a power-of-two n_fft from 256 to 4096
 * (SG_E_UNSUPPORTED / SG_E_INVALID otherwise; non-stationary handles: sg_stream_create_nonstationary
 * below).  The handle must outlive the bank; errors are reported through it
 * (sg_last_error(h)). */
typedef struct sg_stream_bank sg_stream_bank;
typedef struct sg_stream_rec {   /* one stream's part of a step */
  int32_t slot;
  int32_t flush;           /* != 0: the stream ends with this block: every remaining sample is emitted, the slot is empty after */
  int64_t n_samples;       /* block length per channel, 0 .. max_block */
  int64_t in_offset;       /* element offset of channel 0 of the block in in_dev; channel c at in_offset + c * in_stride */
  int64_t in_stride;
  int64_t out_offset;      /* element offset of channel 0 of the emitted samples in out_dev */
  int64_t out_stride;
} sg_stream_rec;
SG_API int sg_stream_create(sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block, sg_stream_bank** out);
SG_API int sg_stream_destroy(sg_stream_bank* b);
/* Threshold (dB, n_fft / 2 + 1 values) of the listed slots: thresh_host, or -- thresh_host == NULL -- the handle's current
 * threshold on the device (sg_noise_stats / sg_set_noise_threshold*), copied: later changes of the handle's do not reach
 * the bank.  Enqueues only. */
SG_API int sg_stream_set_threshold(sg_stream_bank* b, const int32_t* slots, int32_t n_slots, const double* thresh_host,
                                   int32_t n_bins, void* stream);
/* One step.  Record i appends n_samples samples per channel to its stream and writes the E(n + n_samples) - E(n) newly
 * final samples per channel (flush: all n + n_samples - E(n) remaining ones, the inverse transform's zero tail included;
 * fewer than win_length samples in the whole stream: SG_E_INVALID) to out_dev.  A slot appears at most once per step.
 * Samples beyond n_samples are never read, nothing beyond the emitted samples is written.  SG_F32 / SG_F64 buffers
 * (an exact bank, sg_stream_create_ex below: SG_I16 / SG_I32 too).
 * Every argument is checked before any device work; enqueues only. */
SG_API int sg_stream_push(sg_stream_bank* b, const void* in_dev, int in_dtype, void* out_dev, int out_dtype,
                          const sg_stream_rec* recs, int32_t n_recs, void* stream);
/* One step that also hands out the gated spectrogram: sg_stream_push -- same records, same checks, same four launches,
 * bitwise the same audio in out_dev and the same state afterwards -- plus, for every frame the step applies, the frame's
 * gated spectrum Y[t, k] = Z[t, k] * mask[t, k], k = 0 .. n_fft / 2: the very product the step inverts, stored on its way
 * to the inverse transform.  With F = n_fft / 2 + 1, h = win_length / 2, nt and L as above (L = 0 on a stationary bank):
 *   - after n samples a stream has applied A(n) = max(0, floor((n + h - win_length) / hop) - nt - L + 1) frames
 *     (sg_stream_bank_frames: host arithmetic; E(n) = max(0, A(n) * hop - h)).  Record i reports the A(n + n_samples) -
 *     A(n) newly applied ones; a flush reports all remaining ones up to T = (N + 2 h - win_length) / hop + 1, N the
 *     stream's length.  After any sequence of steps the reported frames of a stream, concatenated, are frames 0 .. A(n) -
 *     1 (0 .. T - 1 after the flush); frame t is the frame of samples [t * hop - h, t * hop - h + win_length), zeros
 *     outside the stream.  Frames that pass in a plain sg_stream_push step are simply not reported: the two kinds of
 *     step mix freely.
 *   - Z is scipy.signal.stft's transform of the whole signal (window scaled by 1 / sum(window), padding = 0) and mask the
 *     final mask the audio is gated with: each frame is the offline Z * mask, with the causal -top_db floor (and, on a
 *     non-stationary bank, the bounded lookahead) exactly as for the audio.  The mask is evaluated once per band in
 *     float64 and Y is the float64 product rounded once to spec_dtype; bins 0 and n_fft / 2 carry an imaginary part of
 *     +0.0.  scipy.signal.istft of the concatenated frames is the concatenated audio.
 *   - Y and mask do not depend, bitwise, on the block split, the slot, the other streams of the step, or on whether
 *     earlier steps were sg_stream_push or sg_stream_push_spectrum; sg_stream_export / sg_stream_import between spectrum
 *     steps continue them bit for bit (the payload does not change).
 * spec_dev holds complex values of spec_dtype's real type (SG_F32: float pairs, SG_F64: double pairs; any bank kind);
 * mask_dev, which may be NULL, reals of that type.  spec_recs[i] places record i's frames: frame j of channel c goes to
 * elements spec_offset + c * stride + j * F + k of spec_dev (complex elements) and mask_offset + c * stride + j * F + k of
 * mask_dev, rows of F bins one after the other; stride >= frames * F for a multichannel bank.  Nothing else is written.
 * Every argument is checked before any device work; enqueues only; counters commit at enqueue. */
typedef struct sg_stream_spec_rec {   /* where one stream's newly applied frames go */
  int64_t spec_offset;     /* element (complex) of spec_dev holding bin 0 of channel 0's first new frame */
  int64_t mask_offset;     /* element (real) of mask_dev holding the same cell's mask; ignored when mask_dev is NULL */
  int64_t stride;          /* elements from a channel's first new frame to the next channel's, in both buffers */
} sg_stream_spec_rec;
SG_API int sg_stream_push_spectrum(sg_stream_bank* b, const void* in_dev, int in_dtype, void* out_dev, int out_dtype,
                                   void* spec_dev, int spec_dtype, void* mask_dev, const sg_stream_rec* recs,
                                   const sg_stream_spec_rec* spec_recs, int32_t n_recs, void* stream);
/* A(n) of the bank (nt + L): the frames a stream has applied after n samples.  Host arithmetic only. */
SG_API int sg_stream_bank_frames(const sg_stream_bank* b, int64_t n, int64_t* frames);
/* Filterbank (log-mel) features of live streams.  sg_stream_set_filterbank gives the bank a filterbank of its own
 * (sg_set_filterbank is a variant-T entry point and does not take a stream bank's handle): fb_host is float[F][n_filters]
 * on the host, F = n_fft / 2 + 1, 1 <= n_filters <= 1024, entries finite (negative ones are allowed); SG_E_INVALID
 * otherwise, and the bank keeps the filterbank it had.  The bank owns the device tables (the filterbank, its transpose and
 * the two hull tables of sg_set_filterbank) until sg_stream_destroy; replacing a filterbank synchronises the device first.
 * The filterbank is no part of a stream's state: sg_stream_export / sg_stream_import payloads do not carry it, and a moved
 * stream continues its features where the destination bank holds the same filterbank.
 *
 * sg_stream_push_features is sg_stream_push_spectrum -- same records, same checks, same four launches and one table upload,
 * bitwise the same audio and the same state afterwards, the same frames reported -- with every applied frame's spectrum
 * reduced over the filters while the frame is still on chip instead of being stored:
 *   lin[t, m] = sum_k fb[k][m] * |s * Z[t, k] * mask[t, k]| ^ power        feat = take_log ? ln(lin + eps) : lin
 * power is 1 or 2, eps any number but NaN.  s = scale multiplies the UNSCALED transform (torch.stft's convention at
 * scale = 1); scale = 0 stands for the bank's own 1 / sum(window), the very factor sg_stream_push_spectrum applies, so that
 * the features are those of exactly the Y it reports.  scale is finite and not negative.  Transform, mask, powers and sums
 * are float64, the weights float32 values widened; filter m sums in ascending k over the hull of its non-zero bins, and
 * the value is rounded once at the store (feat_dtype: SG_F32 or SG_F64; mask_dev, which may be NULL, holds reals of that
 * type: exactly the mask rows of sg_stream_push_spectrum).  A frame's features do not depend, bitwise, on the block split,
 * the slot, the other streams of the step, or on whether earlier steps were sg_stream_push, _push_spectrum or
 * _push_features.  feat_recs[i] places record i's frames: filter m of frame j of channel c goes to element feat_offset +
 * c * feat_stride + j * n_filters + m of feat_dev, its mask row to mask_offset + c * mask_stride + j * F + k of mask_dev;
 * feat_stride >= frames * n_filters and mask_stride >= frames * F for a multichannel bank.  Nothing else is written.
 * Without a filterbank: SG_E_INVALID ("no filterbank set").  Every argument is checked before any device work; enqueues
 * only; counters commit at enqueue. */
typedef struct sg_stream_feat_rec {   /* where one stream's newly applied frames go */
  int64_t feat_offset;     /* element of feat_dev holding filter 0 of channel 0's first new frame */
  int64_t feat_stride;     /* elements from a channel's first new frame to the next channel's in feat_dev */
  int64_t mask_offset;     /* element of mask_dev holding bin 0 of the same frame; ignored when mask_dev is NULL */
  int64_t mask_stride;     /* elements from a channel's first new frame to the next channel's in mask_dev */
} sg_stream_feat_rec;
SG_API int sg_stream_set_filterbank(sg_stream_bank* b, const float* fb_host, int32_t n_filters);
SG_API int sg_stream_push_features(sg_stream_bank* b, const void* in_dev, int in_dtype, void* out_dev, int out_dtype,
                                   void* feat_dev, int feat_dtype, void* mask_dev, int32_t power, int32_t take_log,
                                   double eps, double scale, const sg_stream_rec* recs,
                                   const sg_stream_feat_rec* feat_recs, int32_t n_recs, void* stream);
/* Empties the listed slots (their thresholds stay). */
SG_API int sg_stream_reset(sg_stream_bank* b, const int32_t* slots, int32_t n_slots, void* stream);
/* E(n) for the handle's geometry; samples received / emitted so far on a slot.  Host arithmetic only. */
SG_API int sg_stream_emitted(const sg_handle* h, int64_t n, int64_t* emitted);
SG_API int sg_stream_counters(const sg_stream_bank* b, int32_t slot, int64_t* n, int64_t* emitted);
/* The non-stationary gate as a stream (the handle is non-stationary; iir_b, nonstat_thresh, nonstat_slope are its own).
 * No noise profile: sg_stream_set_threshold fails on such a bank; push / reset / destroy / counters serve it as they serve a
 * stationary one.  The forward one-pole pass fwd[f, t] = b A[f, t] + (1 - b) fwd[f, t - 1], fwd[f, -1] = A[f, 0], A = |X|,
 * is carried per band; the smoothed level of frame t is the reference's forward-backward smoother of the signal as known
 * lookahead_frames = L frames later: with e = min(t + L, last frame of the stream), s = fwd[f, e], then
 * s = b fwd[f, k] + (1 - b) s for k = e, e - 1, ..., t.  The mask is sigmoid(((A - s) / s - nonstat_thresh) * nonstat_slope),
 * smoothed and scaled by prop_decrease as sg_process_clips does.  A frame is decided once frames up to t + L lie inside the
 * audio (or at the flush), so E(n) is sg_stream_emitted's with nt + L in place of nt (sg_stream_bank_emitted) and the delay
 * stays below win_length + (nt + L + 1) * hop samples.  With L >= the stream's frame count - 1 the output is the offline
 * gate of the whole signal for padding = 0; a small L with a long time constant gates more causally, by design.  Digital
 * silence gives 0 / 0 = NaN as offline; a NaN / Inf sample keeps the forward state NaN until the slot is flushed or reset.
 * lookahead_frames is 0 .. SG_STREAM_MAX_LOOKAHEAD (SG_E_INVALID beyond: the backward pass of a frame is
 * lookahead_frames + 1 dependent steps per band).  sg_stream_state_bytes: the device memory a bank of the handle's kind
 * would hold (host arithmetic; lookahead_frames is ignored for a stationary handle). */
#define SG_STREAM_MAX_LOOKAHEAD 4096
SG_API int sg_stream_create_nonstationary(sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block,
                                          int32_t lookahead_frames, sg_stream_bank** out);
SG_API int sg_stream_state_bytes(const sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block,
                                 int32_t lookahead_frames, int64_t* bytes);
SG_API int sg_stream_bank_emitted(const sg_stream_bank* b, int64_t n, int64_t* emitted);
/* The stationary gate with the noise profile learnt from the stream itself (the handle is stationary; n_std_thresh and
 * top_db are its own).  Offline, without a noise clip, the reference takes a band's threshold from the mean and the standard
 * deviation of the band's floored dB values over the whole recording; here they are a running estimate, carried per
 * (stream, channel) and band and evaluated inside the decide launch.  For frames t = 0, 1, ... in order, the recurrence being
 * the definition:
 *   db = 20 log10(|X[f, t]| + eps)    rmax = max(rmax, db)    x = max(db, rmax - top_db)          (NaN-sticky)
 *   if learn_frames < 0 or t < learn_frames:  Wn = forget * Wn + 1,  d = x - mu,  mu += d / Wn,  M2 = forget * M2 + d * (x - mu)
 *   thr = mu + n_std_thresh * sqrt(M2 / Wn)    the cell passes when x > thr
 * from Wn = mu = M2 = 0.  forget = 1 gives the cumulative mean and standard deviation (ddof = 0) of frames 0 .. t; forget =
 * exp(-hop / (sr * memory_s)) in (0, 1) forgets exponentially; after learn_frames frames the profile is held.  Frame t is part
 * of its own threshold, so frame 0 is gated whole (thr = x); a band whose dB value is exactly constant stays exactly gated; a
 * NaN / Inf sample gates every band until the slot is flushed or reset; forget <= 1 - 1 / (1 + n_std_thresh^2) (0.69 for 1.5)
 * gates everything, since a cell lies at most sqrt(Wn - 1) deviations above a mean it is part of and Wn < 1 / (1 - forget).
 * Every channel has its own statistics (the reference
 * takes the threshold from the channel mean; no difference for one channel).  With forget = 1, learn_frames < 0 and no band
 * ranging over more than top_db, the threshold after the last frame of a stream is the reference's threshold of that signal as
 * its own noise clip.  Frames, E(n), the delay, flush and the launches per step are a stationary bank's.  forget outside
 * (0, 1] or learn_frames == 0: SG_E_INVALID.  sg_stream_set_threshold fails on such a bank; a flush and sg_stream_reset clear
 * the statistics.
 * sg_stream_noise_profile: the threshold (dB) after the last decided frame of every channel of `slot`, channels x (n_fft / 2 +
 * 1) values to thresh_host, NaN for a channel without a decided frame.  SYNCHRONISES `stream` (the only call here that
 * does).  sg_stream_state_bytes_adaptive: sg_stream_state_bytes for such a bank. */
SG_API int sg_stream_create_adaptive(sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block, double forget,
                                     int64_t learn_frames, sg_stream_bank** out);
SG_API int sg_stream_noise_profile(sg_stream_bank* b, int32_t slot, double* thresh_host, int32_t n_bins, void* stream);
SG_API int sg_stream_state_bytes_adaptive(const sg_handle* h, int32_t n_slots, int32_t channels, int64_t max_block,
                                          int64_t* bytes);
/* Exact banks.  A bank made by the three create calls above stores a frame's segment as float32 and rounds every sample to
 * float32 before it is written: float32-accurate whatever the buffers' type.  sg_stream_create_ex with exact != 0 makes
 * the same bank -- same frames, E(n), delay, flush, launches per step, independence of the block split, the slot and the
 * other streams -- whose segments (and, non-stationary, sigmoid mask rows and smoothed rows) are float64, and whose
 * sg_stream_push takes SG_I16 / SG_I32 as well as SG_F32 / SG_F64 for in_dtype and out_dtype, independently of each
 * other.  An output sample is the float64 result of the streaming gate's definition at the buffer's type: SG_F64 as is,
 * SG_F32 rounded once, SG_I16 / SG_I32 truncated toward zero as ndarray.astype does (the offline integer contract of
 * sg_process_chunks), NaN -> 0 (a non-stationary bank gives 0 / 0 = NaN on digital silence; what astype makes of NaN
 * differs from platform to platform, 0 is the stated choice); a value outside the integer type's range is as unspecified
 * as astype's.  A float64 value within rounding noise of an integer may truncate to either neighbour, as offline.  On any
 * other bank the integer codes are SG_E_INVALID as before, and nothing changes state.
 * kind selects the create call (SG_STREAM_FIXED: sg_stream_create; SG_STREAM_NONSTATIONARY: lookahead_frames is read;
 * SG_STREAM_ADAPTIVE: forget and learn_frames are read; fields a kind does not read are ignored).  With exact == 0 the
 * bank is the one the matching create call makes.  sg_stream_state_bytes_ex: the device memory such a bank would hold --
 * an exact non-stationary bank keeps its mask rows at 8 bytes, nothing else differs (host arithmetic; SG_E_INVALID when
 * kind does not fit the handle).
 * A handle of variant T (TorchGate) streams too, its NON-STATIONARY gate alone: sg_stream_create_ex makes, and
 * sg_stream_state_bytes_ex sizes, a bank of kind SG_STREAM_NONSTATIONARY whose level is TorchGate's moving mean instead of
 * the one-pole smoother.  With K = the handle's n_movemean (1 .. SG_STREAM_MAX_LOOKAHEAD), lo = (K - 1) / 2 and
 * L = K - 1 - lo:  S[f, t] = (1 / K) sum of A[f, q] over q in [t - lo, t - lo + K) cut to [0, last frame of the stream],
 * every sum taken afresh in ascending q in float64, A = |X| unscaled;  raw = sigmoid(((A - S) / S - nonstat_thresh) *
 * nonstat_slope);  the mask is prop_decrease * (raw - 1) + 1 smoothed with the zero-padded triangle over the stream's own
 * field (prop_decrease first: TorchGate's order).  That mean reads nothing beyond frame t + L, so with a lookahead of L
 * frames the stream EQUALS the offline gate of the whole signal: E(n) and the delay are the non-stationary bank's with
 * this L, and desc->lookahead_frames must be 0 (n_movemean decides it; SG_E_INVALID otherwise).  Frame t is the frame of
 * samples [t hop - win_length / 2, .. + win_length) -- the samples torch.stft(center = 1) windows; win_length must be even
 * -- and a flushed stream of N samples has emitted N samples: hop * (N / hop) of them are sg_process_batch's, the rest the
 * same overlap-add over the window envelope continued.  exact != 0 works as for the non-stationary bank.  It stays
 * SG_E_INVALID, with a message that says so, for a stationary variant-T handle (its statistics need xn or the whole
 * recording), for any other kind on a variant-T handle and for an odd win_length.  On such a bank sg_stream_export_bytes,
 * sg_stream_export and sg_stream_import (a header of kind 1 could not tell the two non-stationary gates apart; the header
 * format does not change) and sg_stream_push_spectrum (it would have to take torch.stft's phase and scale) return
 * SG_E_INVALID and leave the bank untouched; sg_stream_push_features with scale = 1 gives sg_gate_features' features.
 * sg_stream_create, sg_stream_create_nonstationary and sg_stream_create_adaptive answer a variant-T handle as before
 * ("... is a variant-S entry point"). */
#define SG_STREAM_FIXED 0
#define SG_STREAM_NONSTATIONARY 1
#define SG_STREAM_ADAPTIVE 2
typedef struct sg_stream_desc {
  int32_t n_slots;
  int32_t channels;
  int64_t max_block;
  int32_t kind;              /* SG_STREAM_FIXED / SG_STREAM_NONSTATIONARY / SG_STREAM_ADAPTIVE */
  int32_t lookahead_frames;  /* non-stationary: 0 .. SG_STREAM_MAX_LOOKAHEAD */
  double forget;             /* adaptive: forgetting factor per frame, (0, 1] */
  int64_t learn_frames;      /* adaptive: frames that update the statistics (negative: all) */
  int32_t exact;             /* != 0: float64 segments, every sample type in and out */
} sg_stream_desc;
SG_API int sg_stream_create_ex(sg_handle* h, const sg_stream_desc* desc, sg_stream_bank** out);
SG_API int sg_stream_state_bytes_ex(const sg_handle* h, const sg_stream_desc* desc, int64_t* bytes);
/* State transfer.  sg_stream_export copies what the listed slots' streams need to go on -- and nothing else -- out of the
 * bank into blob_dev; sg_stream_import writes such payloads into slots of a COMPATIBLE bank (this one, or one of another
 * n_slots, max_block, device or process), after which sg_stream_counters and the next sg_stream_push continue each stream
 * bit for bit as if it had always lived there.  Compatible: every signature field of sg_stream_head equal (SG_E_INVALID
 * names the first that differs).  One launch per call, however many slots; enqueues only.  Export does not disturb the
 * streams; import drops whatever the target slots held, their thresholds included (has_thr is the source's).
 *   slot i's payload lies at blob_dev + offsets[i]: offsets are multiples of 256 bytes, blob_dev is 256-byte aligned; the
 *   payloads of an export must not overlap, those of an import may (two slots fed from one payload: a fork);
 *   heads[i] is written by export (host memory) and read by import; payload_bytes = sg_stream_export_bytes (host
 *   arithmetic from the slot's counters, a multiple of 8); `client` is opaque to the library and travels unchanged.
 * The payload is canonical: samples and frame rows in index order from the first live one, not at their ring positions,
 * so it does not depend on max_block.  Per slot: a fixed bank's thr and T2 rows; then per channel the ring samples
 * [max(0, n - RC), n), the live overlap-add carry [E, ta * hop - h + win_length), and -- stationary / adaptive -- the band
 * maxima and the bit rows of frames [max(0, ta + 1 - nt), td], -- adaptive -- the three rows of noise statistics, -- non-
 * stationary -- the forward state, the A / fwd rows of frames (ts, td] and the sigmoid rows of frames [max(0, ta + 1 -
 * nt), ts].  Every argument is checked before any device work: an unknown slot, a slot listed twice,
 * a bad offset, a head whose magic, version, signature, counters (td, ts, ta, E follow from n) or payload_bytes do not
 * fit are SG_E_INVALID and change nothing.  Import commits the host counters at enqueue, as sg_stream_push does. */
#define SG_STREAM_HEAD_MAGIC 0x54534753 /* "SGST" */
#define SG_STREAM_HEAD_VERSION 1
typedef struct sg_stream_head {
  int32_t magic;
  int32_t version;
  /* signature: what has to be equal between the two banks */
  int32_t n_fft;
  int32_t win_length;
  int32_t hop_length;
  int32_t channels;
  int32_t kind;              /* SG_STREAM_FIXED / SG_STREAM_NONSTATIONARY / SG_STREAM_ADAPTIVE */
  int32_t n_grad_freq;
  int32_t n_grad_time;
  int32_t smooth_mask;
  int32_t lookahead_frames;
  int32_t exact;
  double prop_decrease;
  double n_std_thresh;
  double top_db;
  double iir_b;
  double nonstat_thresh;
  double nonstat_slope;
  double noise_forget;
  int64_t noise_learn_frames;
  /* counters of the stream */
  int64_t n;                 /* samples received */
  int64_t td;                /* last transformed frame (-1: none) */
  int64_t ts;                /* last frame with a raw mask row */
  int64_t ta;                /* last applied frame */
  int64_t E;                 /* samples emitted */
  int32_t par;               /* the live carry buffer */
  int32_t has_thr;           /* the slot has its noise profile */
  int64_t payload_bytes;
  int32_t client0;           /* opaque to the library (the Python layer: kind of the last block) */
  int32_t client1;
  int32_t client2;
  int32_t client3;
} sg_stream_head;
SG_API int sg_stream_export_bytes(const sg_stream_bank* b, int32_t slot, int64_t* bytes);
/* The payload size that a header's signature and n give: host arithmetic without a bank, a handle or a device (what a
 * receiver checks a header against before it allocates anything).  SG_E_INVALID for a signature no bank can have. */
SG_API int sg_stream_head_bytes(const sg_stream_head* head, int64_t* bytes);
SG_API int sg_stream_export(sg_stream_bank* b, const int32_t* slots, int32_t n_slots, void* blob_dev, const int64_t* offsets,
                            sg_stream_head* heads_out, void* stream);
SG_API int sg_stream_import(sg_stream_bank* b, const int32_t* slots, int32_t n_slots, const void* blob_dev,
                            const int64_t* offsets, const sg_stream_head* heads_in, void* stream);

/* ---- variant T -------------------------------------------------------------------- */

/* Replaces TorchGate.forward(x, xn) (torchgate.py:200-264): x (B, L) -> out
 * (B, sg_output_length(L)) = hop*(T-1) (+1 for an odd n_fft), T = sg_n_frames(L) =
 * 1 + (L + 2*(n_fft/2) - n_fft)/hop -- hop*(L/hop) for an even n_fft.  xn_dev may be NULL (statistics from x itself, per row) or a
 * (Bn, Ln) noise batch with Bn in {1, B}.
 * mask_out_dev: NULL, or a float[B][T][FS] buffer (T = sg_n_frames(L), FS = round_up(n_fft/2+1,16))
 * that receives the final (smoothed) mask, for sg_process_batch_backward. */
SG_API int sg_process_batch(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L,
                     int64_t x_stride, const void* xn_dev, int64_t Bn, int64_t Ln,
                     int64_t xn_stride, void* out_dev, int out_dtype, int64_t out_stride,
                     float* mask_out_dev, void* stream);

/* Adjoint of sg_process_batch with the mask held fixed (TorchGate.forward is differentiable
 * w.r.t. x with the mask detached, torchgate.py:126,167; the reference gets this from autograd
 * through torch.stft/istft): grad_out (B, Lout) -> grad_x (B, L), both of sample type `dtype`
 * (SG_F32 or SG_F64).  mask_dev = the buffer filled by sg_process_batch(mask_out_dev). */
SG_API int sg_process_batch_backward(sg_handle* h, const void* grad_out_dev, int dtype, int64_t B,
                              int64_t L, int64_t go_stride, const float* mask_dev,
                              void* grad_x_dev, int64_t gx_stride, void* stream);

/* The gated spectrogram, TorchGate.gated_stft: what the reference multiplies on the line before its torch.istft
 * (torchgate.py:252).  x (B, L) -> spec [B][T][F] complex (interleaved re, im) of sample type dtype (SG_F32 -> 2 x float,
 * SG_F64 -> 2 x double), T = sg_n_frames(L), F = n_fft/2 + 1, bins contiguous, no padding -- the storage of torch.stft's
 * result; = rfft(window * frame) * mask, unscaled (torch.stft, center=True, pad_mode="constant").  The mask is the one
 * sg_process_batch computes for the same input (same statistics, decisions and smoothing); xn / Bn / Ln as there.
 * mask_out_dev: NULL or float[B][T][FS], the final mask, natural bin order (the buffer sg_gate_spectrum_backward takes).
 * Power-of-two n_fft from 256 to 4096 (SG_E_UNSUPPORTED otherwise); float32 transforms for both sample types.  Rows are
 * processed in sub-batches under the handle's max_workspace_bytes, with the same bits as unsplit.  Enqueues only. */
SG_API int sg_gate_spectrum(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                            const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
                            void* spec_dev, float* mask_out_dev, void* stream);

/* Adjoint of sg_gate_spectrum with the mask held fixed: grad_spec [B][T][F] complex of dtype (dL/dRe + i dL/dIm) ->
 * grad_x (B, L) of dtype = frames^T( window * Re sum_{k=0}^{n_fft/2} mask[k] grad[k] e^{+2 pi i k j / n_fft} ): every bin
 * with weight 1, the imaginary parts of bins 0 and n_fft/2 unused, un-normalised overlap-add cropped to [0, L) -- the
 * adjoint of an STFT, no envelope division.  No atomics: the same bits on every run.  Enqueues only. */
SG_API int sg_gate_spectrum_backward(sg_handle* h, const void* grad_spec_dev, int dtype, int64_t B, int64_t L,
                                     const float* mask_dev, void* grad_x_dev, int64_t gx_stride, void* stream);

/* ---- gated filterbank features, TorchGate.gated_filterbank ----
 * sg_set_filterbank: the handle's filterbank, fb_host float[F][n_filters] (HOST memory, F = n_fft/2 + 1, filters
 * contiguous), 1 <= n_filters <= 1024, every entry finite (SG_E_INVALID otherwise); a mel bank is the common case, any real
 * matrix is taken.  Uploads the bank, its transpose and the hulls of its non-zeros per filter and per bin; replaces an
 * earlier bank after a device synchronisation.  Synchronous.  Power-of-two n_fft from 256 to 4096 (SG_E_UNSUPPORTED
 * otherwise). */
SG_API int sg_set_filterbank(sg_handle* h, const float* fb_host, int32_t n_filters);

/* x (B, L) -> feat [B][T][n_filters] of sample type dtype (SG_F32 / SG_F64), filters contiguous:
 * lin[t][m] = sum_k fb[k][m] * (|X[t][k]| * mask[t][k]) ^ power, X and mask as in sg_gate_spectrum (same statistics,
 * decisions and smoothing; xn / Bn / Ln / mask_out_dev as there), power 1 or 2; take_log != 0 stores ln(lin + eps).
 * The transforms are float32, the sums over the bins run in dtype.  SG_E_INVALID when no filterbank is set or power is
 * neither 1 nor 2; SG_E_UNSUPPORTED outside the power-of-two n_fft from 256 to 4096.  Sub-batches as sg_gate_spectrum.
 * Enqueues only. */
SG_API int sg_gate_features(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                            const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride, int32_t power, int32_t take_log,
                            double eps, void* feat_dev, float* mask_out_dev, void* stream);

/* Adjoint of sg_gate_features w.r.t. x with the mask and the filterbank held fixed: grad_feat [B][T][n_filters] of dtype ->
 * grad_x (B, L) of dtype.  x, power, take_log, eps: what the forward call was given (the frames are transformed again;
 * nothing of size B x T x F is kept but mask_dev, the buffer sg_gate_features filled).  For power 1 the derivative at
 * |X[k]| = 0 is 0.  No atomics: the same bits on every run.  Enqueues only. */
SG_API int sg_gate_features_backward(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                     const void* grad_feat_dev, const float* mask_dev, int32_t power, int32_t take_log,
                                     double eps, void* grad_x_dev, int64_t gx_stride, void* stream);

/* sg_process_batch for a PADDED batch: row i of x (B, L) holds lengths[i] samples of audio, 2 * win_length <= lengths[i] <= L,
 * and padding after them (host array of B entries; NULL: every row is full).  With T_i = 1 + lengths[i] / hop and
 * Lout_i = hop * (lengths[i] / hop): out[i][0 .. Lout_i) is what sg_process_batch returns for the row alone at length
 * lengths[i] (statistics, moving mean, mask smoothing and window envelope over the row's own T_i frames), and
 * out[i][Lout_i .. sg_output_length(L)) is 0.  Samples at or beyond lengths[i] are never read.  xn_lengths: the same for the
 * rows of xn (Bn entries, each in [2 * win_length, Ln]; NULL: full).  A row's result does not depend on the other rows,
 * their order or L.  mask_out_dev as in sg_process_batch (frames >= T_i of row i are 0; natural bin order), for
 * sg_process_rows_backward.  Power-of-two n_fft from 256 to 4096 (SG_E_UNSUPPORTED otherwise); float32 / float64 rows.
 * Rows are packed into sub-batches under the handle's max_workspace_bytes (0: 4 GiB); a fixed number of launches per
 * sub-batch.  Enqueues only. */
SG_API int sg_process_rows(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                           const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
                           const int64_t* xn_lengths, void* out_dev, int out_dtype, int64_t out_stride,
                           float* mask_out_dev, void* stream);

/* Adjoint of sg_process_rows with the mask held fixed: grad_out (B, sg_output_length(L)) -> grad_x (B, L).
 * grad_x[i][0 .. lengths[i]) is the gradient of the row alone, grad_x[i][lengths[i] .. L) is 0, and
 * grad_out[i][Lout_i ..) is never read. */
SG_API int sg_process_rows_backward(sg_handle* h, const void* grad_out_dev, int dtype, int64_t B, int64_t L,
                                    int64_t go_stride, const int64_t* lengths, const float* mask_dev, void* grad_x_dev,
                                    int64_t gx_stride, void* stream);

/* sg_gate_spectrum for a PADDED batch (lengths / xn_lengths as in sg_process_rows): spec [B][T][F] complex of dtype,
 * T = sg_n_frames(L).  With T_i = 1 + lengths[i] / hop: spec[i][0 .. T_i) is what sg_gate_spectrum returns for the row
 * alone at length lengths[i] -- statistics, moving mean, mask smoothing (zero-padded at the row's own last frame) and
 * the -top_db floor over the row's own T_i frames; a frame sees zeros, never the padding, at or beyond lengths[i] -- and
 * spec[i][T_i .. T) is +0.0 + 0.0i.  Samples at or beyond lengths[i] / xn_lengths[j] are never read.  A row's result does
 * not depend on the other rows, their order or L.  mask_out_dev: NULL or float[B][T][FS], bit for bit the mask
 * sg_process_rows writes for the same input (frames >= T_i are 0), for sg_gate_spectrum_rows_backward; the bins are
 * multiplied by this float32 mask.  Float64 transforms for both sample types: a float64 result is stored unrounded, a
 * float32 result rounded once.  Power-of-two n_fft from 256 to 4096 (SG_E_UNSUPPORTED otherwise).  Rows are packed into
 * sub-batches under the handle's max_workspace_bytes (0: 4 GiB) with the same bits as unsplit; a fixed number of
 * launches per sub-batch.  Enqueues only. */
SG_API int sg_gate_spectrum_rows(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                 const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
                                 const int64_t* xn_lengths, void* spec_dev, float* mask_out_dev, void* stream);

/* Adjoint of sg_gate_spectrum_rows with the mask held fixed: grad_spec [B][T][F] complex of dtype -> grad_x (B, L) of
 * dtype, as sg_gate_spectrum_backward on every row alone: grad_x[i][0 .. lengths[i]) is the gradient of the row alone,
 * grad_x[i][lengths[i] .. L) is 0, and grad_spec[i][T_i .. T) is never read.  No envelope division, no atomics: the same
 * bits on every run.  Sub-batches as above.  Enqueues only. */
SG_API int sg_gate_spectrum_rows_backward(sg_handle* h, const void* grad_spec_dev, int dtype, int64_t B, int64_t L,
                                          const int64_t* lengths, const float* mask_dev, void* grad_x_dev,
                                          int64_t gx_stride, void* stream);

/* sg_gate_features for a PADDED batch (lengths / xn_lengths as in sg_process_rows; the bank is sg_set_filterbank's):
 * feat [B][T][n_filters] of dtype, filters contiguous, T = sg_n_frames(L).  With T_i = 1 + lengths[i] / hop:
 * feat[i][t][m] = sum_k fb[k][m] * (|X_i[t][k]| * mask_i[t][k]) ^ power for t < T_i, X_i and mask_i what
 * sg_gate_spectrum_rows computes for the row alone (the same launches up to the mask smoothing), power 1 or 2;
 * take_log != 0 stores ln(. + eps).  feat[i][T_i .. T) is what the formula gives for a zero spectrum: +0.0, or ln(eps)
 * rounded to dtype.  Samples at or beyond lengths[i] / xn_lengths[j] are never read.  A row's result does not depend on
 * the other rows, their order or L.  mask_out_dev: NULL or float[B][T][FS], bit for bit the mask sg_gate_spectrum_rows
 * writes for the same input (frames >= T_i are 0), for sg_gate_features_rows_backward; the powers take this float32 mask.
 * Float64 transforms and sums for both sample types: a float64 result is stored unrounded, a float32 result rounded
 * once.  SG_E_INVALID when no filterbank is set or power is neither 1 nor 2; SG_E_UNSUPPORTED outside the power-of-two
 * n_fft from 256 to 4096.  Rows are packed into sub-batches under the handle's max_workspace_bytes (0: 4 GiB) with the
 * same bits as unsplit; a fixed number of launches per sub-batch.  Enqueues only. */
SG_API int sg_gate_features_rows(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                 const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
                                 const int64_t* xn_lengths, int32_t power, int32_t take_log, double eps,
                                 void* feat_dev, float* mask_out_dev, void* stream);

/* Adjoint of sg_gate_features_rows w.r.t. x with the mask and the filterbank held fixed: grad_feat [B][T][n_filters] of
 * dtype -> grad_x (B, L) of dtype, as sg_gate_features_backward on every row alone: grad_x[i][0 .. lengths[i]) is the
 * gradient of the row alone, grad_x[i][lengths[i] .. L) is 0, and grad_feat[i][T_i .. T) is never read.  x, lengths, power,
 * take_log, eps: what the forward call was given (the frames are transformed again; nothing of size B x T x F is kept
 * but mask_dev).  For power 1 the derivative at |X[k]| = 0 is 0.  No atomics: the same bits on every run.  Sub-batches
 * as above.  Enqueues only. */
SG_API int sg_gate_features_rows_backward(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                          const int64_t* lengths, const void* grad_feat_dev, const float* mask_dev,
                                          int32_t power, int32_t take_log, double eps, void* grad_x_dev,
                                          int64_t gx_stride, void* stream);

/* ---- stage taps (used by the parity tests; also plain STFT/ISTFT operators) ------ */

/* Forward STFT of (B, L) rows -> complex float64 Z[B][T][F] (interleaved re,im), same
 * scaling as the variant's reference call (S: 1/sum(w), scipy stft; T: unscaled). */
SG_API int sg_stft(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t stride,
            double* z_dev, void* stream);
/* ---- options ------------------------------------------------------------------------- */
/* Product options.  The A/B, fault-injection and profiling switches the tests and tools use live in
 * mi355gate_debug.h (same library, same sg_set_option). */
#define SG_OPT_FAST_INTEGER 8   /* value != 0: integer (SG_I16 / SG_I32) outputs from the fused float32 kernels: <= 1 LSB away from
                                 * the reference on ~1 % of the samples.  Default: the float64 pipeline, whose truncated result IS
                                 * the reference's (base.py:217-226 casts a float64 array), an order of magnitude slower */
#define SG_OPT_FORCE_EXACT 9    /* value != 0: float64 pipeline for every output dtype (float64 recordings: float64-accurate results) */
SG_API int sg_set_option(sg_handle* h, int32_t option, int64_t value);
/* Current value of an option (the library's default if it was never set). */
SG_API int sg_get_option(const sg_handle* h, int32_t option, int64_t* value);

/* ---- deferred device-side errors -------------------------------------------------------- */
/* The fused kernels of the default geometry hand data from workgroup to workgroup INSIDE a launch (mask bits,
 * partial hops; placement-independent ticket protocol, every wait bounded to about a second).  A wait that
 * times out -- the device was preempted or time-sliced for that long -- cannot be reported by the asynchronous
 * call that enqueued the kernel.  sg_check_errors synchronises `stream` and returns SG_E_HANDOFF when a launch
 * enqueued on this handle since the previous check lost a hand-off: those calls' outputs are invalid and must
 * be re-run.  Entry points that synchronise anyway (sg_get_noise_threshold; the stage taps of mi355gate_debug.h) report
 * the same way; a caller
 * that never checks gets SG_E_HANDOFF from its NEXT compute call on the handle -- and never plausible-looking audio:
 * a tile that lost a hand-off writes NaN to every output hop it could not finalise.  The Python layer checks after
 * every call that returns host arrays and re-runs a failed call on the kernels without in-launch hand-offs.
 * (No counterpart in the reference: base.py:206-216 joins its joblib workers.) */
SG_API int sg_check_errors(sg_handle* h, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355GATE_H */
