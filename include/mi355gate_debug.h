/*
 * mi355gate_debug.h -- development surface of libmi355gate.so: stage taps for the parity tests, A/B and
 * fault-injection options, per-kernel event timing for bench.py.  Not part of the drop-in boundary
 * (mi355gate.h): nothing here replaces a reference interface, and a caller of the product ABI never needs it.
 * Same library, same handle; the entry points are exported next to the product ones.
 */
#ifndef MI355GATE_DEBUG_H
#define MI355GATE_DEBUG_H

#include "mi355gate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- stage taps (parity tests) ---------------------------------------------------------- */
/* Fields of the last processed unit batch, copied to the host (synchronises):
 * what = 0: raw mask  float[units][T][FS];  1: final mask float[units][T][FS];
 *        2: power     double[units][T][FS] (stationary, materialised path only);
 *        3: raw mask as bits uint64[units][T][ceil(F/64)] (fused stationary path only).
 * FS = third entry of sg_debug_dims. */
SG_API int sg_debug_dims(const sg_handle* h, int64_t dims[3]); /* units, T, FS */
/* Frame range [t0, t1) for which field 3 (mask bits) was computed: the fast path only decides
 * the frames that reach the kept output samples (+- the smoothing half width). */
SG_API int sg_debug_range(const sg_handle* h, int64_t range[2]);
/* Diagnostic counters (synchronises `stream`).  which = 0: (row, band) pairs of the one-kernel TorchGate row gate that were
 * re-evaluated in float64 since the handle was created (the float32 statistics could not decide them within their error
 * bound); divide by rows x 513 for the rate.  which = 1 / 2: batches of the one-pass gate that took the in-kernel / the a-priori
 * floor test (SG_OPT_FLOOR_TEST) since the handle was created (host counters, no synchronisation); which = 3: launch epoch of the
 * last gate call in which some chunk's floor test fired (0: never; synchronises).  which = 4 .. 15: word `which` of the host-mapped
 * error block (synchronises; no kernel of the product library writes these words: 0), except which = 8 in a -DOP_TRACE=1
 * development library of the persistent one-pass gate (tools/trace_onepass.py, tools/ab_persist.py): the unfinished tiles of the
 * last first launch's phase trace, listed on stderr.  which = 16: SG_E_INVALID.  which = 17: the mask smoothing of the last
 * variant-S gate call or sg_process_batch call on the handle, 0 when that call launched none or failed before it (host
 * bookkeeping, no synchronisation; sg_process_rows / sg_process_clips / streams do not route on the widths and leave it alone): bits 0..7 the SG_SMOOTH_* kernel below, bits 8..15 the bytes of the cell it sums in (1 / 2: integer counts,
 * 4 / 8: float / double), bits 16.. the output frames of one of its tiles (0: no tile). */
#define SG_SMOOTH_OFF 1         /* no filter: k_prop_only / k_bits_to_k16 / kx_prop_only, or k_iir_mask<0> before a general smoothing launch */
#define SG_SMOOTH_TILED 2       /* k_smooth_tiled: both float passes in one LDS tile */
#define SG_SMOOTH_SEPARATE 3    /* k_smooth_f + k_smooth_t: two direct passes through global memory */
#define SG_SMOOTH_BITS2 4       /* k_smooth_bits2<uint8_t / uint16_t>: integer sums over decision bits, tile of sm2_tt frames */
#define SG_SMOOTH_BITS 5        /* k_smooth_bits (first generation, n_grad_freq > 30) */
#define SG_SMOOTH_ONEPASS 6     /* k_gate_onepass (n_fft = 1024): MFMA smoothing inside the one-pass gate */
#define SG_SMOOTH_ONEPASS_REG 7 /* k_gate_onepass512 / 256 / 2048 */
#define SG_SMOOTH_ROW_GATE 8    /* k_row_gate (TorchGate rows of <= 64 frames) */
#define SG_SMOOTH_IIR_MASK 9    /* k_iir_mask<nt>, nt >= 1: recurrence, sigmoid and both passes in one kernel */
#define SG_SMOOTH_BOX_MASK 10   /* k_box_mask<nt> (TorchGate, non-stationary, n_movemean = 20) */
#define SG_SMOOTH_X_TILED 11    /* kx_smooth_tiled (float64 pipeline) */
#define SG_SMOOTH_X_SEPARATE 12 /* kx_smooth_f + kx_smooth_t (float64 pipeline) */
/* which = 18: the route of the last sg_gate_spectrum call on the handle, 0 when that call failed before its first spectrum
 * launch (host bookkeeping, no synchronisation; no kernel reads or writes it): bits 0..7 the SG_SPEC_* branch that made the
 * decisions of the last sub-batch, bit 8 SG_SPEC_BITS_TO_RAW, bit 9 SG_SPEC_MASK_DIRECT, bits 16.. the number of sub-batches. */
#define SG_SPEC_ROW_DECIDE 1    /* k_row_decide: statistics, constants and decision bits of a (row, 64 bands) tile, rows of <= 128 frames */
#define SG_SPEC_T2_BITS 2       /* k_t2_rows + k_decide_bits_t2: decision bits of longer rows */
#define SG_SPEC_DECIDE 3        /* stage_decide: the general float decisions */
#define SG_SPEC_BOX_MASK 4      /* stage_box_mask: k_box_mask<nt> (non-stationary, n_movemean = 20) */
#define SG_SPEC_NONSTAT_RAW 5   /* stage_nonstat_raw: the raw sigmoid field, smoothed by the general kernels */
#define SG_SPEC_BITS_TO_RAW 0x100 /* the decision bits went through k_spec_bits_to_raw into the float smoothing kernels */
#define SG_SPEC_MASK_DIRECT 0x200 /* the smoothing wrote straight into the caller's mask buffer (no copy from the workspace) */
/* which = 19: the form of the last noise statistics of fewer than 16 units on the handle (sg_noise_stats, the noise rows of
 * sg_process_batch), 0 when there were none (host bookkeeping, no synchronisation; no kernel reads or writes it). */
#define SG_STATS_THREE_LAUNCH 1 /* k_stft<double>, k_colstats1, k_colstats1_final */
#define SG_STATS_TWO_LAUNCH 2   /* k_noise_moments (transform + slice partials), k_colstats1_final over its slices */
/* which = 20: the form of the floor fix-up of the last one-pass gate call on the handle (the launches behind the gate launch of
 * a call whose floor test ran in the gate kernel, SG_OPT_FLOOR_TEST), 0 when that call took the a-priori test or there was
 * none (host bookkeeping, no synchronisation; no kernel reads or writes it). */
#define SG_FLOOR_ONE_LAUNCH 1 /* k_floor_fix: band maxima and the second gate pass of the chunks that reported, one launch */
#define SG_FLOOR_TWO_LAUNCH 2 /* k_stft_bits<max>, then the gate's REDO instantiation */
SG_API int sg_debug_counter(sg_handle* h, int32_t which, int64_t* value, void* stream);
/* what = 5: the stationary gate's compare constants as the last sg_noise_stats call left them: T2 double[n_bins] (power-domain
 * threshold per band), then the 64 words of the floor-test block (word 2 + b: bit pattern of band block b's float bound on
 * max|x|); bytes = 8 n_bins + 256.  Needs no processed batch. */
SG_API int sg_debug_fetch(sg_handle* h, int32_t what, void* host, int64_t bytes, void* stream);

/* Per-noise-source thresholds in dB of the last sg_process_clips call, [n_noise][n_bins] float64 (stationary gate;
 * stationary.py:79-81 for each source).  Synchronises. */
SG_API int sg_debug_clip_thresholds(sg_handle* h, double* host, int32_t n_noise, int32_t n_bins, void* stream);
/* Sub-batches the last sg_process_clips call was split into. */
SG_API int sg_debug_clip_batches(const sg_handle* h, int64_t* value);
/* Sub-batches the last sg_process_rows / sg_process_rows_backward / sg_gate_spectrum_rows / sg_gate_spectrum_rows_backward
 * call was split into. */
SG_API int sg_debug_rows_batches(const sg_handle* h, int64_t* value);
/* Which kernels the last sg_process_batch_backward / sg_process_rows_backward call on this handle launched (0: none yet).
 * Host bookkeeping only: no kernel reads or writes it. */
#define SG_BWD_ROW 1  /* k_row_backward: a row of at most 64 frames in one workgroup (n_fft = 1024) */
#define SG_BWD_FAST 2 /* k_env_scale + the tiled k_apply_fast (n_fft = 1024) */
#define SG_BWD_REG 3  /* k_env_scale + the register apply kernels (n_fft = 512 / 256 / 2048) */
#define SG_BWD_OLA 4  /* k_env_scale + k_apply_istft + k_ola (every other geometry, or SG_OPT_FORCE_NOFAST) */
#define SG_BWD_ROWS 5 /* rw_backward (sg_process_rows_backward) */
SG_API int sg_debug_backward_route(const sg_handle* h, int64_t* value);

/* ---- development options (sg_set_option / sg_get_option of mi355gate.h) ----------------- */
#define SG_OPT_FORCE_UNFUSED 1 /* value != 0: use the materialised (v1) kernels everywhere */
#define SG_OPT_FORCE_F64_DECIDE 3 /* value != 0: decide every mask cell from a float64 STFT */
#define SG_OPT_FORCE_NOSEAM 4   /* value != 0: overlapping apply tiles instead of abutting tiles + seam kernel */
#define SG_OPT_FORCE_NOLEAN 5   /* value != 0: apply kernel with full-size LDS slices and stored frames */
#define SG_OPT_FORCE_SPLIT 6    /* value != 0: default geometry: decide / smooth / apply as three kernels instead of the one-pass kernel; non-stationary gate: the serial tile chain (k_iir_comb + k_iir_chain) instead of k_iir_chain_par */
#define SG_OPT_INJECT_HANDOFF_FAULT 7 /* tests: the next launch with in-launch hand-offs reports `value` (bits 0..2) as lost hand-offs
                                       * (the output is fine); bits 3..6 make the KERNEL lose its hand-offs (3 or 4: the one-pass
                                       * gate, 5: the fused apply, 6: only the one-launch floor fix-up's wait for a chunk's band maxima,
                                       * which bits 3 and 4 lose too): the producers' tags are never accepted and the polls give up --
                                       * the bounded-poll timeout path itself: error word set by the kernel, affected hops NaN */
#define SG_OPT_FORCE_NOROWGATE 10 /* variant T, stationary, rows of <= 64 frames: 0 (default) = the one-kernel row gate for calls of >= 160
                                   * rows, the four-kernel path (float64 transform of every frame, k_row_decide, k_smooth_bits2,
                                   * k_apply_fast) below; 1 = never the row gate; 2 = the row gate whenever the shape is eligible */
#define SG_OPT_ROWGATE_TAP 11     /* value != 0: the row gate also writes its float32 power tile (4 |X|^2, [rows][64][528]) for
                                   * sg_debug_fetch(what = 4): measurements behind the decision margin */
#define SG_OPT_ROWGATE_SHAPE 12   /* value = 16 (default) or 8: wavefronts per workgroup of the row gate (16 x one quad of frames at 128
                                   * VGPRs, or 8 x two quads at 256 VGPRs without scratch): A/B measurements */
#define SG_OPT_FLOOR_TEST 13      /* one-pass gate (k_gate_onepass): how "can _amp_to_db's -top_db floor lift a band of this chunk over its
                                   * threshold?" is answered.  1 = a priori (k_unit_absmax reads the recording once more before the gate);
                                   * 2 = by the gate kernel on the samples it stages -- free unless a chunk reports, which is then gated a
                                   * second time with its float64 band maxima; 0 (default) = predicted from what recent calls on the handle
                                   * found (no synchronisation).  Same result either way: exact band maxima decide */
#define SG_OPT_TILE_ORDER 15      /* one-pass gate (n_fft = 1024): how workgroups come by their tiles.  0 (default, round 6) = PERSISTENT
                                   * workgroups: three per compute unit, each looping over atomic tickets -- constant tables staged once, the
                                   * next ticket drawn and the next tile's samples prefetched under the current tile's second half (1 % faster
                                   * than 2 for one call at a time; bit-identical).  2 = one ticket-drawn tile per workgroup (rounds 2-5: the better form when SEVERAL
                                   * calls are in flight on their own handles and streams -- persistent workgroups hold every workgroup slot until their launch
                                   * ends: 111 against 97 Gsamples/s at two calls in flight, bench.py --streams; REDO launches, a-priori floor
                                   * flags and the fault-injection instantiation always run this form).
                                   * 1 = tile = block index -- no atomic at all, at the price of assuming that the dispatcher starts workgroups
                                   * in index order (it does on gfx950; HIP does not promise it).  Waits stay bounded and reported in every
                                   * mode; on an otherwise idle GPU the outputs are bit-identical */
#define SG_OPT_EXACT_MATERIALISED 16 /* value != 0: the float64 pipeline (integer outputs, SG_OPT_FORCE_EXACT) as it was before round 5 -- every
                                      * field materialised, the recurrence serial per band, two direct smoothing passes, masked frames + gather --
                                      * also where the fused float64 apply (k_apply_fast64), the tile-parallel recurrence and the LDS-tiled
                                      * smoothing would do: A/B and parity of the two */
#define SG_OPT_STATS_THREE_LAUNCH 17 /* value != 0: the noise statistics of one clip always in three launches (k_stft<double>, k_colstats1,
                                      * k_colstats1_final), also where k_noise_moments + k_colstats1_final would do (variant S, one clip of
                                      * >= 512 frames at n_fft = 256 / 512 / 1024 / 2048, at most 256 slices): A/B and parity of the two.
                                      * Thresholds differ by summation order only */
#define SG_OPT_FLOOR_TWO_LAUNCH 18 /* value != 0: the floor fix-up of a one-pass gate call always as two launches (k_stft_bits<max>, then
                                    * the gate's REDO instantiation), also where the n_fft = 1024 gate would enqueue k_floor_fix once: A/B
                                    * and parity of the two.  Bit-identical output; n_fft = 512 / 256 / 2048 always take the two launches */
#define SG_OPT_FORCE_NOFAST 2  /* value != 0: keep the bit-mask stages but use the general apply kernels */

/* ---- per-kernel timing (bench.py's roofline leg) ------------------------------------- */
#define SG_STAGE_CHANNEL_MEAN 0
#define SG_STAGE_STFT_POWER 1
#define SG_STAGE_COLMAX 2
#define SG_STAGE_COLSTATS 3
#define SG_STAGE_DECIDE 4
#define SG_STAGE_STFT_MAG 5
#define SG_STAGE_NONSTAT_MASK 6
#define SG_STAGE_SMOOTH 7
#define SG_STAGE_APPLY_ISTFT 8
#define SG_STAGE_OLA 9
#define SG_STAGE_NOISE_STATS 10 /* every launch of sg_noise_stats */
#define SG_STAGE_PREP 11
#define SG_STAGE_STFT_MAX 12
#define SG_STAGE_STFT_BITS 13
#define SG_STAGE_APPLY_FAST 14
#define SG_STAGE_DECIDE_FAST 15
#define SG_STAGE_ONEPASS 16
#define SG_STAGE_ROW_GATE 17   /* k_row_gate: TorchGate.forward of a whole row (<= 64 frames) in one kernel */
#define SG_STAGE_IIR_CHAIN 18 /* non-stationary gate: carries of the time tiles (k_iir_chain_par; serial form k_iir_part / k_iir_comb + k_iir_chain) */
#define SG_STAGE_IIR_MASK 19  /* non-stationary gate: k_iir_mask<nt> -- recurrence, sigmoid and both smoothing passes in one kernel */
/* ragged batches (sg_process_clips, ragged.hip): one launch of each per sub-batch.  sg_process_rows (rows.hip) books its
 * launches under the same seven stages (its moving mean under SG_STAGE_RG_IIR), and so does sg_gate_spectrum_rows: its
 * spectrum store and its adjoint frames under SG_STAGE_RG_APPLY, the adjoint's overlap-add under SG_STAGE_RG_OLA.
 * sg_gate_features_rows books its feature store and its adjoint frames the same way. */
#define SG_STAGE_RG_NOISE_POWER 20 /* stationary: float64 transform of every noise frame */
#define SG_STAGE_RG_NOISE_FINAL 21 /* stationary: per-source band maxima, moments, thresholds, compare constants */
#define SG_STAGE_RG_DECIDE 22      /* float64 transform of every data frame: decision bits + band maxima (stationary) / magnitudes */
#define SG_STAGE_RG_IIR 23         /* non-stationary: one-pole filtfilt over each unit's frames + sigmoid */
#define SG_STAGE_RG_FSMOOTH 24     /* mask smoothing along frequency (with the -top_db floor override, stationary) */
#define SG_STAGE_RG_APPLY 25       /* smoothing along time + masked multiply + inverse transform of every live frame */
#define SG_STAGE_RG_OLA 26         /* overlap-add of the kept samples */
#define SG_N_STAGES 27
/* stages beyond the 27 every reader of sg_profile_read(..., SG_N_STAGES, ...) knows: state transfer of stream banks */
#define SG_STAGE_ST_EXPORT 27      /* k_st_export (sg_stream_export): one launch per call */
#define SG_STAGE_ST_IMPORT 28      /* k_st_import (sg_stream_import): one launch per call */
#define SG_N_STAGES_ALL 29
/* When enabled, every kernel launch is bracketed by a hipEvent pair recorded on the launch
 * stream.  sg_profile_read synchronises those events and returns accumulated milliseconds
 * and launch counts per stage (arrays of n_stages = SG_N_STAGES, or SG_N_STAGES_ALL with the
 * stages above); reset != 0 clears the accumulators of every stage. */
SG_API int sg_profile_enable(sg_handle* h, int32_t on);
/* Restrict the event pairs to the stages whose bit (1 << SG_STAGE_*) is set; 0 = all stages.  Timing
 * one kernel costs two event records per step instead of ~30. */
SG_API int sg_profile_select(sg_handle* h, int64_t stage_mask);
SG_API int sg_profile_read(sg_handle* h, double* ms, int64_t* counts, int32_t n_stages, int32_t reset);
SG_API const char* sg_stage_name(int32_t stage);

#ifdef __cplusplus
}
#endif
#endif /* MI355GATE_DEBUG_H */
