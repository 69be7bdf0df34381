// Banks of live streams (sg_stream_*, mi355gate.h): the stationary gate, or the non-stationary gate with a bounded
// lookahead, advanced block by block.
//
// A bank holds n_slots independent streams of `channels` channels each.  Every step (sg_stream_push) takes whatever block
// each pushed stream received and runs a FIXED number of launches, whatever the number of streams and the block lengths;
// the state that survives between steps lives in HBM and belongs to the bank:
//   ring   [unit][RC]          float64 samples not yet covered by an applied frame (RC = W + (nt + 1) H)
//   bits   [unit][RB][wpr]     final raw-mask bits of the last decided frames (causal -top_db floor already applied)
//   rmax   [unit][FS]          running band maximum of the power, float64, NaN-sticky
//   carry  [unit][2][W]        partial overlap-add sums of the samples not yet emitted (double buffered per step)
//   thr/T2 [slot][FS]          threshold in dB and its compare constant on the raw power
// A non-stationary bank (lookahead L frames; no thresholds) holds instead of bits / rmax / thr / T2:
//   fst    [unit][FS]          forward one-pole state fwd[f, last transformed frame], float64
//   fa     [unit][RF][2][FS]   A = |X| and fwd of the last transformed frames, float64 (RF = L + 1 + frames of max_block)
//   mk     [unit][RB][FS]      raw sigmoid mask rows, float32 -- float64 in an exact bank -- (RB = 2 nt + 1 + L + frames of
//                              max_block)
// and its ring is RC = W + (nt + L + 1) H samples.
// A box bank (a handle of variant T: TorchGate's non-stationary gate, the level a moving mean over K = Lb + 1 + L frames) is
// a non-stationary bank without fst and without the fwd half of fa:
//   fa     [unit][RF][FS]      A = |X| of the last transformed frames AND of the Lb frames behind the next one to decide,
//                              float64 (RF = L + Lb + 1 + frames of max_block)
// (DESIGN section 13h).
// An adaptive bank (the stationary gate with the noise profile learnt from the stream itself) holds no thr / T2 but
//   nst    [unit][3][FS]       Wn, mu, M2: weight sum, mean and weighted squared deviations of the floored dB values, float64
// (unit = slot * channels + channel).  Of a slot the bank remembers n, the samples received (and which carry buffer is
// current, and whether a threshold is set): t_dec, t_applied and E are functions of n, stated once (stream_plan.hpp's
// st_counters_at).  That header holds all host arithmetic of a bank -- counters, the bytes of every buffer (StLayout), the
// checks and the plan of a step -- as plain C++ without HIP.
// st_export / st_import move the live part of all this between banks of the same gate.
//
// The frame work of the kernels is tile_core.hpp's, shared with the clips and the rows.
// This header is shared by api.hip (thin C wrappers) and stream.hip (tables, kernels); it holds no kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/mi355gate.h"
#include "ragged.hpp"   // RgCtx
#include "stream_plan.hpp"

namespace sg {

struct StBank;

// an adaptive bank's estimate: forgetting factor per frame in (0, 1], frames that update it (>= 1; negative: all)
struct StAdaptive {
  double forget;
  int64_t learn_frames;
};

// ns: a non-stationary bank with `lookahead` frames (the handle must be non-stationary); else lookahead is ignored.
// ad: non-null for an adaptive bank (the handle must be stationary)
// box_k: non-zero for a box bank (TorchGate's non-stationary gate: the level is the moving mean over box_k frames; ns must be
// set, `lookahead` is ignored: it is box_k - 1 - (box_k - 1) / 2; the handle may be of variant T, its window is re-embedded)
// exact: float64 segments (and, non-stationary, float64 mk rows): the bank takes and returns every sample type, each
// exactly (sg_stream_create_ex)
int st_create(StBank** out, const RgCtx& c, int32_t n_slots, int32_t channels, int64_t max_block, bool ns, int32_t lookahead,
              const StAdaptive* ad, bool exact, std::string* err, int32_t box_k = 0);
// bytes of device state st_create allocates for such a bank (host arithmetic)
int64_t st_state_bytes(const RgCtx& c, bool ns, int64_t n_slots, int64_t channels, int64_t max_block, int64_t L,
                       bool adaptive = false, bool exact = false, int32_t box_k = 0);
// adaptive banks: the threshold (dB) after the last decided frame of every channel of `slot`, channels x F values, NaN
// where no frame was decided yet.  Synchronises the stream.
int st_noise_profile(StBank* b, int32_t slot, double* thresh_host, hipStream_t st, std::string* err);
// samples a stream of this bank has emitted after n received: st_emitted with nt + lookahead
int64_t st_bank_emitted(const StBank* b, int64_t n);
// frames a stream of this bank has applied after n received: max(0, t_dec(n) - nt - lookahead + 1)
int64_t st_bank_frames(const StBank* b, int64_t n);
void st_destroy(StBank* b);
// thresh_dev: F dB values on the device (the handle's); thresh_host: F dB values on the host; exactly one is non-null
int st_set_threshold(StBank* b, const int32_t* slots, int32_t n, const double* thresh_dev, const double* thresh_host,
                     hipStream_t st, std::string* err);
// so == fo == nullptr: sg_stream_push.  Otherwise the same plan and launches, the apply launch in its spectrum-storing
// form (so) or its feature form (fo); at most one of the two is non-null
int st_push(StBank* b, const void* in_dev, int in_dtype, void* out_dev, int out_dtype, const sg_stream_rec* recs,
            int32_t n_recs, hipStream_t st, std::string* err, const StSpecOut* so = nullptr, const StFeatOut* fo = nullptr);
// the bank's own filterbank (sg_stream_set_filterbank): fb_host float[F][M]; the device tables are feat_tables.hpp's four
// arrays, owned by the bank.  Synchronises the device when it replaces a filterbank; a refused one leaves the earlier in place
int st_set_filterbank(StBank* b, const float* fb_host, int32_t n_filters, std::string* err);
int st_reset(StBank* b, const int32_t* slots, int32_t n, hipStream_t st, std::string* err);
int st_counters(const StBank* b, int32_t slot, int64_t* n, int64_t* emitted, std::string* err);
// state transfer (sg_stream_export_bytes / _export / _import): `sig` carries the handle's part of the signature (the gate's
// parameters); the bank's part, the counters and the payload size are filled in / checked here.  One launch each.
int st_export_bytes(const StBank* b, int32_t slot, int64_t* bytes, std::string* err);
// the payload size a header's signature and n give: no bank, no device
int st_head_bytes(const sg_stream_head& hd, int64_t* bytes);
int st_export(StBank* b, const int32_t* slots, int32_t n, void* blob_dev, const int64_t* offsets, const sg_stream_head& sig,
              sg_stream_head* heads, hipStream_t st, std::string* err);
int st_import(StBank* b, const int32_t* slots, int32_t n, const void* blob_dev, const int64_t* offsets, const sg_stream_head& sig,
              const sg_stream_head* heads, hipStream_t st, std::string* err);

}  // namespace sg
