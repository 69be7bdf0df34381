// Ragged batches: many recordings of different lengths gated in one call (sg_process_clips, mi355gate.h).
//
// The existing kernels take one Geom per launch -- one window length and one frame count for every unit.  Here
// every unit (one channel of one chunk of one clip: the padded window base.py:144-150 gates as one piece) has its own
// window length Lp and frame count T, and every kernel finds its work through a TILE TABLE (workgroup -> unit or noise
// source, first / last frame or sample).  The number of launches per sub-batch is fixed: it does not depend on the number
// or the lengths of the clips.
//
// This header is shared by api.hip (thin C wrappers, sg_handle) and ragged.hip (tables, kernels); it holds no kernels.
// RgCtx is also what rows.hip and stream.hip take of a handle, and what tile_core.hpp's fill_consts reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/mi355gate.h"

namespace sg {

// what the table-driven paths (ragged.hip, rows.hip, stream.hip) need of a handle (filled by handle.hpp's rg_ctx: sg_handle stays private to the host units that include that header)
struct RgCtx {
  int n, N, W, H, F, FS, padL;       // n_fft, n_fft / 2, win_length, hop, bins, padded bins, zero extension W / 2
  double mag_scale;                  // 1 / sum(w)
  const void* tw64;                  // cx<double>[N]: w_2N^k
  const double* wfull64;             // window embedded in an n_fft frame
  int stationary;
  int64_t cs, pad;                   // chunk_size (units of a longer clip), padding (base.py:66-67)
  int nf, nt;                        // smoothing half widths (0, 0: no smoothing)
  double prop, top_db, n_std, iir_b, nthresh, slope;
  int ddof;
  // profiler hooks (api.hip's ProfScope): begin returns a token that end() closes
  void* hook_ctx;
  void* (*prof_begin)(void* hook_ctx, int stage, hipStream_t st);
  void (*prof_end)(void* token);
};

struct RgState;   // per-handle workspace of the batched path (ragged.hip)
void rg_free(RgState* s);

int rg_workspace_bytes(const RgCtx& c, const sg_noise_src* noise, int32_t n_noise, const sg_clip* clips, int64_t n_clips,
                       int64_t* bytes, std::string* err);
int rg_process(RgState** sp, const RgCtx& c, const void* x_dev, int in_dtype, const void* noise_dev, int noise_dtype,
               const sg_noise_src* noise, int32_t n_noise, const sg_clip* clips, int64_t n_clips, void* out_dev,
               int out_dtype, int64_t max_ws, hipStream_t st, std::string* err);
// thresholds (dB) of the last rg_process call, [n_noise][F] float64; synchronises
int rg_thresholds(RgState* s, double* host, int32_t n_noise, int32_t n_bins, hipStream_t st, std::string* err);
// sub-batches the last call was split into
int64_t rg_last_batches(const RgState* s);

}  // namespace sg
