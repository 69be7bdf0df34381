// Padded batches of different-length rows (sg_process_rows / sg_process_rows_backward, sg_gate_spectrum_rows /
// sg_gate_spectrum_rows_backward, sg_gate_features_rows / sg_gate_features_rows_backward, mi355gate.h): TorchGate.forward,
// TorchGate.gated_stft and TorchGate.gated_filterbank on a (B, L) tensor whose row i holds lengths[i] samples of audio and
// padding after them.
//
// sg_process_batch takes one Geom per launch -- one length and one frame count for every row.  Here every row has its
// own length, frame count T_i = 1 + len_i / hop and output length hop * (len_i / hop), and every kernel finds its work
// through a TILE TABLE (workgroup -> row or noise row, first / last frame, band or sample): the number of launches per
// sub-batch is fixed, whatever the batch size and the lengths.  The frame work is tile_core.hpp's.
//
// This header is shared by api.hip (thin C wrappers, sg_handle) and rows.hip (tables, kernels); it holds no kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "feat.hpp"     // FeatBank
#include "ragged.hpp"   // RgCtx

namespace sg {

struct RwState;   // per-handle workspace of the rows path (rows.hip)
void rw_free(RwState* s);

// c: the handle's geometry and gate parameters (RgCtx; cs / pad / iir_b unused); kbox: moving-mean length of the
// non-stationary gate.  lengths / xn_lengths: host arrays or nullptr (every row full).  mask_out: nullptr or
// float[B][1 + L / H][FS].  max_ws: sub-batch budget in bytes (<= 0: 4 GiB).
int rw_process(RwState** sp, const RgCtx& c, int kbox, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
               const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
               const int64_t* xn_lengths, void* out_dev, int out_dtype, int64_t out_stride, float* mask_out,
               int64_t max_ws, hipStream_t st, std::string* err);
// adjoint with the mask fixed: grad_out (B, H * (L / H)) -> grad_x (B, L); mask: what rw_process wrote
int rw_backward(RwState** sp, const RgCtx& c, const void* go_dev, int dtype, int64_t B, int64_t L, int64_t go_stride,
                const int64_t* lengths, const float* mask, void* gx_dev, int64_t gx_stride, int64_t max_ws,
                hipStream_t st, std::string* err);
// The gated spectrogram of the padded batch (sg_gate_spectrum_rows): rw_process up to and including the mask smoothing
// along frequency -- the same launches with the same arguments, so mask_out holds the same bits -- then X * mask stored
// as spec [B][1 + L / H][F] complex of `dtype` instead of the inverse transform and the overlap-add.  Frames at or beyond
// T_i are stored as zeros; nothing is loaded for them.
int rw_spectrum(RwState** sp, const RgCtx& c, int kbox, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
                const int64_t* xn_lengths, void* spec_dev, float* mask_out, int64_t max_ws, hipStream_t st,
                std::string* err);
// its adjoint with the mask fixed: grad_spec [B][1 + L / H][F] complex of dtype -> grad_x (B, L), zero at and beyond
// lengths[i]; frames at or beyond T_i of grad_spec are never read.  No envelope division, no atomics.
int rw_spectrum_backward(RwState** sp, const RgCtx& c, const void* gs_dev, int dtype, int64_t B, int64_t L,
                         const int64_t* lengths, const float* mask, void* gx_dev, int64_t gx_stride, int64_t max_ws,
                         hipStream_t st, std::string* err);
// The filterbank features of the padded batch (sg_gate_features_rows): rw_spectrum's launches up to
// and including the mask smoothing along frequency -- mask_out holds the same bits -- then
// lin[m] = sum_k fb[k][m] (|X[k]| mask[k])^power (or ln(lin + eps)) stored as feat [B][1 + L / H][M] of `dtype`, in
// float64 and rounded once, while the frame is in LDS.  Frames at or beyond T_i hold 0 (ln(eps)); nothing is loaded for
// them.  bank: the handle's (feat.hpp).  SG_E_INVALID without a bank or for a power other than 1 or 2.
int rw_features(RwState** sp, const RgCtx& c, int kbox, const FeatBank& bank, const void* x_dev, int dtype, int64_t B,
                int64_t L, int64_t x_stride, const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln,
                int64_t xn_stride, const int64_t* xn_lengths, int power, int take_log, double eps, void* feat_dev,
                float* mask_out, int64_t max_ws, hipStream_t st, std::string* err);
// its adjoint w.r.t. x with the mask and the bank fixed: grad_feat [B][1 + L / H][M] of dtype -> grad_x (B, L), zero at
// and beyond lengths[i]; the frames are transformed again from x; frames at or beyond T_i of grad_feat are never read.
// No atomics.
int rw_features_backward(RwState** sp, const RgCtx& c, const FeatBank& bank, const void* x_dev, int dtype, int64_t B,
                         int64_t L, int64_t x_stride, const int64_t* lengths, const void* grad_feat_dev, const float* mask,
                         int power, int take_log, double eps, void* gx_dev, int64_t gx_stride, int64_t max_ws,
                         hipStream_t st, std::string* err);
// sub-batches the last call was split into
int64_t rw_last_batches(const RwState* s);

}  // namespace sg
