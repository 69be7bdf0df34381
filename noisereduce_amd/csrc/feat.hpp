// Gated filterbank features (sg_set_filterbank / sg_gate_features / sg_gate_features_backward, mi355gate.h):
// TorchGate.gated_filterbank.
//
// lin[b][t][m] = sum_k fb[k][m] * (|X[b][t][k]| * mask[b][t][k]) ^ power, power 1 or 2, and optionally ln(lin + eps), stored
// [B][T][M] with the filters contiguous -- the spectrogram of spec.hpp reduced over the filters' supports while the frame
// is still in LDS, and the adjoint w.r.t. x with mask and filterbank held fixed.  The mask is sg_process_batch's own, as in
// spec.hpp.
//
// This header is shared by api.hip (sub-batches, the C entry points; the bank's tables come from feat_tables.hpp) and feat.hip
// (kernels); it holds no kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geom.hpp"

namespace sg {

constexpr int FEAT_MAX_FILTERS = 1024;

// The uploaded bank.  fb: float[F][M]; fbT: float[M][F]; khull: int2[M], the hull [k_lo, k_hi) of filter m's non-zero bins
// (0, 0 for an all-zero filter); mhull: int2[F], the hull [m_lo, m_hi) of the filters that are non-zero at bin k.
struct FeatBank {
  const float* fb;
  const float* fbT;
  const int2* khull;
  const int2* mhull;
  int32_t M;
};

// tw32, win, mask as spec_forward.  feat: [units][T][M] of `dtype` (SG_F32: float, SG_F64: double; the sums run in that type).
hipError_t feat_forward(const View& v, const Geom& g, int64_t units, const void* tw32, const float* win, const float* mask,
                        const FeatBank& bank, int power, int take_log, double eps, void* feat, int dtype, hipStream_t st);

// seg[u][t][0..n) = win * Re sum_{k <= n/2} G[k] e^{+2 pi i k j / n} with G = dL/dX, formed from grad_feat [units][T][M] of
// `dtype` and the frame's own re-computed spectrum: the windowed adjoint frames spec_backward_ola gathers.
hipError_t feat_backward_frames(const View& v, const Geom& g, int64_t units, const void* tw32, const float* win,
                                const float* mask, const FeatBank& bank, int power, int take_log, double eps,
                                const void* grad_feat, int dtype, float* seg, hipStream_t st);

}  // namespace sg
