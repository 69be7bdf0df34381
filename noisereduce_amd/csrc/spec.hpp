// The gated spectrogram (sg_gate_spectrum / sg_gate_spectrum_backward, mi355gate.h): TorchGate.gated_stft.
//
// Y[b][t][k] = rfft(window * frame_t(x_b))[k] * mask[b][t][k], stored as torch.stft stores a spectrogram -- [B][T][F]
// complex, bins contiguous, no padding -- and its adjoint with the mask held fixed.  The mask is sg_process_batch's own
// (api.hip runs the same statistics / decision / smoothing stages and stops before the inverse transform); this unit
// holds the two per-frame kernels and the overlap-add gather of the adjoint.
//
// This header is shared by api.hip (workspace, sub-batches, the C entry points) and spec.hip (kernels); it holds no kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geom.hpp"

namespace sg {

// Frame lengths the kernels are instantiated for: powers of two from 256 to 4096.
bool spec_native(int n_fft);

// tw32: w_n^k, k < n / 2 (cx<float>); win: the analysis window centred in an n_fft frame (float[n]).
// mask: float[units][T][FS], natural bin order.  spec: [units][T][F] complex of `dtype` (SG_F32: float2, SG_F64: double2).
hipError_t spec_forward(const View& v, const Geom& g, int64_t units, const void* tw32, const float* win,
                        const float* mask, void* spec, int dtype, hipStream_t st);

// raw[u][t][f] = bit f of bits[(u T + t) wpr ..] as 0.0f / 1.0f, f < F: the decisions of the bit-mask route as the field the
// float smoothing kernels read (what k_decide writes on the general route).
hipError_t spec_bits_to_raw(const unsigned long long* bits, const Geom& g, int wpr, float* raw, int64_t units, hipStream_t st);

// seg[u][t][0..n) = win * Re sum_{k <= n/2} mask[k] grad[k] e^{+2 pi i k j / n}: the windowed adjoint frames.
hipError_t spec_backward_frames(const Geom& g, int64_t units, const void* tw32, const float* win, const float* mask,
                                const void* grad_spec, int dtype, float* seg, hipStream_t st);

// grad_x[u][p] = sum_t seg[u][t][p + n/2 - t hop], p < L: one thread per sample, frames summed in ascending order (no
// atomics -- the same bits every run).
hipError_t spec_backward_ola(const Geom& g, int64_t units, int64_t L, const float* seg, void* grad_x, int dtype,
                             int64_t gx_stride, hipStream_t st);

}  // namespace sg
