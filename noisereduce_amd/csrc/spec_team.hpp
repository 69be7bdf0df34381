// The merge the adjoint kernels of spec.hip (gated spectrogram) and feat.hip (gated filterbank features) share: a Hermitian
// half spectrum into the half-size complex spectrum the inverse transform of fft_wave.hpp takes.
#pragma once
#include <hip/hip_runtime.h>

#include "fft_wave.hpp"

namespace sg {

// The merge of k_apply_istft.  Y is the Hermitian half (bins 0 .. N) of a length-2N spectrum; the un-normalised half-size
// inverse transform of the merged buffer is N * irfft(Y).  Bins 0 and N are real: y0, yN.
__device__ __forceinline__ void merge_dc(cx<float>* buf, float y0, float yN) {
  buf[0] = {0.5f * (y0 + yN), 0.5f * (y0 - yN)};
}
// Bins k and N - k, 0 < k <= N / 2, with w = tw[k].
__device__ __forceinline__ void merge_pair(cx<float>* buf, cx<float> w, int k, int N, cx<float> Yk, cx<float> Yn) {
  // merge: E' = (Yk + conj Yn)/2 ; O' = (Yk - conj Yn)/2 * conj(w) ; Zc'[k] = E' + i O'
  const cx<float> Ep = {(Yk.x + Yn.x) * 0.5f, (Yk.y - Yn.y) * 0.5f};
  const cx<float> D = {(Yk.x - Yn.x) * 0.5f, (Yk.y + Yn.y) * 0.5f};
  const cx<float> wc = {w.x, -w.y};
  const cx<float> Op = cmul(D, wc);
  buf[k] = {Ep.x - Op.y, Ep.y + Op.x};
  if (k != N - k) buf[N - k] = {Ep.x + Op.y, -Ep.y + Op.x};   // Zc'[N-k] = conj(E') + i conj(O')
}

}  // namespace sg
