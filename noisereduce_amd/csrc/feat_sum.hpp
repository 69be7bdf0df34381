// The filter sum of the feature kernels, shared by rows_feat.hip (padded batches) and stream.hip (live
// streams): the power of one bin, the float64 sum of one filter over its hull in a fixed order, and the
// one rounding at the store.  Device code only; it holds no kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_wave.hpp"   // cx
#include "feat.hpp"

namespace sg {

// p = (|X| m)^power of one bin, in float64
__device__ __forceinline__ double feat_power(cx<double> X, double m, int power) {
  const double re = X.x * m, im = X.y * m;
  const double s = re * re + im * im;
  return power == 2 ? s : sqrt(s);
}
// lin[m] = sum_k fbT[m][k] p[k] over the hull of filter m, ascending k, in float64.  p_at(k): p[k] for k < N; pN: p[N]
template <class PAt>
__device__ __forceinline__ double feat_filter_sum(const FeatBank& bank, int F, int m, PAt&& p_at, double pN) {
  const int2 hull = bank.khull[m];
  const float* __restrict__ row = bank.fbT + (int64_t)m * F;
  const int hi = hull.y < F ? hull.y : F - 1;
  double acc = 0.0;
  int k = hull.x;
  // eight weights in flight at a time (a rolled loop waits for each global load in turn); the sum keeps its order
  for (; k + 8 <= hi; k += 8) {
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = row[k + j];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += (double)w[j] * p_at(k + j);
  }
  for (; k < hi; ++k) acc += (double)row[k] * p_at(k);
  if (hull.y == F) acc += (double)row[F - 1] * pN;
  return acc;
}
// The lane index as a value the optimiser cannot see through (feat.hip's): the addresses formed from it -- mask, bank and
// output rows -- are then computed where they are used, after the transform, instead of once before the frame loop and
// held in registers across it (the difference between two and three waves per SIMD at n_fft = 512 and 1024).
__device__ __forceinline__ int fresh_lane(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}
__device__ __forceinline__ void feat_store(void* out, int dtype, int64_t e, double v) {
  if (dtype == 1) ((double*)out)[e] = v;
  else ((float*)out)[e] = (float)v;
}

}  // namespace sg
