// Kernels of the gated filterbank features (feat.hpp; sg_gate_features / sg_gate_features_backward).
//
// Both kernels keep the team shapes, the twiddle staging and the frames-per-workgroup loop of spec.hip's k_spec_fwd, so a
// workgroup covers the same frames (SPEC_Q of the tests); the frame never leaves LDS between the transform and the features.
//
//   k_feat_fwd   window -> FFT -> split -> p[k] = (|X[k]| mask[k])^power, in place -> lane m sums
//                fbT[m][k] p[k] over the hull of filter m -> optionally ln(. + eps) -> store; consecutive lanes store
//                consecutive filters.
//   k_feat_bwd   the same front end (the frame is transformed again: nothing of size B x T x F is saved but the mask), then
//                g'[m] = grad[m] (/ (lin[m] + eps)) into a per-team row, gp[k] = sum_m fb[k][m] g'[m] over the hull of bin k,
//                G[k] = gp[k] d(|X| mask)^power / dX, merged in place (spec_team.hpp), inverse FFT, * window -> seg.
//
// Where p lives.  A lane that split one bin at a time could not write p over the transform buffer: bin k reads buf[k] and
// buf[N - k].  The forward therefore splits the PAIR (k, N - k) in one lane, as the adjoint merge does: both bins come from
// buf[k] and buf[N - k] and both powers go back into the real parts of those two cells (bins 0 and N into the two halves of
// buf[0]), so k_feat_fwd needs no LDS beyond k_spec_fwd's and keeps its workgroups per CU at every frame length.  The
// backward needs the spectrum again after lin[m] (log only), so there p is a float row of its own, N + 1 floats per team
// (odd stride: the teams of a workgroup start in different banks), next to the M floats of g'.  A mel filter's hull is a
// few dozen bins and neighbouring lanes read neighbouring, overlapping stretches of p; a dense bank reads p[k] as a
// broadcast.
#include <hip/hip_runtime.h>

#include "feat.hpp"
#include "fft_wave.hpp"
#include "geom.hpp"
#include "launch.hpp"
#include "spec_team.hpp"

namespace sg {

namespace {

// The rows a launch reads, cut down from the View of api.hip to what full rows need (sample s of row r is
// x[r * stride + s], 0 <= s < L; row0: the sub-batch's first row).
struct FeatRows {
  const void* x;
  int dtype;
  int64_t stride, L, row0;
};

// the team shapes and frames per workgroup of spec.hip, restated (tests/test_gated_filterbank_host.py compares the two files)
template <int N>
constexpr int spec_nt() { return N >= 2048 ? 256 : (N <= 128 ? 16 : (N == 256 ? 32 : 64)); }
template <int N>
constexpr int spec_teams() { return N >= 2048 ? 1 : (spec_nt<N>() < 64 ? 256 / spec_nt<N>() : (N * sizeof(cx<float>) > 16384 ? 2 : 4)); }
constexpr int SPEC_FPW = 4;   // frames per team and workgroup: the twiddle table is staged once for all of them

// window * frame t of row `r` as complex pairs (x[2j], x[2j+1]) into buf; samples outside the row are torch.stft's zero
// padding, an invalid frame is all zero (k_spec_fwd's loads, on full rows: the View's window is the row)
template <int N, int NT>
__device__ __forceinline__ void load_frame(cx<float>* buf, const FeatRows& in, const Geom& g, int64_t r, int64_t t, bool valid,
                                           const float* __restrict__ win, int lane) {
  // the window through a scalar base and unsigned 32-bit indices: one offset register per load instead of a 64-bit address
  // per load held across the whole frame loop
  const float2* __restrict__ w2 = reinterpret_cast<const float2*>(win);
  const int64_t s0 = t * g.H - g.padL;
  const bool direct = valid && in.dtype == 0 && s0 >= 0 && s0 + 2 * N <= in.L;  // team-uniform
  if (direct) {
    const float* fp = (const float*)in.x + r * in.stride + s0;
    for (unsigned j = lane; j < (unsigned)N; j += NT) {
      const float2 w = w2[j];
      buf[j] = {fp[2 * j] * w.x, fp[2 * j + 1] * w.y};
    }
  } else {
    for (unsigned j = lane; j < (unsigned)N; j += NT) {
      cx<float> z = {0.f, 0.f};
      const float2 w = w2[j];
      const int64_t s = s0 + 2 * j;
      if (valid && s >= 0 && s < in.L) z.x = (float)load_sample(in.x, in.dtype, r * in.stride + s) * w.x;
      if (valid && s + 1 >= 0 && s + 1 < in.L) z.y = (float)load_sample(in.x, in.dtype, r * in.stride + s + 1) * w.y;
      buf[j] = z;
    }
  }
}

// The lane index as a value the optimiser cannot see through.  Addresses formed from it are then computed where they are
// used, in every pass of the frame loop, instead of once before the loop and held in registers across the transforms (a
// dozen 64-bit window and table addresses: the difference between three and four waves per SIMD).
__device__ __forceinline__ int fresh(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

template <bool POW2>
__device__ __forceinline__ float bin_power(cx<float> X, float m) {
  const float re = X.x * m, im = X.y * m;
  const float s = re * re + im * im;
  return POW2 ? s : sqrtf(s);
}

// p[k] = (|X[k]| mask[k])^power, k <= N, from the transformed half-size frame into a row of its own (the backward)
template <int N, int NT, bool POW2>
__device__ __forceinline__ void power_row(float* prow, const cx<float>* buf, const cx<float>* tw, const float* __restrict__ Mrow,
                                          int lane) {
  for (int k = lane; k <= N; k += NT) {
    const cx<float> a = buf[k == N ? 0 : k];
    const cx<float> b = buf[(k == 0 || k == N) ? 0 : N - k];
    prow[k] = bin_power<POW2>(rfft_bin(a, b, tw[k == N ? 0 : k], k, N), Mrow[k]);
  }
}

// ... and in place (the forward): p[k] into buf[k].x for 0 <= k < N, p[N] into buf[0].y; a lane owns both cells it touches
template <int N, int NT, bool POW2>
__device__ __forceinline__ void power_in_place(cx<float>* buf, const cx<float>* tw, const float* __restrict__ Mrow, int lane) {
  for (int k = lane; k <= N / 2; k += NT) {
    if (k == 0) {
      const cx<float> a = buf[0];
      buf[0] = {bin_power<POW2>(rfft_bin(a, a, tw[0], 0, N), Mrow[0]), bin_power<POW2>(rfft_bin(a, a, tw[0], N, N), Mrow[N])};
    } else {
      const cx<float> a = buf[k], b = buf[N - k];
      const float pk = bin_power<POW2>(rfft_bin(a, b, tw[k], k, N), Mrow[k]);
      const float pn = bin_power<POW2>(rfft_bin(b, a, tw[N - k], N - k, N), Mrow[N - k]);
      buf[k].x = pk;
      if (k != N - k) buf[N - k].x = pn;
    }
  }
}

// lin[m] = sum_k fbT[m][k] p[k] over the filter's hull, in ascending k, accumulated in T.  p[k] = p[S k] for k < n_half and
// pN for the last bin (S = 1, pN = p[n_half]: a row; S = 2, pN = p[1]: in place)
template <typename T, int S>
__device__ __forceinline__ T filter_sum(const FeatBank& bank, int F, int m, const float* p, float pN) {
  const int2 hull = bank.khull[m];
  const float* __restrict__ row = bank.fbT + (int64_t)m * F;
  const int hi = hull.y < F ? hull.y : F - 1;
  T acc = (T)0;
  for (int k = hull.x; k < hi; ++k) acc += (T)row[k] * (T)p[S * k];
  if (hull.y == F) acc += (T)row[F - 1] * (T)pN;
  return acc;
}

// G[k] = gp[k] d(|X| mask)^power / dX with gp[k] = sum_m fb[k][m] g'[m] over the bin's hull, in ascending m
template <bool POW2>
__device__ __forceinline__ cx<float> bin_grad(const FeatBank& bank, int k, const float* grow, cx<float> X, float m) {
  const int2 hull = bank.mhull[k];
  const float* __restrict__ row = bank.fb + (int64_t)k * bank.M;
  float gp = 0.f;
  for (int j = hull.x; j < hull.y; ++j) gp += row[j] * grow[j];
  float s;
  if (POW2) {
    s = 2.0f * gp * m * m;
  } else {
    const float a = sqrtf(X.x * X.x + X.y * X.y);
    s = a > 0.f ? gp * m / a : 0.f;   // the derivative of |X| at 0 is defined as 0
  }
  return {s * X.x, s * X.y};
}

}  // namespace

template <int N, int WAVES, int FPW, int NT, typename TO, bool POW2, bool LOG>
__global__ __launch_bounds__(WAVES * NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_feat_fwd(FeatRows in, Geom g, const cx<float>* __restrict__ tw_g,
                                                         const float* __restrict__ win, const float* __restrict__ mask,
                                                         FeatBank bank, double eps, TO* __restrict__ feat) {
  constexpr int SY = NT <= 64 ? 1 : NT;   // a team of <= 64 lanes is (part of) one wavefront and its buffers are its own
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<float>* tw = reinterpret_cast<cx<float>*>(smem);
  cx<float>* bufs = tw + N;
  const int lane = threadIdx.x % NT;
  const int wave = threadIdx.x / NT;
  cx<float>* buf = bufs + wave * N;
  const float* p = reinterpret_cast<const float*>(buf);   // after power_in_place: p[2 k], k < N, and p[1] for bin N
  stage_twiddles<WAVES * NT, N>(tw, tw_g, (int)threadIdx.x);
  const int64_t u = blockIdx.y;
  const int64_t row = in.row0 + u;
  const int M = bank.M;
  __syncthreads();
#pragma unroll 1
  for (int fi = 0; fi < FPW; ++fi) {
    const int64_t t = ((int64_t)blockIdx.x * FPW + fi) * WAVES + wave;
    const bool valid = t < g.T;
    load_frame<N, NT>(buf, in, g, row, t, valid, win, fresh(lane));
    team_sync<SY>();
    wave_fft<float, N, false, NT, SY>(buf, tw, lane);
    const int ln = fresh(lane);
    if (valid) power_in_place<N, NT, POW2>(buf, tw, mask + (u * g.T + t) * g.FS, ln);
    team_sync<SY>();
    if (valid) {
      TO* frow = feat + (u * g.T + t) * M;
#pragma unroll 1
      for (int m = ln; m < M; m += NT) {
        const TO lin = filter_sum<TO, 2>(bank, g.F, m, p, p[1]);
        frow[m] = LOG ? (TO)log((double)lin + eps) : lin;
      }
    }
    team_sync<SY>();
  }
}

template <int N, int WAVES, int FPW, int NT, typename TI, bool POW2, bool LOG>
__global__ __launch_bounds__(WAVES * NT) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_feat_bwd(FeatRows in, Geom g, const cx<float>* __restrict__ tw_g,
                                                         const float* __restrict__ win, const float* __restrict__ mask,
                                                         FeatBank bank, double eps, const TI* __restrict__ grad,
                                                         float* __restrict__ seg) {
  constexpr int SY = NT <= 64 ? 1 : NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<float>* tw = reinterpret_cast<cx<float>*>(smem);
  cx<float>* bufs = tw + N;
  const int lane = threadIdx.x % NT;
  const int wave = threadIdx.x / NT;
  const int M = bank.M;
  cx<float>* buf = bufs + wave * N;
  float* prow = reinterpret_cast<float*>(bufs + WAVES * N) + wave * (N + 1);
  float* grow = reinterpret_cast<float*>(bufs + WAVES * N) + (LOG ? WAVES * (N + 1) : 0) + wave * M;   // no p row without log
  stage_twiddles<WAVES * NT, N>(tw, tw_g, (int)threadIdx.x);
  const int64_t u = blockIdx.y;
  const int64_t row = in.row0 + u;
  __syncthreads();
#pragma unroll 1
  for (int fi = 0; fi < FPW; ++fi) {
    const int64_t t = ((int64_t)blockIdx.x * FPW + fi) * WAVES + wave;
    const bool valid = t < g.T;
    const float* Mrow = mask + (u * g.T + (valid ? t : 0)) * g.FS;
    load_frame<N, NT>(buf, in, g, row, t, valid, win, fresh(lane));
    team_sync<SY>();
    wave_fft<float, N, false, NT, SY>(buf, tw, lane);
    const int ln = fresh(lane);
    if (LOG) {   // lin[m] as the forward formed it
      if (valid) power_row<N, NT, POW2>(prow, buf, tw, Mrow, ln);
      team_sync<SY>();
    }
    if (valid) {
      const TI* gr = grad + (u * g.T + t) * M;
#pragma unroll 1
      for (int m = ln; m < M; m += NT) {
        TI gm = gr[m];
        if (LOG) gm = (TI)((double)gm / ((double)filter_sum<TI, 1>(bank, g.F, m, prow, prow[N]) + eps));
        grow[m] = (float)gm;
      }
    }
    team_sync<SY>();
    if (valid) {
      // bins k and N - k come from buf[k] and buf[N - k] and their merge goes back to the same two cells: in place
      for (int k = ln; k <= N / 2; k += NT) {
        if (k == 0) {
          const cx<float> a = buf[0];
          const cx<float> G0 = bin_grad<POW2>(bank, 0, grow, rfft_bin(a, a, tw[0], 0, N), Mrow[0]);
          const cx<float> GN = bin_grad<POW2>(bank, N, grow, rfft_bin(a, a, tw[0], N, N), Mrow[N]);
          merge_dc(buf, 2.0f * G0.x, 2.0f * GN.x);
        } else {
          const cx<float> a = buf[k], b = buf[N - k];
          const cx<float> w = tw[k];
          const cx<float> Gk = bin_grad<POW2>(bank, k, grow, rfft_bin(a, b, w, k, N), Mrow[k]);
          const cx<float> Gn = bin_grad<POW2>(bank, N - k, grow, rfft_bin(b, a, tw[N - k], N - k, N), Mrow[N - k]);
          merge_pair(buf, w, k, N, Gk, Gn);   // G is the gradient w.r.t. X already: the merge takes it with mask 1
        }
      }
    }
    team_sync<SY>();
    wave_fft<float, N, true, NT, SY>(buf, tw, lane);
    if (valid) {
      float2* srow = reinterpret_cast<float2*>(seg + (u * g.T + t) * (int64_t)g.n);
      const float2* __restrict__ w2 = reinterpret_cast<const float2*>(win);
      for (unsigned j = fresh(lane); j < (unsigned)N; j += NT) {
        const cx<float> z = buf[j];
        const float2 w = w2[j];
        srow[j] = make_float2(z.x * w.x, z.y * w.y);
      }
    }
    team_sync<SY>();
  }
}

namespace {

FeatRows rows_of(const View& v) { return {v.x, v.dtype, v.stride, v.N, v.unit0}; }

// one launch per (sample type, power, log): the two switches are compile-time, so neither costs the frame loop a register
template <int N, typename T, bool POW2, bool LOG>
hipError_t fwd_launch(const View& v, const Geom& g, int64_t units, const void* tw, const float* win, const float* mask,
                      const FeatBank& bank, double eps, void* feat, hipStream_t st) {
  constexpr int NT = spec_nt<N>(), WAVES = spec_teams<N>();
  const size_t lds = (size_t)(N + WAVES * N) * sizeof(cx<float>);   // k_spec_fwd's
  const dim3 grid((unsigned)((g.T + WAVES * SPEC_FPW - 1) / (WAVES * SPEC_FPW)), (unsigned)units);
  hipLaunchKernelGGL((k_feat_fwd<N, WAVES, SPEC_FPW, NT, T, POW2, LOG>), grid, dim3(WAVES * NT), lds, st, rows_of(v), g,
                     (const cx<float>*)tw, win, mask, bank, eps, (T*)feat);
  return hipGetLastError();
}

template <int N, typename T, bool POW2, bool LOG>
hipError_t bwd_launch(const View& v, const Geom& g, int64_t units, const void* tw, const float* win, const float* mask,
                      const FeatBank& bank, double eps, const void* grad, float* seg, hipStream_t st) {
  constexpr int NT = spec_nt<N>(), WAVES = spec_teams<N>();
  const size_t lds = (size_t)(N + WAVES * N) * sizeof(cx<float>) + (size_t)WAVES * ((LOG ? N + 1 : 0) + bank.M) * sizeof(float);
  const dim3 grid((unsigned)((g.T + WAVES * SPEC_FPW - 1) / (WAVES * SPEC_FPW)), (unsigned)units);
  // dynamic LDS beyond 64 KiB (many filters on the 16-team shapes) has to be asked for
  return host::launch_lds_if(lds > 64 * 1024, k_feat_bwd<N, WAVES, SPEC_FPW, NT, T, POW2, LOG>, grid, dim3(WAVES * NT), lds, st, rows_of(v), g,
                             (const cx<float>*)tw, win, mask, bank, eps, (const T*)grad, seg);
}

#define FEAT_SWITCH(fn, N, ...)                                                          \
  (dtype == 1 ? (power == 2 ? (take_log ? fn<N, double, true, true>(__VA_ARGS__)         \
                                        : fn<N, double, true, false>(__VA_ARGS__))       \
                            : (take_log ? fn<N, double, false, true>(__VA_ARGS__)        \
                                        : fn<N, double, false, false>(__VA_ARGS__)))     \
              : (power == 2 ? (take_log ? fn<N, float, true, true>(__VA_ARGS__)          \
                                        : fn<N, float, true, false>(__VA_ARGS__))        \
                            : (take_log ? fn<N, float, false, true>(__VA_ARGS__)         \
                                        : fn<N, float, false, false>(__VA_ARGS__))))

template <int N>
hipError_t fwd_n(const View& v, const Geom& g, int64_t units, const void* tw, const float* win, const float* mask,
                 const FeatBank& bank, int power, int take_log, double eps, void* feat, int dtype, hipStream_t st) {
  return FEAT_SWITCH(fwd_launch, N, v, g, units, tw, win, mask, bank, eps, feat, st);
}

template <int N>
hipError_t bwd_n(const View& v, const Geom& g, int64_t units, const void* tw, const float* win, const float* mask,
                 const FeatBank& bank, int power, int take_log, double eps, const void* grad, int dtype, float* seg,
                 hipStream_t st) {
  return FEAT_SWITCH(bwd_launch, N, v, g, units, tw, win, mask, bank, eps, grad, seg, st);
}

bool args_ok(int64_t units, const FeatBank& bank, int power, int dtype) {
  return units >= 1 && units <= 65535 && (dtype == 0 || dtype == 1) && (power == 1 || power == 2) && bank.M >= 1 &&
         bank.M <= FEAT_MAX_FILTERS && bank.fb && bank.fbT && bank.khull && bank.mhull;
}

}  // namespace

hipError_t feat_forward(const View& v, const Geom& g, int64_t units, const void* tw32, const float* win, const float* mask,
                        const FeatBank& bank, int power, int take_log, double eps, void* feat, int dtype, hipStream_t st) {
  if (!args_ok(units, bank, power, dtype)) return hipErrorInvalidValue;
  switch (g.n) {
    case 256: return fwd_n<128>(v, g, units, tw32, win, mask, bank, power, take_log, eps, feat, dtype, st);
    case 512: return fwd_n<256>(v, g, units, tw32, win, mask, bank, power, take_log, eps, feat, dtype, st);
    case 1024: return fwd_n<512>(v, g, units, tw32, win, mask, bank, power, take_log, eps, feat, dtype, st);
    case 2048: return fwd_n<1024>(v, g, units, tw32, win, mask, bank, power, take_log, eps, feat, dtype, st);
    case 4096: return fwd_n<2048>(v, g, units, tw32, win, mask, bank, power, take_log, eps, feat, dtype, st);
  }
  return hipErrorInvalidValue;
}

hipError_t feat_backward_frames(const View& v, const Geom& g, int64_t units, const void* tw32, const float* win,
                                const float* mask, const FeatBank& bank, int power, int take_log, double eps,
                                const void* grad_feat, int dtype, float* seg, hipStream_t st) {
  if (!args_ok(units, bank, power, dtype)) return hipErrorInvalidValue;
  switch (g.n) {
    case 256: return bwd_n<128>(v, g, units, tw32, win, mask, bank, power, take_log, eps, grad_feat, dtype, seg, st);
    case 512: return bwd_n<256>(v, g, units, tw32, win, mask, bank, power, take_log, eps, grad_feat, dtype, seg, st);
    case 1024: return bwd_n<512>(v, g, units, tw32, win, mask, bank, power, take_log, eps, grad_feat, dtype, seg, st);
    case 2048: return bwd_n<1024>(v, g, units, tw32, win, mask, bank, power, take_log, eps, grad_feat, dtype, seg, st);
    case 4096: return bwd_n<2048>(v, g, units, tw32, win, mask, bank, power, take_log, eps, grad_feat, dtype, seg, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace sg
