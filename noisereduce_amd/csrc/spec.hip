// Kernels of the gated spectrogram (spec.hpp; sg_gate_spectrum / sg_gate_spectrum_backward).
//
// Every frame is independent: no overlap-add in the forward, no tickets, no hand-offs between workgroups.  Both per-frame
// kernels run the LDS Stockham transform of fft_wave.hpp on the half-size complex frame (N = n_fft / 2), with the team
// shapes of the general apply kernel (k_apply_istft): sub-wavefront teams for short frames, one wavefront per frame from
// N = 512, the whole workgroup on one frame at N = 2048.
//
//   k_spec_fwd   window -> FFT -> split to the n_fft/2 + 1 bins -> * mask row -> complex store; consecutive lanes store
//                consecutive bins (a complex64 row of a wavefront is 512 contiguous bytes).
//   k_spec_bwd   mask .* grad -> merge to the half-size spectrum -> inverse FFT -> * window -> seg[u][t][0..n)
//   k_spec_ola   un-normalised overlap-add gather of seg onto [0, L): one thread per sample, frames in ascending order.
#include <hip/hip_runtime.h>

#include "fft_wave.hpp"
#include "geom.hpp"
#include "spec.hpp"
#include "spec_team.hpp"

namespace sg {

namespace {

// threads that share one frame / frames in flight per workgroup (the rules of api.hip's team_threads / team_count)
template <int N>
constexpr int spec_nt() { return N >= 2048 ? 256 : (N <= 128 ? 16 : (N == 256 ? 32 : 64)); }
template <int N>
constexpr int spec_teams() { return N >= 2048 ? 1 : (spec_nt<N>() < 64 ? 256 / spec_nt<N>() : (N * sizeof(cx<float>) > 16384 ? 2 : 4)); }
constexpr int SPEC_FPW = 4;   // frames per team and workgroup: the twiddle table is staged once for all of them

template <typename T> struct pair_of;
template <> struct pair_of<float> { using type = float2; };
template <> struct pair_of<double> { using type = double2; };

}  // namespace

template <int N, int WAVES, int FPW, int NT, typename TO>
__global__ __launch_bounds__(WAVES * NT) void k_spec_fwd(View view, Geom g, const cx<float>* __restrict__ tw_g,
                                                         const float* __restrict__ win, const float* __restrict__ mask,
                                                         TO* __restrict__ spec) {
  using V2 = typename pair_of<TO>::type;
  constexpr int SY = NT <= 64 ? 1 : NT;   // a team of <= 64 lanes is (part of) one wavefront and its buffer is its own
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<float>* tw = reinterpret_cast<cx<float>*>(smem);
  cx<float>* bufs = tw + N;
  const int lane = threadIdx.x % NT;
  const int wave = threadIdx.x / NT;
  cx<float>* buf = bufs + wave * N;
  stage_twiddles<WAVES * NT, N>(tw, tw_g, (int)threadIdx.x);
  const int64_t u = blockIdx.y;
  const int64_t row = view.unit0 + u;
  __syncthreads();
  for (int fi = 0; fi < FPW; ++fi) {
    const int64_t t = ((int64_t)blockIdx.x * FPW + fi) * WAVES + wave;
    const bool valid = t < g.T;
    // window * frame as complex pairs (x[2j], x[2j+1]); samples outside the row are torch.stft's zero padding
    const int64_t s0 = t * g.H - g.padL;
    const float* fp = valid ? frame_ptr_f32(view, row, 0, s0, 2 * N) : nullptr;  // team-uniform
    if (fp) {
      for (int j = lane; j < N; j += NT) buf[j] = {fp[2 * j] * win[2 * j], fp[2 * j + 1] * win[2 * j + 1]};
    } else {
      for (int j = lane; j < N; j += NT) {
        cx<float> z = {0.f, 0.f};
        if (valid) {
          z.x = (float)view_sample(view, row, 0, s0 + 2 * j) * win[2 * j];
          z.y = (float)view_sample(view, row, 0, s0 + 2 * j + 1) * win[2 * j + 1];
        }
        buf[j] = z;
      }
    }
    team_sync<SY>();
    wave_fft<float, N, false, NT, SY>(buf, tw, lane);
    if (valid) {
      const float* Mrow = mask + (u * g.T + t) * g.FS;
      V2* srow = reinterpret_cast<V2*>(spec) + (u * g.T + t) * g.F;
      for (int k = lane; k <= N; k += NT) {
        const cx<float> a = buf[k == N ? 0 : k];
        const cx<float> b = buf[(k == 0 || k == N) ? 0 : N - k];
        const cx<float> X = rfft_bin(a, b, tw[k == N ? 0 : k], k, N);
        const float m = Mrow[k];
        V2 o;
        o.x = (TO)(X.x * m);
        o.y = (TO)(X.y * m);
        srow[k] = o;
      }
    }
    team_sync<SY>();
  }
}

// The adjoint frame.  With Y[k] = mask[k] grad[k] (0 < k < N), Y[0] = 2 mask[0] Re grad[0], Y[N] = 2 mask[N] Re grad[N] read
// as the Hermitian half of a length-2N spectrum, the un-normalised half-size inverse transform of its merge is
// N * irfft(Y)[j] = Re sum_{k=0}^{N} mask[k] grad[k] e^{+2 pi i k j / 2N}: every bin with weight 1, the imaginary parts of
// grad[0] and grad[N] unused.  The merge is k_apply_istft's (spec_team.hpp).
template <int N, int WAVES, int FPW, int NT, typename TI>
__global__ __launch_bounds__(WAVES * NT) void k_spec_bwd(Geom g, const cx<float>* __restrict__ tw_g,
                                                         const float* __restrict__ win, const float* __restrict__ mask,
                                                         const TI* __restrict__ grad, float* __restrict__ seg) {
  using V2 = typename pair_of<TI>::type;
  constexpr int SY = NT <= 64 ? 1 : NT;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<float>* tw = reinterpret_cast<cx<float>*>(smem);
  cx<float>* bufs = tw + N;
  const int lane = threadIdx.x % NT;
  const int wave = threadIdx.x / NT;
  cx<float>* buf = bufs + wave * N;
  stage_twiddles<WAVES * NT, N>(tw, tw_g, (int)threadIdx.x);
  const int64_t u = blockIdx.y;
  __syncthreads();
  for (int fi = 0; fi < FPW; ++fi) {
    const int64_t t = ((int64_t)blockIdx.x * FPW + fi) * WAVES + wave;
    const bool valid = t < g.T;
    if (valid) {
      const float* Mrow = mask + (u * g.T + t) * g.FS;
      const V2* grow = reinterpret_cast<const V2*>(grad) + (u * g.T + t) * g.F;
      for (int k = lane; k <= N / 2; k += NT) {
        if (k == 0) {
          const float y0 = 2.0f * (float)grow[0].x * Mrow[0];
          const float yN = 2.0f * (float)grow[N].x * Mrow[N];
          merge_dc(buf, y0, yN);
        } else {
          const V2 gk = grow[k], gn = grow[N - k];
          const float mk = Mrow[k], mn = Mrow[N - k];
          const cx<float> w = tw[k];
          const cx<float> Yk = {(float)gk.x * mk, (float)gk.y * mk};
          const cx<float> Yn = {(float)gn.x * mn, (float)gn.y * mn};
          merge_pair(buf, w, k, N, Yk, Yn);
        }
      }
    }
    team_sync<SY>();
    wave_fft<float, N, true, NT, SY>(buf, tw, lane);
    if (valid) {
      float2* srow = reinterpret_cast<float2*>(seg + (u * g.T + t) * (int64_t)g.n);
      for (int j = lane; j < N; j += NT) {
        const cx<float> z = buf[j];
        srow[j] = make_float2(z.x * win[2 * j], z.y * win[2 * j + 1]);
      }
    }
    team_sync<SY>();
  }
}

__global__ __launch_bounds__(256) void k_spec_ola(Geom g, int64_t L, const float* __restrict__ seg, void* __restrict__ gx,
                                                  int dtype, int64_t stride) {
  const int64_t u = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= L) return;
  const int64_t e = p + g.padL;
  int64_t t_hi = e / g.H;
  if (t_hi > g.T - 1) t_hi = g.T - 1;
  int64_t t_lo = (e - g.n + g.H) / g.H;  // ceil((e - n + 1) / H)
  if (e - g.n + 1 <= 0) t_lo = 0;
  float acc = 0.f;
  for (int64_t t = t_lo; t <= t_hi; ++t) acc += seg[(u * g.T + t) * (int64_t)g.n + (e - t * g.H)];
  store_sample(gx, dtype, u * stride + p, acc);
}

// one thread per four cells (FS is a multiple of 16): a 16-byte store, the padding cells beyond bin F - 1 as 0
__global__ __launch_bounds__(256) void k_spec_bits_to_raw(const unsigned long long* __restrict__ bits, Geom g, int wpr,
                                                          float* __restrict__ raw, int64_t n_units) {
  const int qpr = g.FS >> 2;
  const int64_t quads = n_units * g.T * qpr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t ut = i / qpr;
    const int f0 = (int)(i - ut * qpr) * 4;
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = f0 + e;
      o[e] = (f < g.F && ((bits[ut * wpr + (f >> 6)] >> (f & 63)) & 1ull)) ? 1.0f : 0.0f;
    }
    *reinterpret_cast<float4*>(raw + i * 4) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

namespace {

template <int N>
hipError_t fwd_n(const View& v, const Geom& g, int64_t units, const void* tw, const float* win, const float* mask,
                 void* spec, int dtype, hipStream_t st) {
  constexpr int NT = spec_nt<N>(), WAVES = spec_teams<N>();
  const size_t lds = (size_t)(N + WAVES * N) * sizeof(cx<float>);
  const dim3 grid((unsigned)((g.T + WAVES * SPEC_FPW - 1) / (WAVES * SPEC_FPW)), (unsigned)units);
  if (dtype == 1)
    hipLaunchKernelGGL((k_spec_fwd<N, WAVES, SPEC_FPW, NT, double>), grid, dim3(WAVES * NT), lds, st, v, g,
                       (const cx<float>*)tw, win, mask, (double*)spec);
  else
    hipLaunchKernelGGL((k_spec_fwd<N, WAVES, SPEC_FPW, NT, float>), grid, dim3(WAVES * NT), lds, st, v, g,
                       (const cx<float>*)tw, win, mask, (float*)spec);
  return hipGetLastError();
}

template <int N>
hipError_t bwd_n(const Geom& g, int64_t units, const void* tw, const float* win, const float* mask, const void* grad,
                 int dtype, float* seg, hipStream_t st) {
  constexpr int NT = spec_nt<N>(), WAVES = spec_teams<N>();
  const size_t lds = (size_t)(N + WAVES * N) * sizeof(cx<float>);
  const dim3 grid((unsigned)((g.T + WAVES * SPEC_FPW - 1) / (WAVES * SPEC_FPW)), (unsigned)units);
  if (dtype == 1)
    hipLaunchKernelGGL((k_spec_bwd<N, WAVES, SPEC_FPW, NT, double>), grid, dim3(WAVES * NT), lds, st, g,
                       (const cx<float>*)tw, win, mask, (const double*)grad, seg);
  else
    hipLaunchKernelGGL((k_spec_bwd<N, WAVES, SPEC_FPW, NT, float>), grid, dim3(WAVES * NT), lds, st, g,
                       (const cx<float>*)tw, win, mask, (const float*)grad, seg);
  return hipGetLastError();
}

}  // namespace

bool spec_native(int n_fft) { return n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048 || n_fft == 4096; }

hipError_t spec_bits_to_raw(const unsigned long long* bits, const Geom& g, int wpr, float* raw, int64_t units, hipStream_t st) {
  const int64_t quads = units * g.T * (g.FS >> 2);
  if (units < 1 || quads < 1) return hipErrorInvalidValue;
  const int64_t blocks = (quads + 255) / 256;
  hipLaunchKernelGGL(k_spec_bits_to_raw, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, bits, g, wpr,
                     raw, units);
  return hipGetLastError();
}

hipError_t spec_forward(const View& v, const Geom& g, int64_t units, const void* tw32, const float* win,
                        const float* mask, void* spec, int dtype, hipStream_t st) {
  if (units < 1 || units > 65535 || (dtype != 0 && dtype != 1)) return hipErrorInvalidValue;
  switch (g.n) {
    case 256: return fwd_n<128>(v, g, units, tw32, win, mask, spec, dtype, st);
    case 512: return fwd_n<256>(v, g, units, tw32, win, mask, spec, dtype, st);
    case 1024: return fwd_n<512>(v, g, units, tw32, win, mask, spec, dtype, st);
    case 2048: return fwd_n<1024>(v, g, units, tw32, win, mask, spec, dtype, st);
    case 4096: return fwd_n<2048>(v, g, units, tw32, win, mask, spec, dtype, st);
  }
  return hipErrorInvalidValue;
}

hipError_t spec_backward_frames(const Geom& g, int64_t units, const void* tw32, const float* win, const float* mask,
                                const void* grad_spec, int dtype, float* seg, hipStream_t st) {
  if (units < 1 || units > 65535 || (dtype != 0 && dtype != 1)) return hipErrorInvalidValue;
  switch (g.n) {
    case 256: return bwd_n<128>(g, units, tw32, win, mask, grad_spec, dtype, seg, st);
    case 512: return bwd_n<256>(g, units, tw32, win, mask, grad_spec, dtype, seg, st);
    case 1024: return bwd_n<512>(g, units, tw32, win, mask, grad_spec, dtype, seg, st);
    case 2048: return bwd_n<1024>(g, units, tw32, win, mask, grad_spec, dtype, seg, st);
    case 4096: return bwd_n<2048>(g, units, tw32, win, mask, grad_spec, dtype, seg, st);
  }
  return hipErrorInvalidValue;
}

hipError_t spec_backward_ola(const Geom& g, int64_t units, int64_t L, const float* seg, void* grad_x, int dtype,
                             int64_t gx_stride, hipStream_t st) {
  if (units < 1 || units > 65535 || L < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_spec_ola, dim3((unsigned)((L + 255) / 256), (unsigned)units), dim3(256), 0, st, g, L, seg,
                     grad_x, dtype, gx_stride);
  return hipGetLastError();
}

}  // namespace sg
