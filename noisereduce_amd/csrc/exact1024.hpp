// Exact float64 |X[f]|^2 of one frame at n_fft = 1024, computed by a whole wavefront: the re-evaluation of a cell whose
// float32 power lies within delta of its threshold (k_decide_fast, k_gate_onepass).  One body for both kernels, so their
// decisions stay bit-identical.
//
// Lane l sums the terms m = l + 64 i, i = 0..15.  Their twiddles factor,
//     w_1024^(f m) = w_1024^(f l) * rho^i,   rho = w_16^f  (wave-uniform, f is),
// so a lane needs ONE entry of the float64 table (with the table's sign fold at 512) instead of sixteen scattered ones, and
// rho^8 = (-1)^f exactly: the sum splits into two Horner chains of eight terms,
//     X_l = w^(f l) * (H(x_0 .. x_7) + (-1)^f H(x_8 .. x_15)),   H(y_0 .. y_7) = y_0 + rho (y_1 + rho (y_2 + ... rho y_7)).
// A term in flight is then the sample and its float64 window value (3 registers for float32 input, not 7): the loads of
// eight terms are issued together and waited for once.  Sample loads are unconditional at an index clamped into the
// frame's readable terms [a, b) and zeroed by a select afterwards (a predicated load serialises every load behind it); the
// sample type is dispatched once, outside the term loops.
// Reduction: the first exchange hands the real parts to lanes 0..31 and the imaginary parts to lanes 32..63 (two
// half-wave swaps), so each half reduces one double over the pairs and in the order a full butterfly of both would.
#pragma once
#include "fft_wave.hpp"
#include "geom.hpp"

namespace sg {
namespace fast {

// the terms m of [0, 1024) whose sample exists (view_sample's two tests): term m is sample s0 + m of the unit window
// [0, Lp) and element e + m of a row that is readable in [lo, hi)
__device__ __forceinline__ void exact1024_terms(int64_t s0, int64_t e, int64_t Lp, int64_t lo, int64_t hi, int& a, int& b) {
  const int64_t first = -s0 > lo - e ? -s0 : lo - e;
  const int64_t end = Lp - s0 < hi - e ? Lp - s0 : hi - e;
  a = (int)(first < 0 ? 0 : first > 1024 ? 1024 : first);
  b = (int)(end < 0 ? 0 : end > 1024 ? 1024 : end);
}

__device__ __forceinline__ double ex_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// A wave-uniform pointer as a GLOBAL one in scalar registers: a load is then `scalar base + 32-bit lane offset`, one address
// register per load in flight instead of a 64-bit pair (the one-pass gate's pointers come out of an opaque re-read of its
// kernel arguments: generic addresses in vector registers otherwise)
template <typename T>
using ex_gptr = const __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ ex_gptr<T> ex_global(const T* p) {
  const unsigned long long v = (unsigned long long)(uintptr_t)p;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return (ex_gptr<T>)(uintptr_t)((unsigned long long)lo | ((unsigned long long)hi << 32));
}

// xor-exchange within a half-wave (off < 32) without an address register
template <int OFF>
__device__ __forceinline__ double ex_swz_xor(double v) {
  constexpr int pat = (OFF << 10) | 0x1f;   // bit-mask mode: and 0x1f, or 0, xor OFF
  return __hiloint2double(__builtin_amdgcn_ds_swizzle(__double2hiint(v), pat), __builtin_amdgcn_ds_swizzle(__double2loint(v), pat));
}

// eight terms from term 64 * I0: loads first, one wait, then the Horner chain in rho = (rx, ry).
// xa: the sample of term a; la = lane - a; n = b - a terms exist
template <typename T, int I0>
__device__ __forceinline__ void ex_horner8(ex_gptr<T> xa, ex_gptr<double> win64, int lane, int la, int n, double rx, double ry,
                                           double& hr, double& hi) {
  T xs[8];
  double wv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = la + 64 * (I0 + i);
    const int rc = r < 0 ? 0 : r >= n ? n - 1 : r;
    xs[i] = *(ex_gptr<T>)((ex_gptr<char>)xa + (unsigned)rc * (unsigned)sizeof(T));
    wv[i] = *(ex_gptr<double>)((ex_gptr<char>)win64 + (unsigned)(lane + 64 * (I0 + i)) * 8u);
  }
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" : "+v"(la));   // the range tests are made again from `la`: eight indices less in registers under the loads
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    const int r = la + 64 * (I0 + i);
    const double xv = ((unsigned)r < (unsigned)n ? (double)xs[i] : 0.0) * wv[i];
    const double nr = fma(hr, rx, fma(-hi, ry, xv));
    hi = fma(hr, ry, hi * rx);
    hr = nr;
  }
}

// xp: the sample of term 0 (only terms of [a, b) are read; a < b)
template <typename T>
__device__ __forceinline__ double ex_power_t(const T* xp, int a, int b, const double* win64_, const cx<double>* tw64_,
                                             int f, int lane) {
  asm volatile("" : "+v"(lane));   // nothing of this rare path is precomputed outside the caller's loop and kept in registers
  const ex_gptr<T> xa = ex_global(xp + a);
  const ex_gptr<double> win64 = ex_global(win64_);
  const ex_gptr<double> tw64 = ex_global(reinterpret_cast<const double*>(tw64_));   // {cos, sin} pairs
  const int n = b - a, la = lane - a;
  const int jl = (f * lane) & 1023, jr = (f * 64) & 1023;
  // issued with the first batch
  const ex_gptr<double> pl = (ex_gptr<double>)((ex_gptr<char>)tw64 + (unsigned)(jl & 511) * 16u);
  const ex_gptr<double> pr = (ex_gptr<double>)((ex_gptr<char>)tw64 + (unsigned)(jr & 511) * 16u);
  cx<double> wl = {pl[0], pl[1]}, rho = {pr[0], pr[1]};
  double h0r, h0i, h1r, h1i;
  {
    if (jr >= 512) { rho.x = -rho.x; rho.y = -rho.y; }
    const double rx = ex_uniform(rho.x), ry = ex_uniform(rho.y);
    h0r = h0i = h1r = h1i = 0.0;
    ex_horner8<T, 0>(xa, win64, lane, la, n, rx, ry, h0r, h0i);
    ex_horner8<T, 8>(xa, win64, lane, la, n, rx, ry, h1r, h1i);
  }
  if (jl >= 512) { wl.x = -wl.x; wl.y = -wl.y; }
  const double sr = (f & 1) ? h0r - h1r : h0r + h1r, si = (f & 1) ? h0i - h1i : h0i + h1i;
  const double re = fma(sr, wl.x, -(si * wl.y)), im = fma(sr, wl.y, si * wl.x);
  // lanes 32..63 of `re` <-> lanes 0..31 of `im`: a lower lane then holds re_l and re_(l + 32), an upper one im_(l - 32)
  // and im_l
  const auto s_lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(re), (unsigned)__double2loint(im), false, false);
  const auto s_hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(re), (unsigned)__double2hiint(im), false, false);
  double v = __hiloint2double((int)s_hi[0], (int)s_lo[0]) + __hiloint2double((int)s_hi[1], (int)s_lo[1]);
  v += ex_swz_xor<16>(v);
  v += ex_swz_xor<8>(v);
  v += ex_swz_xor<4>(v);
  v += ex_swz_xor<2>(v);
  v += ex_swz_xor<1>(v);
  const int v_lo = __double2loint(v), v_hi = __double2hiint(v);
  const double tr = __hiloint2double(__builtin_amdgcn_readlane(v_hi, 0), __builtin_amdgcn_readlane(v_lo, 0));
  const double ti = __hiloint2double(__builtin_amdgcn_readlane(v_hi, 32), __builtin_amdgcn_readlane(v_lo, 32));
  return fma(tr, tr, ti * ti);
}

// x[e0 + m] is the sample of term m, a term outside [a, b) is zero (exact1024_terms); win64: the 1024 float64 window
// values, tw64: w_1024^j, j < 512.  Wave-uniform arguments but `lane`.
__device__ __forceinline__ double exact1024_power(const void* x, int dtype, int64_t e0, int a, int b, const double* win64,
                                                  const cx<double>* tw64, int f, int lane) {
  if (a >= b) return 0.0;   // no sample of the frame exists
  f = __builtin_amdgcn_readfirstlane(f);
  switch (dtype) {
    case 0: return ex_power_t((const float*)x + e0, a, b, win64, tw64, f, lane);
    case 1: return ex_power_t((const double*)x + e0, a, b, win64, tw64, f, lane);
    case 2: return ex_power_t((const int16_t*)x + e0, a, b, win64, tw64, f, lane);
    default: return ex_power_t((const int32_t*)x + e0, a, b, win64, tw64, f, lane);
  }
}

}  // namespace fast
}  // namespace sg
