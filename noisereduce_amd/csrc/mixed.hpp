// Mixed-radix frames (round 6; SURVEY.md section 8 row f3, VERDICT r5 "missing" item 4).
//
// The reference hands any n_fft to scipy's pocketfft (stationary.py:87-93), which transforms 400, 1000, 1536 or 3000
// points as fast as 512 or 1024.  Up to round 5 every frame length that was not a power of two went through the
// chirp-z kernels of czt.hpp -- two transforms of M >= 2 n complex points where a real frame of n = 2 N samples needs one
// of N: 15 - 70 x slower than the neighbouring powers of two.  Here: a Stockham autosort transform whose radix schedule
// is a RUN-TIME argument (8 / 4 / 2 / 5 / 3, plus a direct small-prime butterfly for 7, 11, 13), on the same real-packed
// layout, master twiddle table (w_2N^k, k < N: it serves the passes -- w_N^t = w_2N^(2t) -- and the real-FFT split) and
// surrounding kernels as the power-of-two LDS path (kernels.hpp k_stft / k_apply_istft, fused.hpp k_stft_bits /
// k_decide_lds), whose outputs these kernels reproduce field for field.  Chirp-z remains for odd n, for n with a prime
// factor above 13 and for N = n / 2 > 2048.
//
// One pass of radix R at stride S (the product of the radices before it), NB = N / R butterflies:
//     butterfly i = p S + q (q < S):   v[j] = x[i + j NB];   v = DFT_R(v);   v[k] *= w_N^(p S k);   y[p S R + q + S k] = v[k]
// -- the formula of FftPass (fft_wave.hpp) with `&` replaced by `%`.  The passes PING-PONG between two buffers: the
// in-place form needs every read of a pass in registers before its first write, i.e. compile-time trip counts.
#pragma once
#include "fft_wave.hpp"
#include "thresh.hpp"

namespace sg {

// LDS index padding of the transform buffers: float64 as fft_wave.hpp's lp (one spare element per 8); float32 NONE.  A
// Stockham pass reads lane-contiguous and WRITES with strides of R (first pass) or in runs of S elements R S apart: unpadded,
// the 8-byte float32 elements of a wavefront land on a few banks (radix 8, first pass: a 16-way conflict by address).
// Measured (round 6, with one spare float32 element per 32, i.e. per bank cycle, which moves successive 256-byte rows two
// banks apart): k_decide_mr 112 -> 118 us, k_apply_istft_mr 136 -> 176 us at n_fft = 1000 -- the index arithmetic costs more
// than the conflicts did, as fft_wave.hpp found for its own per-8 padding.
template <typename T>
__host__ __device__ constexpr int mlp(int e) { return sizeof(T) == 8 ? e + (e >> 3) : e; }
template <typename T>
__host__ __device__ constexpr int mlpn(int n) { return mlp<T>(n) + 1; }

constexpr int MR_MAXP = 8;        // passes (2^11 = 2048 = 8 8 8 4; 2 3 5 7 11 13 > 2048)
constexpr int MR_MAXR = 13;       // largest radix
struct MrPlan {
  int N;                          // complex length (n_fft / 2)
  int np;                         // passes
  unsigned char R[MR_MAXP];       // radices, in pass order; product = N
  // per-pass twiddle tables: butterfly i = g S + q of pass p multiplies output k (1 <= k < R) by w_N^(g S k) =
  // ptab[toff[p] + g (R - 1) + (k - 1)] -- the R - 1 factors of a butterfly are CONTIGUOUS (one or two 16-byte LDS reads,
  // no index arithmetic; looked up in the master table they cost ten integer instructions each: half of a pass).  The last
  // pass (all ones) has no entries.  Built by mr_pass_tables(), staged in LDS behind the master table.
  int toff[MR_MAXP];
  int ptotal;                     // entries of all passes together (< 2 N)
};

// Launchers (mixed.hip: a translation unit of its own -- the kernel bodies below it are instantiated for four team sizes
// and two precisions, and compile beside api.hip).  Plain arguments, no engine handle.
bool mr_make_plan(int N, MrPlan* pl);   // false: N has a prime factor above 13 (or N > 2048)
// the plan's pass tables, ptotal entries (re, im) in long double precision rounded to double: out[2 i], out[2 i + 1]
void mr_pass_tables(const MrPlan& pl, double* out);
hipError_t mr_launch_stft32(const MrPlan& pl, const View& v, const Geom& g, int64_t units, const cx<float>* tw, const cx<float>* ptab,
                            const float* wfull, double* P, float* mag, double* z, double zscale, unsigned long long* pmax_bits,
                            hipStream_t st);
hipError_t mr_launch_stft64(const MrPlan& pl, const View& v, const Geom& g, int64_t units, const cx<double>* tw, const cx<double>* ptab,
                            const double* wfull, double* P, float* mag, double* z, double zscale, unsigned long long* pmax_bits,
                            hipStream_t st);
hipError_t mr_launch_bits(int mode, const MrPlan& pl, const View& v, const Geom& g, int64_t units, const cx<double>* tw,
                          const cx<double>* ptab, const double* wfull, const ThreshConsts& tc, double mag_scale, double top_db,
                          unsigned long long* pmax_bits, unsigned long long* bits, int wpr, hipStream_t st);
hipError_t mr_launch_decide(const MrPlan& pl, const View& v, const Geom& g, int64_t units, const cx<float>* tw32, const cx<float>* ptab32,
                            const float* win32, const cx<double>* tw64, const double* win64, const ThreshConsts& tc, double mag_scale, double top_db,
                            unsigned long long* bits, int wpr, hipStream_t st);
hipError_t mr_launch_apply(const MrPlan& pl, const View& v, const Geom& g, int64_t units, const cx<float>* tw32, const cx<float>* ptab32,
                           const float* wa, const float* ws, const float* M, float* seg, const unsigned short* K16, float kscale, hipStream_t st);

}  // namespace sg
