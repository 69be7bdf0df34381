// Banks of live streams (sg_stream_push): tables, kernels and the host side.  See stream.hpp and DESIGN section 13.
//
// Four launches per step, each driven by a tile table built on the host (one upload per step), as in ragged.hip:
//   k_st_decide   one workgroup per (stream, channel) with newly decidable frames, frames IN ORDER: float64 transform,
//                 running band maximum (a prefix maximum: frame t's floor never sees frame t + 1), final raw-mask bits
//   k_st_fsmooth  frequency smoothing of the bit rows the step's applied frames read
//   k_st_apply    time smoothing, prop_decrease, masked multiply, inverse transform (the frame is transformed again from
//                 the ring / the caller's block, as k_rg_apply does)
//   k_st_finish   overlap-add of the newly final samples into the caller's output + partial sums of the samples still
//                 open (carry), then the state update: block -> ring, band maxima of flushed streams cleared
// A non-stationary bank (sg_stream_create_nonstationary) runs the same four launches with k_sn_decide in the first place:
// float64 transform, A = |X|, the forward one-pole pass carried per band, the A / fwd rows of the last L + 1 frames kept,
// and for every frame that has L frames after it (or the stream's end, at a flush) the backward pass over those L + 1
// rows and the sigmoid into a ring of float mask rows, which k_st_fsmooth<true> / k_st_apply<N, true> read instead of bits.
// Nothing waits on another workgroup.  No workgroup reads state that another workgroup of the same launch writes: the
// ring is only written by k_st_finish (which does not read it), the carry is double buffered, the bit rows of a unit are
// written by its one decide workgroup.  One fixed evaluation order per frame and per output sample: a stream's output
// does not depend on the block split, the slot, or the other streams of the step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fft_wave.hpp"
#include "geom.hpp"
#include "thresh.hpp"
#include "stream.hpp"
#include "../../include/mi355gate_debug.h"

namespace sg {

// ---- tables ------------------------------------------------------------------------------------------------------
struct StUnit {
  int64_t in_off, out_off;   // element of in holding the block's first sample / of out receiving sample E0
  int64_t n0, n1;            // samples received before / after this step
  int64_t td0, td1;          // last decided (transformed) frame before / after (-1: none)
  int64_t ts0, ts1;          // non-stationary: last frame with a raw mask row before / after (td - lookahead; td at a flush)
  int64_t ta0, ta1;          // last applied frame before / after
  int64_t Tend;              // frames of the whole stream when flushing, else "unbounded"
  int64_t Lout;              // flush: valid samples of the inverse transform (zero tail beyond)
  int64_t E0, E1;            // emitted before / after
  int64_t cov0;              // end of the samples the applied frames of earlier steps reach (carry valid below it)
  int64_t r0, r1;            // mask rows the applied frames read
  int64_t mrow, srow;        // first row of this unit in the smoothed-row / segment scratch
  int32_t state;             // slot * channels + channel
  int32_t slot;
  int32_t par;               // carry buffer to read (the other one is written)
  int32_t flush;
};
struct StTile {
  int32_t idx, kind;
  int64_t a, b;
};
enum { ST_OLA = 0, ST_APPEND = 1, ST_CLEAR = 2 };

struct StArgs {
  const void* x; int in_dtype;
  void* out; int out_dtype;
  const StUnit* units;
  const StTile* tiles;
  int64_t t_dec, n_dec, t_fs, n_fs, t_ap, n_ap, t_fin, n_fin;
  const cx<double>* tw;
  const double* wfull;
  double* ring;
  unsigned long long* bits;
  double* rmax;
  double* carry;
  const double* thr;
  const double* T2;
  float* R;
  float* seg;
  int n, W, H, F, FS, padL, wpr, RC, RB, nf, nt;
  double mag_scale, top_db, prop, ktot;
  // non-stationary banks
  double* fst;     // [unit][FS] forward state fwd[f, td]
  double* fa;      // [unit][RF][2][FS] A and fwd rows of the last transformed frames, frame t at t % RF
  float* mk;       // [unit][RB][FS] raw (sigmoid) mask rows, frame t at t % RB
  int RF, L;
  double iir_b;
  float nthresh, slope;
};

__device__ __forceinline__ double st_nan_if_nonfinite(double P) { return (P <= 1.79769313486231570e308) ? P : (double)NAN; }

template <int N>
constexpr int st_nt() { return N <= 512 ? 64 : 256; }
template <int N>
constexpr int st_sy() { return st_nt<N>() <= 64 ? 1 : st_nt<N>(); }

// sample s of the stream: zeros before 0 and from n1 on, the ring below n0, the caller's block from n0 on
__device__ __forceinline__ double st_sample(const StArgs& A, const StUnit& U, int64_t s) {
  if (s < 0 || s >= U.n1) return 0.0;
  if (s < U.n0) return A.ring[(int64_t)U.state * A.RC + s % A.RC];
  return load_sample(A.x, A.in_dtype, U.in_off + (s - U.n0));
}

// window * frame t (samples [t H - h, t H - h + W), the frame zero-padded to n_fft at its end), forward transform in place
template <int N>
__device__ __forceinline__ void st_frame_fft(const StArgs& A, const StUnit& U, int64_t t, cx<double>* buf,
                                             const cx<double>* tw, int lane) {
  constexpr int NT = st_nt<N>(), SY = st_sy<N>();
  const int64_t s0 = t * A.H - A.padL;
  for (int j = lane; j < N; j += NT) {
    double v[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int jj = 2 * j + q;
      v[q] = jj < A.W ? st_sample(A, U, s0 + jj) * A.wfull[jj] : 0.0;
    }
    buf[lp<double>(j)] = {v[0], v[1]};
  }
  team_sync<SY>();
  wave_fft<double, N, false, NT, SY>(buf, tw, lane);
}

template <int N>
__device__ __forceinline__ cx<double> st_bin(const cx<double>* buf, const cx<double>* tw, int k) {
  cx<double> a = buf[lp<double>(k == N ? 0 : k)];
  cx<double> b = buf[lp<double>((k == 0 || k == N) ? 0 : N - k)];
  return rfft_bin(a, b, tw[k == N ? 0 : k], k, N);
}

// what the running maximum makes of a band: 0 = the cell's own compare decides, 1 = every cell passes (the floor
// max - top_db lies above the threshold, or the threshold below 20 log10(eps)), 2 = none passes (NaN maximum or threshold)
__device__ __forceinline__ int st_mode(double rm, double th, double t2, double mag_scale, double top_db) {
  if (th != th) return 2;
  const double fl = cell_db(rm, mag_scale) - top_db;
  if (fl != fl) return 2;
  return (fl > th || t2 < 0.0) ? 1 : 0;
}

// ---- thresholds of slots: dB -> compare constant on the raw power (k_rg_noise_final's) -------------------------------
__global__ __launch_bounds__(64) void k_st_thresh(const double* src, const int32_t* slots, double* thr, double* T2, int F, int FS,
                                                  double mag_scale) {
  const int64_t s = slots[blockIdx.x];
  const double eps = 2.220446049250313e-16;
  for (int f = threadIdx.x; f < F; f += 64) {
    const double th = src[f];
    double t2;
    if (th != th) {
      t2 = T2_NEVER;
    } else if (20.0 * log10(eps) > th) {
      t2 = -1.0;
    } else {
      const double tm = (exp10(th / 20.0) - eps) / mag_scale;
      t2 = tm > 0.0 ? tm * tm : 0.0;
    }
    thr[s * FS + f] = th;
    T2[s * FS + f] = t2;
  }
}

// ---- decide: the unit's new frames in order ------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(st_nt<N>()) void k_st_decide(StArgs A) {
  constexpr int NT = st_nt<N>(), SY = st_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const StTile tl = A.tiles[A.t_dec + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  stage_twiddles<NT, N>(tw, A.tw, lane);
  __syncthreads();
  constexpr int M = N / NT + 1;
  const double* T2 = A.T2 + (int64_t)U.slot * A.FS;
  const double* thr = A.thr + (int64_t)U.slot * A.FS;
  double* rmax = A.rmax + (int64_t)U.state * A.FS;
  double rm[M];
  int md[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int k = lane + NT * m;
    rm[m] = 0.0;
    md[m] = 2;
    if (k <= N) {
      rm[m] = rmax[k];
      md[m] = st_mode(rm[m], thr[k], T2[k], A.mag_scale, A.top_db);
    }
  }
  for (int64_t t = tl.a; t < tl.b; ++t) {
    st_frame_fft<N>(A, U, t, buf, tw, lane);
    unsigned long long* row = A.bits + ((int64_t)U.state * A.RB + t % A.RB) * A.wpr;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      bool pass = false;
      if (k <= N) {
        const cx<double> X = st_bin<N>(buf, tw, k);
        const double P = st_nan_if_nonfinite(X.x * X.x + X.y * X.y);
        if (P != P || P > rm[m]) {   // the maximum moves: so may the band's floor
          rm[m] = nanmax(rm[m], P);
          md[m] = st_mode(rm[m], thr[k], T2[k], A.mag_scale, A.top_db);
        }
        pass = md[m] == 1 || (md[m] == 0 && P > T2[k]);
      }
      const unsigned long long word = __ballot(pass);
      if ((lane & 63) == 0 && (k >> 6) < A.wpr) row[k >> 6] = word;
    }
    team_sync<SY>();
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int k = lane + NT * m;
    if (k <= N) rmax[k] = rm[m];
  }
}

// ---- non-stationary decide: forward pass over the unit's new frames, backward pass + sigmoid of the decidable ones ------
// Band k belongs to one thread for the whole launch: the A / fwd rows it reads in the second loop are its own stores of
// the first loop or of an earlier step, so no barrier separates the two.  S_L[f, t] = the reference's forward-backward
// smoother of frames 0 .. e, e = min(t + L, last frame): seeded with fwd[e], then k = e .. t in that order whatever the
// block split.  The sigmoid is the offline kernels' (ragged.hip rg_sigmoid_ratio): S = 0 gives 0 / 0 = NaN as there.
template <int N>
__global__ __launch_bounds__(st_nt<N>()) void k_sn_decide(StArgs A) {
  constexpr int NT = st_nt<N>(), SY = st_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const StTile tl = A.tiles[A.t_dec + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  stage_twiddles<NT, N>(tw, A.tw, lane);
  __syncthreads();
  constexpr int M = N / NT + 1;
  const double b = A.iir_b, c = 1.0 - A.iir_b;
  double* fst = A.fst + (int64_t)U.state * A.FS;
  double* fa = A.fa + (int64_t)U.state * A.RF * 2 * A.FS;
  double fw[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int k = lane + NT * m;
    fw[m] = (k <= N && U.td0 >= 0) ? fst[k] : 0.0;
  }
  for (int64_t t = U.td0 + 1; t <= U.td1; ++t) {
    st_frame_fft<N>(A, U, t, buf, tw, lane);
    double* row = fa + (t % A.RF) * 2 * A.FS;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      if (k <= N) {
        const cx<double> X = st_bin<N>(buf, tw, k);
        const double a = sqrt(st_nan_if_nonfinite(X.x * X.x + X.y * X.y));
        if (t == 0) fw[m] = a;   // fwd[f, -1] = A[f, 0]
        fw[m] = b * a + c * fw[m];
        row[k] = a;
        row[A.FS + k] = fw[m];
      }
    }
    team_sync<SY>();
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int k = lane + NT * m;
    if (k <= N && U.td1 > U.td0) fst[k] = fw[m];
  }
  for (int64_t t = U.ts0 + 1; t <= U.ts1; ++t) {
    const int64_t e = t + A.L < U.td1 ? t + A.L : U.td1;
    float* mrow = A.mk + ((int64_t)U.state * A.RB + t % A.RB) * A.FS;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      if (k <= N) {
        double s = fa[((e % A.RF) * 2 + 1) * A.FS + k];
        for (int64_t q = e; q >= t; --q) s = b * fa[((q % A.RF) * 2 + 1) * A.FS + k] + c * s;
        const double av = fa[(t % A.RF) * 2 * A.FS + k];
        const float ratio = (float)(av - s) / (float)s;
        mrow[k] = 1.0f / (1.0f + __expf(-(ratio - A.nthresh) * A.slope));
      }
    }
  }
}

// ---- mask smoothing along frequency: R[row][f] = sum_df (nf + 1 - |df|) raw[row][f + df] ----------------------------
// NS: the raw mask is a row of floats (the sigmoid) instead of a row of bits
template <bool NS>
__global__ __launch_bounds__(256) void k_st_fsmooth(StArgs A) {
  if ((int64_t)blockIdx.x >= A.n_fs) return;
  const StTile tl = A.tiles[A.t_fs + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  const int nf = A.nf;
  for (int64_t r = tl.a; r < tl.b; ++r) {
    const unsigned long long* brow = NS ? nullptr : A.bits + ((int64_t)U.state * A.RB + r % A.RB) * A.wpr;
    const float* frow = NS ? A.mk + ((int64_t)U.state * A.RB + r % A.RB) * A.FS : nullptr;
    float* out = A.R + (U.mrow + r - U.r0) * A.FS;
    for (int f = threadIdx.x; f < A.F; f += blockDim.x) {
      float acc = 0.f;
      for (int df = -nf; df <= nf; ++df) {
        const int g = f + df;
        if (g < 0 || g >= A.F) continue;
        acc += (float)(nf + 1 - (df < 0 ? -df : df)) * (NS ? frow[g] : (float)((brow[g >> 6] >> (g & 63)) & 1ull));
      }
      out[f] = acc;
    }
  }
}

// ---- applied frames: time smoothing, masked multiply, inverse transform (k_rg_apply) ---------------------------------
template <int N, bool NS>
__global__ __launch_bounds__(st_nt<N>()) void k_st_apply(StArgs A) {
  constexpr int NT = st_nt<N>(), SY = st_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const StTile tl = A.tiles[A.t_ap + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  stage_twiddles<NT, N>(tw, A.tw, lane);
  __syncthreads();
  const int nt = A.nt;
  for (int64_t t = tl.a; t < tl.b; ++t) {
    st_frame_fft<N>(A, U, t, buf, tw, lane);
    const int64_t ta = t - nt < 0 ? 0 : t - nt, tb = t + nt >= U.Tend ? U.Tend - 1 : t + nt;
    const double Et = (double)tri_valid(nt, t, U.Tend);
    auto mask_at = [&](int k) -> double {
      double K = 0.0;
      for (int64_t q = ta; q <= tb; ++q) {
        const int64_t d = q - t;
        K += (double)(nt + 1 - (d < 0 ? -d : d)) * (double)A.R[(U.mrow + q - U.r0) * A.FS + k];
      }
      if (NS) return (K / A.ktot) * A.prop + (1.0 - A.prop);   // smoothed first, prop_decrease after (k_rg_apply)
      return (A.prop * K + (1.0 - A.prop) * Et * (double)tri_valid(A.nf, k, A.F)) / A.ktot;
    };
    for (int k = lane; k <= N / 2; k += NT) {
      if (k == 0) {
        cx<double> a = buf[lp<double>(0)];
        const double y0 = (a.x + a.y) * mask_at(0);
        const double yN = (a.x - a.y) * mask_at(N);
        buf[lp<double>(0)] = {0.5 * (y0 + yN), 0.5 * (y0 - yN)};
      } else {
        cx<double> a = buf[lp<double>(k)], b = buf[lp<double>(N - k)];
        cx<double> w = tw[k];
        cx<double> E = {(a.x + b.x) * 0.5, (a.y - b.y) * 0.5};
        cx<double> O = {(a.y + b.y) * 0.5, (b.x - a.x) * 0.5};
        cx<double> wO = cmul(w, O);
        const double mk = mask_at(k), mn = mask_at(N - k);
        cx<double> Yk = {(E.x + wO.x) * mk, (E.y + wO.y) * mk};
        cx<double> Yn = {(E.x - wO.x) * mn, (-E.y + wO.y) * mn};
        cx<double> Ep = {(Yk.x + Yn.x) * 0.5, (Yk.y - Yn.y) * 0.5};
        cx<double> D = {(Yk.x - Yn.x) * 0.5, (Yk.y + Yn.y) * 0.5};
        cx<double> wc = {w.x, -w.y};
        cx<double> Op = cmul(D, wc);
        buf[lp<double>(k)] = {Ep.x - Op.y, Ep.y + Op.x};
        if (k != N - k) buf[lp<double>(N - k)] = {Ep.x + Op.y, -Ep.y + Op.x};
      }
    }
    team_sync<SY>();
    wave_fft<double, N, true, NT, SY>(buf, tw, lane);
    float2* srow = reinterpret_cast<float2*>(A.seg + (U.srow + t - (U.ta0 + 1)) * (int64_t)A.n);
    const double inv = 1.0 / (double)N;
    for (int j = lane; j < N; j += NT) {
      const cx<double> z = buf[lp<double>(j)];
      srow[j] = make_float2((float)(z.x * A.wfull[2 * j] * inv), (float)(z.y * A.wfull[2 * j + 1] * inv));
    }
    team_sync<SY>();
  }
}

// ---- overlap-add of the newly final samples, partial sums of the open ones, state update ----------------------------
// Sample p sums its frames in frame order, continuing the partial sum an earlier step left in the carry: the additions
// are the same whatever the block split.  out = sum seg / sum w^2 (k_rg_ola); positions >= Lout are the zero tail.
__global__ __launch_bounds__(256) void k_st_finish(StArgs A) {
  if ((int64_t)blockIdx.x >= A.n_fin) return;
  const StTile tl = A.tiles[A.t_fin + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  if (tl.kind == ST_CLEAR) {
    for (int f = threadIdx.x; f < A.FS; f += blockDim.x) A.rmax[(int64_t)U.state * A.FS + f] = 0.0;
    return;
  }
  const int64_t p = tl.a + threadIdx.x;
  if (p >= tl.b) return;
  if (tl.kind == ST_APPEND) {
    A.ring[(int64_t)U.state * A.RC + p % A.RC] = load_sample(A.x, A.in_dtype, U.in_off + (p - U.n0));
    return;
  }
  const double* cold = A.carry + ((int64_t)U.state * 2 + U.par) * A.W;
  double* cnew = A.carry + ((int64_t)U.state * 2 + (U.par ^ 1)) * A.W;
  const int64_t e = p + A.padL;
  int64_t t_hi = e / A.H;
  if (t_hi > U.Tend - 1) t_hi = U.Tend - 1;
  const int64_t t_lo = (e - A.W + 1 <= 0) ? 0 : (e - A.W + A.H) / A.H;
  double acc = p < U.cov0 ? cold[p % A.W] : 0.0;
  const int64_t ta = t_lo > U.ta0 + 1 ? t_lo : U.ta0 + 1, tb = t_hi < U.ta1 ? t_hi : U.ta1;
  for (int64_t t = ta; t <= tb; ++t)
    acc += (double)A.seg[(U.srow + t - (U.ta0 + 1)) * (int64_t)A.n + (int)(e - t * A.H)];
  if (p >= U.E1) {
    cnew[p % A.W] = acc;
    return;
  }
  double val = 0.0;
  if (!U.flush || p < U.Lout) {
    double norm = 0.0;
    for (int64_t t = t_lo; t <= t_hi; ++t) {
      const int m = (int)(e - t * A.H);
      norm += A.wfull[m] * A.wfull[m];
    }
    val = norm > 1e-10 ? acc / norm : acc;
  }
  store_sample(A.out, A.out_dtype, U.out_off + (p - U.E0), (float)val);
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct StSlot {
  int64_t n = 0, td = -1, ts = -1, ta = -1, E = 0;
  int par = 0;
  bool has_thr = false;
};

struct StBank {
  RgCtx c{};
  int n_slots = 0, C = 0, RC = 0, RB = 0, wpr = 0;
  int ns = 0, L = 0, RF = 0;   // non-stationary bank, its lookahead in frames, depth of the A / fwd ring
  int64_t max_block = 0;
  double *ring = nullptr, *rmax = nullptr, *carry = nullptr, *thr = nullptr, *T2 = nullptr, *stage = nullptr;
  double *fst = nullptr, *fa = nullptr;
  float* mk = nullptr;
  unsigned long long* bits = nullptr;
  int32_t* slot_list = nullptr;
  void* tabs = nullptr;
  size_t tabs_bytes = 0;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  std::vector<StSlot> slots;
};

static int64_t st_fdiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static int64_t st_cdiv(int64_t a, int64_t b) { return -st_fdiv(-a, b); }
static size_t st_al(size_t b) { return (b + 255) & ~(size_t)255; }

static int64_t st_tdec(int W, int H, int64_t n) {
  const int64_t a = n + W / 2 - W;
  return a < 0 ? -1 : a / H;
}

int64_t st_emitted(int W, int H, int nt, int64_t n) {
  const int64_t e = (st_tdec(W, H, n) - nt + 1) * (int64_t)H - W / 2;
  return e > 0 ? e : 0;
}

void st_destroy(StBank* b) {
  if (!b) return;
  for (void* p : {(void*)b->ring, (void*)b->rmax, (void*)b->carry, (void*)b->thr, (void*)b->T2, (void*)b->stage, (void*)b->bits,
                  (void*)b->fst, (void*)b->fa, (void*)b->mk, (void*)b->slot_list, b->tabs, b->ws})
    if (p) (void)hipFree(p);
  delete b;
}

namespace {
constexpr int FPT = 2;     // frames per apply tile
constexpr int RPT = 16;    // rows per smoothing tile
constexpr size_t WS_PREALLOC = (size_t)256 << 20;

bool geom_ok(const RgCtx& c) { return c.N == 128 || c.N == 256 || c.N == 512 || c.N == 1024 || c.N == 2048; }

// frames one step can decide or apply for a stream: those of max_block samples plus the zero-extended ones of a flush
int64_t max_frames(const RgCtx& c, int64_t max_block) { return (max_block + c.W / 2) / c.H + 3; }

int grow(void** p, size_t* have, size_t need, hipStream_t st, std::string* err, const char* what) {
  if (*have >= need) return SG_OK;
  if (*p) { (void)hipStreamSynchronize(st); (void)hipFree(*p); *p = nullptr; *have = 0; }
  if (hipMalloc(p, need) != hipSuccess) {
    *p = nullptr;
    char b[160];
    snprintf(b, sizeof b, "sg_stream_push: %s allocation of %zu bytes failed", what, need);
    *err = b;
    return SG_E_NOMEM;
  }
  *have = need;
  return SG_OK;
}

struct Prof {
  const RgCtx& c;
  void* tok;
  Prof(const RgCtx& c_, int stage, hipStream_t st) : c(c_), tok(c_.prof_begin ? c_.prof_begin(c_.hook_ctx, stage, st) : nullptr) {}
  ~Prof() { if (c.prof_end) c.prof_end(tok); }
};

// which: 0 = k_st_decide, 1 = k_st_apply<N, false>, 2 = k_sn_decide, 3 = k_st_apply<N, true>
template <int N>
hipError_t launch_fft_kernel(const StArgs& A, int which, unsigned grid, hipStream_t st) {
  const size_t lds = (size_t)(N + lpn<double>(N)) * sizeof(cx<double>);
  const void* k = which == 0   ? reinterpret_cast<const void*>(k_st_decide<N>)
                  : which == 1 ? reinterpret_cast<const void*>(k_st_apply<N, false>)
                  : which == 2 ? reinterpret_cast<const void*>(k_sn_decide<N>)
                               : reinterpret_cast<const void*>(k_st_apply<N, true>);
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const dim3 blk(st_nt<N>());
  if (which == 0) hipLaunchKernelGGL(k_st_decide<N>, dim3(grid), blk, lds, st, A);
  else if (which == 1) hipLaunchKernelGGL((k_st_apply<N, false>), dim3(grid), blk, lds, st, A);
  else if (which == 2) hipLaunchKernelGGL(k_sn_decide<N>, dim3(grid), blk, lds, st, A);
  else hipLaunchKernelGGL((k_st_apply<N, true>), dim3(grid), blk, lds, st, A);
  return hipGetLastError();
}

hipError_t launch_fft(int N, const StArgs& A, int which, int64_t ntiles, hipStream_t st) {
  const unsigned grid = (unsigned)std::max<int64_t>(1, ntiles);
  switch (N) {
    case 128: return launch_fft_kernel<128>(A, which, grid, st);
    case 256: return launch_fft_kernel<256>(A, which, grid, st);
    case 512: return launch_fft_kernel<512>(A, which, grid, st);
    case 1024: return launch_fft_kernel<1024>(A, which, grid, st);
    case 2048: return launch_fft_kernel<2048>(A, which, grid, st);
  }
  return hipErrorInvalidValue;
}

int check_slots(const StBank* b, const int32_t* slots, int32_t n, const char* who, std::string* err) {
  if (n < 0 || (n > 0 && !slots)) { *err = std::string(who) + ": bad slot list"; return SG_E_INVALID; }
  for (int32_t i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= b->n_slots) {
      char m[160];
      snprintf(m, sizeof m, "%s: unknown slot %d (the bank has %d)", who, slots[i], b->n_slots);
      *err = m;
      return SG_E_INVALID;
    }
  return SG_OK;
}
}  // namespace

int64_t st_state_bytes(const RgCtx& c, bool ns, int64_t n_slots, int64_t channels, int64_t max_block, int64_t L) {
  const int64_t nu = n_slots * channels, mf = max_frames(c, max_block);
  const int64_t RC = c.W + (c.nt + L + 1) * c.H, RB = 2 * (int64_t)c.nt + 1 + L + mf;
  int64_t per = RC * 8 + 2 * (int64_t)c.W * 8;
  if (ns) per += (int64_t)c.FS * 8 + (L + 1 + mf) * 2 * c.FS * 8 + RB * c.FS * 4;
  else per += (int64_t)c.FS * 8 + RB * ((c.F + 63) / 64) * 8;
  return nu * per;
}

int st_create(StBank** out, const RgCtx& c, int32_t n_slots, int32_t channels, int64_t max_block, bool ns, int32_t lookahead,
              std::string* err) {
  if (!geom_ok(c)) { *err = "sg_stream_create: n_fft must be a power of two from 256 to 4096"; return SG_E_UNSUPPORTED; }
  if (!ns && !c.stationary) {
    *err = "sg_stream_create: a non-stationary handle streams through sg_stream_create_nonstationary";
    return SG_E_INVALID;
  }
  if (ns && c.stationary) { *err = "sg_stream_create_nonstationary: the handle is stationary"; return SG_E_INVALID; }
  // (one thread per band walks the L + 1 forward rows of every decided frame: the cap bounds a step's serial work)
  if (ns && (lookahead < 0 || lookahead > SG_STREAM_MAX_LOOKAHEAD)) {
    char m[120];
    snprintf(m, sizeof m, "sg_stream_create_nonstationary: lookahead_frames must be 0 .. %d", SG_STREAM_MAX_LOOKAHEAD);
    *err = m;
    return SG_E_INVALID;
  }
  if (n_slots < 1 || channels < 1 || max_block < 1 || (int64_t)n_slots * channels > (1 << 24)) {
    *err = "sg_stream_create: n_slots, channels and max_block must be at least 1";
    return SG_E_INVALID;
  }
  StBank* b = new StBank();
  b->c = c;
  b->n_slots = n_slots;
  b->C = channels;
  b->max_block = max_block;
  b->ns = ns ? 1 : 0;
  b->L = ns ? lookahead : 0;
  // (a flush decides the L frames a push holds back on top of the block's own: the mask rows are L deeper for it)
  const int64_t RC = c.W + ((int64_t)c.nt + b->L + 1) * c.H, RB = 2 * (int64_t)c.nt + 1 + b->L + max_frames(c, max_block);
  const int64_t RF = (int64_t)b->L + 1 + max_frames(c, max_block);
  if (ns && (RC > INT32_MAX || RF > INT32_MAX || RB > INT32_MAX)) {
    char m[200];
    snprintf(m, sizeof m, "sg_stream_create_nonstationary: max_block = %lld with lookahead_frames = %d needs rings deeper than 2^31",
             (long long)max_block, b->L);
    *err = m;
    delete b;
    return SG_E_INVALID;
  }
  b->RC = (int)RC;
  b->RB = (int)std::min<int64_t>(INT32_MAX, RB);
  b->RF = (int)RF;
  b->wpr = (c.F + 63) / 64;
  b->slots.assign(n_slots, StSlot());
  if (ns)
    for (auto& sl : b->slots) sl.has_thr = true;   // a non-stationary stream needs no noise profile
  const size_t nu = (size_t)n_slots * channels;
  bool ok = true;
  auto take = [&](void** p, size_t bytes, bool zero) {
    if (!ok) return;
    if (hipMalloc(p, bytes) != hipSuccess) { *p = nullptr; ok = false; return; }
    if (zero && hipMemset(*p, 0, bytes) != hipSuccess) ok = false;
  };
  take((void**)&b->ring, nu * b->RC * 8, false);
  take((void**)&b->carry, nu * 2 * c.W * 8, false);
  if (ns) {
    take((void**)&b->fst, nu * c.FS * 8, true);
    take((void**)&b->fa, nu * (size_t)b->RF * 2 * c.FS * 8, false);
    take((void**)&b->mk, nu * (size_t)b->RB * c.FS * 4, false);
  } else {
    take((void**)&b->rmax, nu * c.FS * 8, true);
    take((void**)&b->bits, nu * (size_t)b->RB * b->wpr * 8, false);
    take((void**)&b->thr, (size_t)n_slots * c.FS * 8, true);
    take((void**)&b->T2, (size_t)n_slots * c.FS * 8, true);
    take((void**)&b->stage, (size_t)c.FS * 8, true);
  }
  take((void**)&b->slot_list, (size_t)n_slots * 4, true);
  // tables and scratch of a typical step up front (a larger step grows them, which synchronises once)
  const int64_t mf = max_frames(c, max_block);
  b->tabs_bytes = st_al(nu * sizeof(StUnit)) + st_al(nu * 16 * sizeof(StTile));
  take(&b->tabs, b->tabs_bytes, false);
  const size_t per_unit = st_al((size_t)(mf + 2 * c.nt) * c.FS * 4) + st_al((size_t)mf * c.n * 4);
  b->ws_bytes = std::min<size_t>(WS_PREALLOC, nu * per_unit);
  take(&b->ws, b->ws_bytes, false);
  if (!ok) {
    char m[200];
    snprintf(m, sizeof m, "sg_stream_create: device allocation failed (the bank's state is %lld bytes)",
             (long long)st_state_bytes(c, ns, n_slots, channels, max_block, b->L));
    st_destroy(b);
    *err = m;
    return SG_E_NOMEM;
  }
  *out = b;
  return SG_OK;
}

int st_set_threshold(StBank* b, const int32_t* slots, int32_t n, const double* thresh_dev, const double* thresh_host,
                     hipStream_t st, std::string* err) {
  int rc = check_slots(b, slots, n, "sg_stream_set_threshold", err);
  if (rc) return rc;
  if (b->ns) { *err = "sg_stream_set_threshold: a non-stationary bank takes no noise threshold"; return SG_E_INVALID; }
  if (n > b->n_slots) { *err = "sg_stream_set_threshold: more slots listed than the bank has"; return SG_E_INVALID; }
  if (n == 0) return SG_OK;
  const double* src = thresh_dev;
  if (thresh_host) {
    if (hipMemcpyAsync(b->stage, thresh_host, (size_t)b->c.F * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
      *err = "sg_stream_set_threshold: threshold upload failed";
      return SG_E_HIP;
    }
    src = b->stage;
  }
  if (hipMemcpyAsync(b->slot_list, slots, (size_t)n * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
    *err = "sg_stream_set_threshold: slot list upload failed";
    return SG_E_HIP;
  }
  hipLaunchKernelGGL(k_st_thresh, dim3(n), dim3(64), 0, st, src, b->slot_list, b->thr, b->T2, b->c.F,
                     b->c.FS, b->c.mag_scale);
  if (hipGetLastError() != hipSuccess) { *err = "sg_stream_set_threshold: launch failed"; return SG_E_HIP; }
  for (int32_t i = 0; i < n; ++i) b->slots[slots[i]].has_thr = true;
  return SG_OK;
}

int st_reset(StBank* b, const int32_t* slots, int32_t n, hipStream_t st, std::string* err) {
  int rc = check_slots(b, slots, n, "sg_stream_reset", err);
  if (rc) return rc;
  for (int32_t i = 0; i < n; ++i) {
    // (the ring, the bit rows and the carry need no clearing: a fresh stream reads none of them before it writes them)
    // (nor does the forward state of a non-stationary unit: frame 0 seeds it)
    if (!b->ns &&
        hipMemsetAsync(b->rmax + (size_t)slots[i] * b->C * b->c.FS, 0, (size_t)b->C * b->c.FS * 8, st) != hipSuccess) {
      *err = "sg_stream_reset: hipMemsetAsync failed";
      return SG_E_HIP;
    }
    const bool thr = b->slots[slots[i]].has_thr;
    b->slots[slots[i]] = StSlot();
    b->slots[slots[i]].has_thr = thr;
  }
  return SG_OK;
}

int64_t st_bank_emitted(const StBank* b, int64_t n) { return st_emitted(b->c.W, b->c.H, b->c.nt + b->L, n); }

int st_counters(const StBank* b, int32_t slot, int64_t* n, int64_t* emitted, std::string* err) {
  if (slot < 0 || slot >= b->n_slots) { *err = "sg_stream_counters: unknown slot"; return SG_E_INVALID; }
  *n = b->slots[slot].n;
  *emitted = b->slots[slot].E;
  return SG_OK;
}

int st_push(StBank* b, const void* in_dev, int in_dtype, void* out_dev, int out_dtype, const sg_stream_rec* recs,
            int32_t n_recs, hipStream_t st, std::string* err) {
  const RgCtx& c = b->c;
  const int h = c.W / 2;
  char msg[200];
  // ---- every argument is checked before any device work or state change
  std::vector<char> seen(b->n_slots, 0);
  for (int32_t i = 0; i < n_recs; ++i) {
    const sg_stream_rec& r = recs[i];
    if (r.slot < 0 || r.slot >= b->n_slots) {
      snprintf(msg, sizeof msg, "sg_stream_push: record %d: unknown slot %d (the bank has %d)", i, r.slot, b->n_slots);
      *err = msg;
      return SG_E_INVALID;
    }
    if (seen[r.slot]) {
      snprintf(msg, sizeof msg, "sg_stream_push: slot %d appears twice in one step", r.slot);
      *err = msg;
      return SG_E_INVALID;
    }
    seen[r.slot] = 1;
    if (r.n_samples < 0 || r.n_samples > b->max_block) {
      snprintf(msg, sizeof msg, "sg_stream_push: slot %d: block of %lld samples (max_block is %lld)", r.slot,
               (long long)r.n_samples, (long long)b->max_block);
      *err = msg;
      return SG_E_INVALID;
    }
    if (r.in_offset < 0 || r.out_offset < 0 || (b->C > 1 && (r.in_stride < r.n_samples || r.out_stride < 0))) {
      snprintf(msg, sizeof msg, "sg_stream_push: slot %d: bad offsets / strides", r.slot);
      *err = msg;
      return SG_E_INVALID;
    }
    if (!b->slots[r.slot].has_thr) {
      snprintf(msg, sizeof msg, "sg_stream_push: slot %d has no noise threshold yet", r.slot);
      *err = msg;
      return SG_E_STATE;
    }
    if (r.flush && b->slots[r.slot].n + r.n_samples < c.W) {
      snprintf(msg, sizeof msg, "sg_stream_push: slot %d: a stream of %lld samples is shorter than win_length=%d", r.slot,
               (long long)(b->slots[r.slot].n + r.n_samples), c.W);
      *err = msg;
      return SG_E_INVALID;
    }
  }
  // ---- plan
  std::vector<StUnit> units;
  std::vector<StSlot> after(n_recs);
  int64_t mrows = 0, sframes = 0;
  const int64_t UNBOUNDED = (int64_t)1 << 60;
  for (int32_t i = 0; i < n_recs; ++i) {
    const sg_stream_rec& r = recs[i];
    const StSlot& S = b->slots[r.slot];
    StUnit U{};
    U.n0 = S.n;
    U.n1 = S.n + r.n_samples;
    U.td0 = S.td;
    U.ts0 = S.ts;
    U.ta0 = S.ta;
    U.E0 = S.E;
    U.flush = r.flush ? 1 : 0;
    if (r.flush) {
      const int64_t T = (U.n1 + 2 * (int64_t)h - c.W) / c.H + 1;
      U.Tend = T;
      U.Lout = (T - 1) * c.H + c.W - 2 * (int64_t)h;
      U.td1 = T - 1;
      U.ts1 = T - 1;
      U.ta1 = T - 1;
      U.E1 = U.n1;
    } else {
      U.Tend = UNBOUNDED;
      U.Lout = UNBOUNDED;
      U.td1 = std::max(U.td0, st_tdec(c.W, c.H, U.n1));
      U.ts1 = std::max(U.ts0, U.td1 - b->L);
      U.ta1 = std::max(U.ta0, U.ts1 - c.nt);
      U.E1 = std::max<int64_t>(0, (U.ta1 + 1) * c.H - h);
    }
    U.cov0 = U.ta0 >= 0 ? U.ta0 * c.H - h + c.W : 0;
    if (U.ta1 > U.ta0) {
      U.r0 = std::max<int64_t>(0, U.ta0 + 1 - c.nt);
      U.r1 = std::min<int64_t>(U.Tend, U.ta1 + c.nt + 1);
    }
    U.slot = r.slot;
    U.par = S.par;
    for (int ch = 0; ch < b->C; ++ch) {
      StUnit V = U;
      V.state = r.slot * b->C + ch;
      V.in_off = r.in_offset + (int64_t)ch * r.in_stride;
      V.out_off = r.out_offset + (int64_t)ch * r.out_stride;
      V.mrow = mrows; mrows += V.r1 - V.r0;
      V.srow = sframes; sframes += V.ta1 - V.ta0;
      units.push_back(V);
    }
    StSlot& N = after[i];
    N.has_thr = true;
    if (!r.flush) {
      N.n = U.n1; N.td = U.td1; N.ts = U.ts1; N.ta = U.ta1; N.E = U.E1;
      N.par = U.ta1 > U.ta0 ? (S.par ^ 1) : S.par;
    }
  }
  std::vector<StTile> tiles;
  auto push = [&](size_t u, int kind, int64_t a, int64_t e) { tiles.push_back(StTile{(int32_t)u, kind, a, e}); };
  StArgs A{};
  A.t_dec = 0;
  for (size_t u = 0; u < units.size(); ++u)
    if (units[u].td1 > units[u].td0 || units[u].ts1 > units[u].ts0) push(u, 0, units[u].td0 + 1, units[u].td1 + 1);
  A.n_dec = (int64_t)tiles.size();
  A.t_fs = (int64_t)tiles.size();
  for (size_t u = 0; u < units.size(); ++u)
    for (int64_t r = units[u].r0; r < units[u].r1; r += RPT) push(u, 0, r, std::min(units[u].r1, r + RPT));
  A.n_fs = (int64_t)tiles.size() - A.t_fs;
  A.t_ap = (int64_t)tiles.size();
  for (size_t u = 0; u < units.size(); ++u)
    for (int64_t t = units[u].ta0 + 1; t <= units[u].ta1; t += FPT) push(u, 0, t, std::min(units[u].ta1 + 1, t + FPT));
  A.n_ap = (int64_t)tiles.size() - A.t_ap;
  A.t_fin = (int64_t)tiles.size();
  for (size_t u = 0; u < units.size(); ++u) {
    const StUnit& U = units[u];
    // newly final samples [E0, E1) and the open ones up to the last applied frame's end (a flush closes every sample,
    // also when its last frame was applied before)
    if (U.ta1 > U.ta0 || U.flush) {
      const int64_t end = U.flush ? U.E1 : std::max(U.E1, U.ta1 * c.H - h + c.W);
      for (int64_t p = U.E0; p < end; p += 256) push(u, ST_OLA, p, std::min(end, p + 256));
    }
    if (!U.flush)
      for (int64_t p = std::max(U.n0, U.n1 - b->RC); p < U.n1; p += 256) push(u, ST_APPEND, p, std::min(U.n1, p + 256));
    else if (!b->ns)
      push(u, ST_CLEAR, 0, 0);
  }
  A.n_fin = (int64_t)tiles.size() - A.t_fin;
  // ---- tables and scratch
  const size_t ub = st_al(units.size() * sizeof(StUnit)), tb = st_al(tiles.size() * sizeof(StTile));
  int rc = grow(&b->tabs, &b->tabs_bytes, ub + tb, st, err, "table");
  if (rc) return rc;
  const size_t Rb = st_al((size_t)mrows * c.FS * 4), Sb = st_al((size_t)sframes * c.n * 4);
  if ((rc = grow(&b->ws, &b->ws_bytes, Rb + Sb, st, err, "workspace"))) return rc;
  if (!units.empty()) {
    std::vector<char> host(ub + tb);
    memcpy(host.data(), units.data(), units.size() * sizeof(StUnit));
    if (!tiles.empty()) memcpy(host.data() + ub, tiles.data(), tiles.size() * sizeof(StTile));
    // (pageable host memory: hipMemcpyAsync has staged it before returning, so the vector may go)
    if (hipMemcpyAsync(b->tabs, host.data(), host.size(), hipMemcpyHostToDevice, st) != hipSuccess) {
      *err = "sg_stream_push: table upload failed";
      return SG_E_HIP;
    }
  }
  A.x = in_dev; A.in_dtype = in_dtype; A.out = out_dev; A.out_dtype = out_dtype;
  A.units = (const StUnit*)b->tabs;
  A.tiles = (const StTile*)((char*)b->tabs + ub);
  A.tw = (const cx<double>*)c.tw64; A.wfull = c.wfull64;
  A.ring = b->ring; A.bits = b->bits; A.rmax = b->rmax; A.carry = b->carry; A.thr = b->thr; A.T2 = b->T2;
  A.R = (float*)b->ws; A.seg = (float*)((char*)b->ws + Rb);
  A.n = c.n; A.W = c.W; A.H = c.H; A.F = c.F; A.FS = c.FS; A.padL = c.padL; A.wpr = b->wpr; A.RC = b->RC; A.RB = b->RB;
  A.nf = c.nf; A.nt = c.nt;
  A.mag_scale = c.mag_scale; A.top_db = c.top_db; A.prop = c.prop;
  A.ktot = (double)((int64_t)(c.nf + 1) * (c.nf + 1) * (int64_t)(c.nt + 1) * (c.nt + 1));
  A.fst = b->fst; A.fa = b->fa; A.mk = b->mk; A.RF = b->RF; A.L = b->L;
  A.iir_b = c.iir_b; A.nthresh = (float)c.nthresh; A.slope = (float)c.slope;
  const bool ns = b->ns != 0;
  // ---- the step: the same four launches whatever was pushed
  auto grid = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, n)); };
  hipError_t e = hipSuccess;
  { Prof pr(c, SG_STAGE_RG_DECIDE, st); e = launch_fft(c.N, A, ns ? 2 : 0, A.n_dec, st); }
  if (e == hipSuccess) {
    Prof pr(c, SG_STAGE_RG_FSMOOTH, st);
    if (ns) hipLaunchKernelGGL(k_st_fsmooth<true>, grid(A.n_fs), dim3(256), 0, st, A);
    else hipLaunchKernelGGL(k_st_fsmooth<false>, grid(A.n_fs), dim3(256), 0, st, A);
    e = hipGetLastError();
  }
  if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_APPLY, st); e = launch_fft(c.N, A, ns ? 3 : 1, A.n_ap, st); }
  if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_OLA, st); hipLaunchKernelGGL(k_st_finish, grid(A.n_fin), dim3(256), 0, st, A); e = hipGetLastError(); }
  if (e != hipSuccess) {
    *err = std::string("sg_stream_push: launch failed: ") + hipGetErrorString(e);
    return SG_E_HIP;
  }
  for (int32_t i = 0; i < n_recs; ++i) b->slots[recs[i].slot] = after[i];
  return SG_OK;
}
}  // namespace sg
