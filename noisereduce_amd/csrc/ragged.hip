// Ragged batches of recordings (sg_process_clips): tables, kernels and the host side of the batched path.  See
// ragged.hpp and DESIGN section 11.
//
// Every kernel reads a tile table: tile i = {index (unit or noise source), first, end} -- frames for the transform
// kernels, rows for the frequency smoothing, bands for the recurrence, output samples for the overlap-add.  One wavefront
// per workgroup for the transforms (wave-private LDS buffer: no barrier between passes, fft_wave.hpp SY = 1); nothing
// waits on another workgroup, and every cross-frame reduction is either exact (maxima as integer atomics on the bit
// patterns of non-negative doubles) or serial within one unit / one noise source.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fft_wave.hpp"
#include "geom.hpp"
#include "thresh.hpp"
#include "ragged.hpp"
#include "../../include/mi355gate_debug.h"

namespace sg {

// ---- tables ------------------------------------------------------------------------------------------------------
struct RgUnit {
  int64_t x_off;       // element of x holding clip sample 0 of this unit's channel
  int64_t n;           // clip samples per channel
  int64_t win0;        // clip index of unit sample 0 (chunk * chunk_size - padding)
  int64_t Lp, T, Lout; // window length, frames (n_frames_for), valid ISTFT samples
  int64_t k0, k1;      // kept unit positions [k0, k1)
  int64_t out_off;     // element of out receiving unit position k0
  int64_t d0, d1;      // data frames: windows that reach a readable sample (all others transform to exactly 0)
  int64_t l0, l1;      // live frames: frames that reach a kept sample
  int64_t r0, r1;      // mask rows the time smoothing of the live frames reads: [l0 - nt, l1 + nt) within [0, T)
  int64_t drow;        // first row of this unit's data frames in the bits / magnitude fields
  int64_t frow;        // first row of the forward-recurrence field (non-stationary: frames [d0, T))
  int64_t mrow;        // first row of this unit's mask rows (sigmoid / smoothed fields)
  int64_t srow;        // first live frame in the segment field
  int32_t noise;       // local noise index (stationary)
  int32_t pad_;
};
struct RgNoise {
  int64_t off, n, stride;
  int32_t C, in_x;
  int64_t T;           // frames of the noise clip
  int64_t prow;        // first row in the noise power field
  int64_t gidx;        // index in the caller's noise table (threshold tap)
};
struct RgTile {
  int32_t idx, pad_;
  int64_t a, b;
};

struct RgArgs {
  const void* x; int in_dtype;
  const void* xn; int noise_dtype;
  void* out; int out_dtype;
  const RgUnit* units;
  const RgNoise* noises;
  const RgTile* tiles;           // all tile lists, back to back
  int64_t t_np, n_np;            // noise power tiles (first, count)
  int64_t t_nf, n_nf;            // noise final tiles (noise, band block)
  int64_t t_dec, n_dec;          // data-frame tiles
  int64_t t_iir, n_iir;          // recurrence tiles (unit, band block)
  int64_t t_fs, n_fs;            // frequency smoothing tiles (unit, rows)
  int64_t t_ap, n_ap;            // live-frame tiles
  int64_t t_ola, n_ola;          // output tiles (unit, positions)
  const cx<double>* tw;
  const double* wfull;
  double* Pn;                    // [noise rows][FS] float64 noise power
  double* T2n;                   // [local noise][FS] compare constant from the threshold alone
  double* thr_all;               // [caller noise][FS] thresholds (tap)
  unsigned long long* pmax;      // [units][FS] band maxima of the unit's power (bit patterns)
  unsigned long long* bits;      // [data rows][wpr]
  float* mag;                    // [data rows][FS] (non-stationary)
  float* fw;                     // [forward rows][FS] (non-stationary)
  float* sig;                    // [mask rows][FS] (non-stationary raw mask)
  float* R;                      // [mask rows][FS] frequency-smoothed mask
  float* seg;                    // [live frames][n]
  int n, W, H, F, FS, padL, wpr;
  double mag_scale, top_db, n_std, prop, iir_b, nthresh, slope;
  int ddof, nf, nt, stationary;
  double ktot;
};

// sigmoid(((A - S) / S - thresh) * slope) as kernels.hpp sigmoid_ratio computes it (that header holds non-template kernels)
__device__ __forceinline__ float rg_sigmoid_ratio(double av, double s, float nthresh, float slope) {
  const float ratio = (float)(av - s) / (float)s;
  return 1.0f / (1.0f + __expf(-(ratio - nthresh) * slope));
}

__device__ __forceinline__ double rg_nan_if_nonfinite(double P) { return (P <= 1.79769313486231570e308) ? P : (double)NAN; }

// threads per frame: one wavefront up to N = 512 (wave-private buffer, SY = 1: no barrier between passes); the whole
// 256-thread workgroup from N = 1024 on, where a wavefront's share of a float64 transform would not fit its registers
template <int N>
constexpr int rg_nt() { return N <= 512 ? 64 : 256; }
template <int N>
constexpr int rg_sy() { return rg_nt<N>() <= 64 ? 1 : rg_nt<N>(); }

// window * frame of the unit (frame t: unit samples [t H - padL, t H - padL + n)) into the wave's buffer, forward
// transform, in place.  Samples outside the window or outside the clip read as 0 (SpectralGate._read_chunk).
template <int N>
__device__ __forceinline__ void rg_unit_fft(const RgArgs& A, const RgUnit& U, int64_t t, cx<double>* buf,
                                            const cx<double>* tw, int lane) {
  constexpr int NT = rg_nt<N>(), SY = rg_sy<N>();
  const int64_t s0 = t * A.H - A.padL;
  for (int j = lane; j < N; j += NT) {
    double v[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t s = s0 + 2 * j + q;
      const int64_t g = U.win0 + s;
      v[q] = (s >= 0 && s < U.Lp && g >= 0 && g < U.n) ? load_sample(A.x, A.in_dtype, U.x_off + g) : 0.0;
    }
    buf[lp<double>(j)] = {v[0] * A.wfull[2 * j], v[1] * A.wfull[2 * j + 1]};
  }
  team_sync<SY>();
  wave_fft<double, N, false, NT, SY>(buf, tw, lane);
}

// bin k (0..N) of the real transform held packed in buf
template <int N>
__device__ __forceinline__ cx<double> rg_bin(const cx<double>* buf, const cx<double>* tw, int k) {
  cx<double> a = buf[lp<double>(k == N ? 0 : k)];
  cx<double> b = buf[lp<double>((k == 0 || k == N) ? 0 : N - k)];
  return rfft_bin(a, b, tw[k == N ? 0 : k], k, N);
}

template <int N>
__device__ __forceinline__ void rg_stage(cx<double>* tw, const RgArgs& A) {
  stage_twiddles<rg_nt<N>(), N>(tw, A.tw, (int)threadIdx.x);
  __syncthreads();
}

// ---- stationary: noise statistics ----------------------------------------------------------------------------------
// power of every frame of every noise source: channel mean (sequential float64 sum / C, k_channel_mean), window, transform
template <int N>
__global__ __launch_bounds__(rg_nt<N>()) void k_rg_noise_power(RgArgs A) {
  constexpr int NT = rg_nt<N>(), SY = rg_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_np) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const RgTile tl = A.tiles[A.t_np + blockIdx.x];
  const RgNoise S = A.noises[tl.idx];
  const void* src = S.in_x ? A.x : A.xn;
  const int dt = S.in_x ? A.in_dtype : A.noise_dtype;
  rg_stage<N>(tw, A);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    const int64_t s0 = t * A.H - A.padL;
    for (int j = lane; j < N; j += NT) {
      double v[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int64_t s = s0 + 2 * j + q;
        double acc = 0.0;
        if (s >= 0 && s < S.n) {
          for (int c = 0; c < S.C; ++c) acc += load_sample(src, dt, S.off + c * S.stride + s);
          acc = acc / (double)S.C;
        }
        v[q] = acc;
      }
      buf[lp<double>(j)] = {v[0] * A.wfull[2 * j], v[1] * A.wfull[2 * j + 1]};
    }
    team_sync<SY>();
    wave_fft<double, N, false, NT, SY>(buf, tw, lane);
    double* row = A.Pn + (S.prow + t) * A.FS;
    for (int k = lane; k <= N; k += NT) {
      const cx<double> X = rg_bin<N>(buf, tw, k);
      row[k] = rg_nan_if_nonfinite(X.x * X.x + X.y * X.y);
    }
    team_sync<SY>();
  }
}

// one thread per (noise source, band): maximum, moments of the floored dB relative to it (k_row_decide's summation
// structure: d = max(dB - max_dB, -top_db), s1 = sum d, s2 = sum d^2, serial over the frames), threshold, and the compare
// constant of the threshold alone (k_t2_rows without the floor: the floor is a per-(unit, band) override, k_rg_fsmooth)
__global__ __launch_bounds__(64) void k_rg_noise_final(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_nf) return;
  const RgTile tl = A.tiles[A.t_nf + blockIdx.x];
  const int f = (int)tl.a + (int)threadIdx.x;
  if (f >= A.F) return;
  const RgNoise S = A.noises[tl.idx];
  const double* col = A.Pn + S.prow * A.FS + f;
  double m = 0.0;
  for (int64_t t = 0; t < S.T; ++t) m = nanmax(m, col[t * A.FS]);
  const double mdb = cell_db(m, A.mag_scale);
  double s1 = 0.0, s2 = 0.0;
  for (int64_t t = 0; t < S.T; ++t) {
    double d = cell_db(col[t * A.FS], A.mag_scale) - mdb;
    d = (d != d) ? d : fmax(d, -A.top_db);
    s1 += d;
    s2 += d * d;
  }
  const double Tn = (double)S.T;
  const double mean_d = s1 / Tn;
  double var = (s2 - s1 * s1 / Tn) / (Tn - (double)A.ddof);
  if (var < 0.0) var = 0.0;
  const double th = (mdb + mean_d) + sqrt(var) * A.n_std;
  const double eps = 2.220446049250313e-16;
  double t2;
  if (th != th) {
    t2 = T2_NEVER;
  } else if (20.0 * log10(eps) > th) {
    t2 = -1.0;
  } else {
    const double tm = (exp10(th / 20.0) - eps) / A.mag_scale;
    t2 = tm > 0.0 ? tm * tm : 0.0;
  }
  A.T2n[(int64_t)tl.idx * A.FS + f] = t2;
  A.thr_all[S.gidx * A.FS + f] = th;
}

// ---- per data frame: decision bits + band maxima (stationary) or magnitudes (non-stationary) ------------------------
template <int N>
__global__ __launch_bounds__(rg_nt<N>()) void k_rg_decide(RgArgs A) {
  constexpr int NT = rg_nt<N>(), SY = rg_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const RgTile tl = A.tiles[A.t_dec + blockIdx.x];
  const RgUnit U = A.units[tl.idx];
  rg_stage<N>(tw, A);
  constexpr int M = N / NT + 1;
  double vmax[M];
#pragma unroll
  for (int m = 0; m < M; ++m) vmax[m] = 0.0;
  const double* T2 = A.T2n + (int64_t)U.noise * A.FS;
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rg_unit_fft<N>(A, U, t, buf, tw, lane);
    const int64_t row = U.drow + (t - U.d0);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      double P = 0.0;
      if (k <= N) {
        const cx<double> X = rg_bin<N>(buf, tw, k);
        P = rg_nan_if_nonfinite(X.x * X.x + X.y * X.y);
      }
      if (A.stationary) {
        vmax[m] = nanmax(vmax[m], P);
        const unsigned long long word = __ballot(k <= N && P > T2[k]);
        if ((lane & 63) == 0 && (k >> 6) < A.wpr) A.bits[row * A.wpr + (k >> 6)] = word;
      } else if (k <= N) {
        A.mag[row * A.FS + k] = (float)sqrt(P);
      }
    }
    team_sync<SY>();
  }
  if (A.stationary) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      if (k <= N) atomicMax(&A.pmax[(int64_t)tl.idx * A.FS + k], (unsigned long long)__double_as_longlong(vmax[m]));
    }
  }
}

// ---- non-stationary: filtfilt(padtype=None) one-pole over the unit's frames + sigmoid (k_iir_sigmoid) -------------
// one thread per (unit, band); frames outside [d0, d1) have magnitude 0 and are stepped through all the same
__global__ __launch_bounds__(64) void k_rg_iir(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_iir) return;
  const RgTile tl = A.tiles[A.t_iir + blockIdx.x];
  const int f = (int)tl.a + (int)threadIdx.x;
  if (f >= A.F) return;
  const RgUnit U = A.units[tl.idx];
  auto mag_at = [&](int64_t t) -> double {
    return (t >= U.d0 && t < U.d1) ? (double)A.mag[(U.drow + t - U.d0) * A.FS + f] : 0.0;
  };
  const double b = A.iir_b, c = 1.0 - A.iir_b;
  double s = mag_at(0);
  for (int64_t t = 0; t < U.T; ++t) {
    s = b * mag_at(t) + c * s;
    if (t >= U.d0) A.fw[(U.frow + t - U.d0) * A.FS + f] = (float)s;
    // (before d0 every magnitude is 0 and so is s: the forward value is 0 there)
  }
  const double fprev = s;
  for (int64_t t = U.T - 1; t >= 0; --t) {
    double fwv = t >= U.d0 ? (double)A.fw[(U.frow + t - U.d0) * A.FS + f] : 0.0;
    if (t == U.T - 1) fwv = fprev;
    s = b * fwv + c * s;
    if (t >= U.r0 && t < U.r1) A.sig[(U.mrow + t - U.r0) * A.FS + f] = rg_sigmoid_ratio(mag_at(t), s, (float)A.nthresh, (float)A.slope);
  }
}

// ---- mask smoothing along frequency: R[row][f] = sum_df (nf + 1 - |df|) raw[row][f + df] ----------------------------
// Stationary raw mask: the decision bit, with the -top_db floor applied per (unit, band) from the unit's band maximum
// (k_t2_rows): floor above the threshold -> every cell of the band passes; NaN maximum or threshold -> none does.  Rows
// outside the data frames transform to exactly 0: their bit is 0 unless the band passes everywhere.
__global__ __launch_bounds__(256) void k_rg_fsmooth(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_fs) return;
  __shared__ unsigned char mode[2112];   // per band: 0 = decision bits, 1 = all pass, 2 = none passes (F <= 2049)
  const RgTile tl = A.tiles[A.t_fs + blockIdx.x];
  const RgUnit U = A.units[tl.idx];
  if (A.stationary) {
    const int64_t gi = A.noises[U.noise].gidx;
    for (int f = threadIdx.x; f < A.F; f += blockDim.x) {
      const double th = A.thr_all[gi * A.FS + f];
      const double t2 = A.T2n[(int64_t)U.noise * A.FS + f];   // < 0: 20 log10(eps) > thresh
      const double pm = __longlong_as_double((long long)A.pmax[(int64_t)tl.idx * A.FS + f]);
      const double fl = cell_db(pm, A.mag_scale) - A.top_db;
      mode[f] = (th != th || fl != fl) ? 2 : ((fl > th || t2 < 0.0) ? 1 : 0);
    }
  }
  __syncthreads();
  const int nf = A.nf;
  for (int64_t r = tl.a; r < tl.b; ++r) {
    const bool data = r >= U.d0 && r < U.d1;
    const unsigned long long* brow = A.bits + (U.drow + r - U.d0) * A.wpr;
    const float* srow = A.sig + (U.mrow + r - U.r0) * A.FS;
    float* out = A.R + (U.mrow + r - U.r0) * A.FS;
    for (int f = threadIdx.x; f < A.F; f += blockDim.x) {
      float acc = 0.f;
      for (int df = -nf; df <= nf; ++df) {
        const int g = f + df;
        if (g < 0 || g >= A.F) continue;
        float v;
        if (A.stationary) {
          const unsigned char md = mode[g];
          v = md == 1 ? 1.f : (md == 2 ? 0.f : (data ? (float)((brow[g >> 6] >> (g & 63)) & 1ull) : 0.f));
        } else {
          v = srow[g];
        }
        acc += (float)(nf + 1 - (df < 0 ? -df : df)) * v;
      }
      out[f] = acc;
    }
  }
}

// ---- live frames: time smoothing, masked multiply, inverse transform (k_apply_istft's split / mask / merge) ----------
template <int N>
__global__ __launch_bounds__(rg_nt<N>()) void k_rg_apply(RgArgs A) {
  constexpr int NT = rg_nt<N>(), SY = rg_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const RgTile tl = A.tiles[A.t_ap + blockIdx.x];
  const RgUnit U = A.units[tl.idx];
  rg_stage<N>(tw, A);
  const int nt = A.nt;
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rg_unit_fft<N>(A, U, t, buf, tw, lane);
    const int64_t ta = t - nt < 0 ? 0 : t - nt, tb = t + nt >= U.T ? U.T - 1 : t + nt;
    const double Et = (double)tri_valid(nt, t, U.T);
    auto mask_at = [&](int k) -> double {
      double K = 0.0;
      for (int64_t q = ta; q <= tb; ++q) {
        const int64_t d = q - t;
        K += (double)(nt + 1 - (d < 0 ? -d : d)) * (double)A.R[(U.mrow + q - U.r0) * A.FS + k];
      }
      if (A.stationary) return (A.prop * K + (1.0 - A.prop) * Et * (double)tri_valid(A.nf, k, A.F)) / A.ktot;
      return (K / A.ktot) * A.prop + (1.0 - A.prop);
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
    float2* srow = reinterpret_cast<float2*>(A.seg + (U.srow + t - U.l0) * (int64_t)A.n);
    const double inv = 1.0 / (double)N;
    for (int j = lane; j < N; j += NT) {
      const cx<double> z = buf[lp<double>(j)];
      srow[j] = make_float2((float)(z.x * A.wfull[2 * j] * inv), (float)(z.y * A.wfull[2 * j + 1] * inv));
    }
    team_sync<SY>();
  }
}

// ---- overlap-add of the kept samples (k_ola): out = sum seg / sum w^2; positions >= Lout are the zero tail -----------
__global__ __launch_bounds__(256) void k_rg_ola(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_ola) return;
  const RgTile tl = A.tiles[A.t_ola + blockIdx.x];
  const RgUnit U = A.units[tl.idx];
  const int64_t p = tl.a + threadIdx.x;
  if (p >= tl.b) return;
  double val = 0.0;
  if (p < U.Lout) {
    const int64_t e = p + A.padL;
    int64_t t_hi = e / A.H;
    if (t_hi > U.T - 1) t_hi = U.T - 1;
    int64_t t_lo = (e - A.n + A.H) / A.H;
    if (e - A.n + 1 <= 0) t_lo = 0;
    double acc = 0.0, norm = 0.0;
    for (int64_t t = t_lo; t <= t_hi; ++t) {
      const int m = (int)(e - t * A.H);
      acc += (double)A.seg[(U.srow + t - U.l0) * (int64_t)A.n + m];
      norm += A.wfull[m] * A.wfull[m];
    }
    val = norm > 1e-10 ? acc / norm : acc;
  }
  store_sample(A.out, A.out_dtype, U.out_off + (p - U.k0), (float)val);
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct RgState {
  void* ws = nullptr;
  size_t ws_bytes = 0;
  double* thr = nullptr;
  size_t thr_bytes = 0;
  int64_t last_noise = 0, last_batches = 0;
  int FS = 0;
};

void rg_free(RgState* s) {
  if (!s) return;
  if (s->ws) (void)hipFree(s->ws);
  if (s->thr) (void)hipFree(s->thr);
  delete s;
}

int64_t rg_last_batches(const RgState* s) { return s ? s->last_batches : 0; }

static int64_t fdiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static int64_t cdiv(int64_t a, int64_t b) { return -fdiv(-a, b); }

namespace {
struct Plan {
  std::vector<RgUnit> units;
  std::vector<int64_t> unit_clip;
  int64_t drows = 0, frows = 0, mrows = 0, sframes = 0;
};

constexpr int FPT = 8;     // frames per transform tile
constexpr int RPT = 16;    // rows per smoothing tile

// units of one clip (base.py:167-226): chunk grid or one window, one unit per channel
void plan_clip(const RgCtx& c, int64_t cs, int64_t pad, const sg_clip& cl, int32_t noise_local, Plan& P) {
  const int64_t n = cl.n;
  const bool chunked = cs > 0 && n > cs;
  const int64_t nch = chunked ? cdiv(n, cs) : 1;
  for (int32_t ch = 0; ch < cl.channels; ++ch) {
    for (int64_t i = 0; i < nch; ++i) {
      RgUnit U{};
      U.x_off = cl.x_offset + (int64_t)ch * cl.x_stride;
      U.n = n;
      U.win0 = chunked ? i * cs - pad : -pad;
      U.Lp = chunked ? cs + 2 * pad : n + 2 * pad;
      U.T = (U.Lp + 2 * (int64_t)(c.W / 2) - c.W) / c.H + 1;
      U.Lout = (U.T - 1) * c.H + c.W - 2 * (int64_t)(c.W / 2);
      U.k0 = pad;
      U.k1 = pad + (chunked ? std::min(cs, n - i * cs) : n);
      U.out_off = cl.out_offset + (int64_t)ch * cl.out_stride + (chunked ? i * cs : 0);
      // readable unit positions [a, b)
      const int64_t a = std::max<int64_t>(0, -U.win0), b = std::min<int64_t>(U.Lp, n - U.win0);
      U.d0 = std::max<int64_t>(0, fdiv(a + c.padL - c.W, c.H) + 1);
      U.d1 = std::min<int64_t>(U.T, cdiv(b + c.padL, c.H));
      if (U.d0 > U.T) U.d0 = U.T;
      if (U.d1 < U.d0) U.d1 = U.d0;
      const int64_t ke = std::min(U.k1, U.Lout);
      if (ke > U.k0) {
        int64_t lo = cdiv(U.k0 + c.padL - c.n + 1, c.H);
        U.l0 = std::max<int64_t>(0, lo);
        U.l1 = std::min<int64_t>(U.T - 1, (ke - 1 + c.padL) / c.H) + 1;
      } else {
        U.l0 = U.l1 = 0;
      }
      U.r0 = U.l1 > U.l0 ? std::max<int64_t>(0, U.l0 - c.nt) : 0;
      U.r1 = U.l1 > U.l0 ? std::min<int64_t>(U.T, U.l1 + c.nt) : 0;
      U.noise = noise_local;
      U.drow = P.drows; P.drows += U.d1 - U.d0;
      U.frow = P.frows; P.frows += c.stationary ? 0 : U.T - U.d0;
      U.mrow = P.mrows; P.mrows += U.r1 - U.r0;
      U.srow = P.sframes; P.sframes += U.l1 - U.l0;
      P.units.push_back(U);
    }
  }
}

size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

struct Layout {
  size_t tabs, Pn, T2n, pmax, bits, mag, fw, sig, R, seg, total;
};
Layout layout(const RgCtx& c, int64_t n_units, int64_t n_noise, int64_t noise_rows, int64_t drows, int64_t frows,
              int64_t mrows, int64_t sframes, int64_t n_tiles) {
  Layout L{};
  const int wpr = (c.F + 63) / 64;
  size_t o = 0;
  auto take = [&](size_t b) { size_t r = o; o += al(b); return r; };
  L.tabs = take((size_t)n_units * sizeof(RgUnit) + (size_t)n_noise * sizeof(RgNoise) + (size_t)n_tiles * sizeof(RgTile));
  L.Pn = take((size_t)noise_rows * c.FS * 8);
  L.T2n = take((size_t)n_noise * c.FS * 8);
  L.pmax = take(c.stationary ? (size_t)n_units * c.FS * 8 : 0);
  L.bits = take(c.stationary ? (size_t)drows * wpr * 8 : 0);
  L.mag = take(c.stationary ? 0 : (size_t)drows * c.FS * 4);
  L.fw = take((size_t)frows * c.FS * 4);
  L.sig = take(c.stationary ? 0 : (size_t)mrows * c.FS * 4);
  L.R = take((size_t)mrows * c.FS * 4);
  L.seg = take((size_t)sframes * c.n * 4);
  L.total = o;
  return L;
}

int64_t noise_frames(const RgCtx& c, int64_t n) { return (n + 2 * (int64_t)(c.W / 2) - c.W) / c.H + 1; }

// Exact size of a sub-batch's workspace (tables + fields, layout()): counts units, noise sources, field rows and tiles
// exactly as rg_process builds them.  The packer and sg_clips_workspace_bytes both use it, so a budget equal to the
// query's answer holds every clip in one sub-batch and a budget one byte smaller does not.
struct Sizer {
  int64_t nu = 0, nn = 0, noise_rows = 0, drows = 0, frows = 0, mrows = 0, sframes = 0, ntiles = 0;
  void add_noise(const RgCtx& c, int64_t T) {
    ++nn;
    noise_rows += T;
    ntiles += cdiv(T, FPT) + cdiv(c.F, 64);
  }
  void add_clip(const RgCtx& c, const sg_clip& cl) {
    Plan P;
    plan_clip(c, c.cs, c.pad, cl, 0, P);
    for (const RgUnit& U : P.units) {
      ++nu;
      ntiles += cdiv(U.d1 - U.d0, FPT) + cdiv(U.r1 - U.r0, RPT) + cdiv(U.l1 - U.l0, FPT) + cdiv(U.k1 - U.k0, 256);
      if (!c.stationary && U.r1 > U.r0) ntiles += cdiv(c.F, 64);
    }
    drows += P.drows; frows += P.frows; mrows += P.mrows; sframes += P.sframes;
  }
  Layout layout_of(const RgCtx& c) const { return layout(c, nu, nn, noise_rows, drows, frows, mrows, sframes, ntiles); }
};

template <int N>
hipError_t launch_fft_kernels(const RgCtx& c, const RgArgs& A, int which, unsigned grid, hipStream_t st) {
  const size_t lds = (size_t)(N + lpn<double>(N)) * sizeof(cx<double>);
  const void* k = which == 0 ? reinterpret_cast<const void*>(k_rg_noise_power<N>)
                : which == 1 ? reinterpret_cast<const void*>(k_rg_decide<N>)
                             : reinterpret_cast<const void*>(k_rg_apply<N>);
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const dim3 blk(rg_nt<N>());
  if (which == 0) hipLaunchKernelGGL(k_rg_noise_power<N>, dim3(grid), blk, lds, st, A);
  else if (which == 1) hipLaunchKernelGGL(k_rg_decide<N>, dim3(grid), blk, lds, st, A);
  else hipLaunchKernelGGL(k_rg_apply<N>, dim3(grid), blk, lds, st, A);
  return hipGetLastError();
}

hipError_t launch_fft(const RgCtx& c, const RgArgs& A, int which, int64_t ntiles, hipStream_t st) {
  const unsigned grid = (unsigned)std::max<int64_t>(1, ntiles);
  switch (c.N) {
    case 128: return launch_fft_kernels<128>(c, A, which, grid, st);
    case 256: return launch_fft_kernels<256>(c, A, which, grid, st);
    case 512: return launch_fft_kernels<512>(c, A, which, grid, st);
    case 1024: return launch_fft_kernels<1024>(c, A, which, grid, st);
    case 2048: return launch_fft_kernels<2048>(c, A, which, grid, st);
  }
  return hipErrorInvalidValue;
}

struct Prof {
  const RgCtx& c;
  void* tok;
  Prof(const RgCtx& c_, int stage, hipStream_t st) : c(c_), tok(c_.prof_begin ? c_.prof_begin(c_.hook_ctx, stage, st) : nullptr) {}
  ~Prof() { if (c.prof_end) c.prof_end(tok); }
};
}  // namespace

static bool geom_ok(const RgCtx& c, std::string* err) {
  if (c.N != 128 && c.N != 256 && c.N != 512 && c.N != 1024 && c.N != 2048) {
    *err = "sg_process_clips: n_fft must be a power of two from 256 to 4096";
    return false;
  }
  return true;
}

static int check_clips(const RgCtx& c, const sg_clip* clips, int64_t n_clips, int32_t n_noise, std::string* err) {
  for (int64_t i = 0; i < n_clips; ++i) {
    const sg_clip& cl = clips[i];
    if (cl.n < 1 || cl.channels < 1 || cl.x_offset < 0 || cl.out_offset < 0 || (cl.channels > 1 && (cl.x_stride < cl.n || cl.out_stride < cl.n))) {
      char b[160];
      snprintf(b, sizeof b, "sg_process_clips: clip %lld: bad geometry", (long long)i);
      *err = b;
      return SG_E_INVALID;
    }
    if (c.stationary && (cl.noise < 0 || cl.noise >= n_noise)) {
      char b[160];
      snprintf(b, sizeof b, "sg_process_clips: clip %lld: noise index %d out of range", (long long)i, cl.noise);
      *err = b;
      return SG_E_INVALID;
    }
  }
  return SG_OK;
}

int rg_workspace_bytes(const RgCtx& c, const sg_noise_src* noise, int32_t n_noise, const sg_clip* clips, int64_t n_clips,
                       int64_t* bytes, std::string* err) {
  if (!geom_ok(c, err)) return SG_E_UNSUPPORTED;
  int rc = check_clips(c, clips, n_clips, n_noise, err);
  if (rc) return rc;
  Sizer z;
  std::vector<char> seen(n_noise > 0 ? n_noise : 1, 0);
  for (int64_t i = 0; i < n_clips; ++i) {
    if (c.stationary && !seen[clips[i].noise]) {
      seen[clips[i].noise] = 1;
      z.add_noise(c, noise_frames(c, noise[clips[i].noise].n));
    }
    z.add_clip(c, clips[i]);
  }
  *bytes = (int64_t)z.layout_of(c).total;
  return SG_OK;
}

int rg_thresholds(RgState* s, double* host, int32_t n_noise, int32_t n_bins, hipStream_t st, std::string* err) {
  if (!s || !s->thr || n_noise != s->last_noise) {
    *err = "sg_debug_clip_thresholds: n_noise does not match the last sg_process_clips call";
    return SG_E_STATE;
  }
  if (hipStreamSynchronize(st) != hipSuccess) { *err = "hipStreamSynchronize failed"; return SG_E_HIP; }
  std::vector<double> tmp((size_t)n_noise * s->FS);
  if (!tmp.empty() && hipMemcpy(tmp.data(), s->thr, tmp.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) {
    *err = "hipMemcpy failed";
    return SG_E_HIP;
  }
  for (int32_t i = 0; i < n_noise; ++i)
    for (int32_t f = 0; f < n_bins; ++f) host[(size_t)i * n_bins + f] = tmp[(size_t)i * s->FS + f];
  return SG_OK;
}

int rg_process(RgState** sp, const RgCtx& c, const void* x_dev, int in_dtype, const void* noise_dev, int noise_dtype,
               const sg_noise_src* noise, int32_t n_noise, const sg_clip* clips, int64_t n_clips, void* out_dev,
               int out_dtype, int64_t max_ws, hipStream_t st, std::string* err) {
  if (!geom_ok(c, err)) return SG_E_UNSUPPORTED;
  int rc = check_clips(c, clips, n_clips, n_noise, err);
  if (rc) return rc;
  const int64_t cs = c.cs, pad = c.pad;
  if (c.stationary) {
    for (int32_t i = 0; i < n_noise; ++i) {
      if (noise[i].n < c.W || noise[i].channels < 1 || (noise[i].in_x == 0 && !noise_dev)) {
        char b[200];
        snprintf(b, sizeof b, "sg_process_clips: noise source %d: %lld samples (win_length=%d) / bad table entry", i,
                 (long long)noise[i].n, c.W);
        *err = b;
        return SG_E_INVALID;
      }
    }
  }
  if (!*sp) *sp = new RgState();
  RgState* S = *sp;
  S->FS = c.FS;
  S->last_noise = c.stationary ? n_noise : 0;
  S->last_batches = 0;
  if (c.stationary && n_noise > 0) {
    const size_t tb = (size_t)n_noise * c.FS * 8;
    if (S->thr_bytes < tb) {
      if (S->thr) { (void)hipStreamSynchronize(st); (void)hipFree(S->thr); S->thr = nullptr; S->thr_bytes = 0; }
      if (hipMalloc(&S->thr, tb) != hipSuccess) { S->thr = nullptr; *err = "threshold buffer allocation failed"; return SG_E_NOMEM; }
      S->thr_bytes = tb;
    }
  }
  if (max_ws <= 0) max_ws = (int64_t)4 << 30;
  // sub-batches: clips in order, greedily, under the budget (a clip that alone exceeds it is a sub-batch of its own)
  std::vector<int64_t> nrows_of(n_noise > 0 ? n_noise : 1, 0);
  for (int32_t i = 0; i < n_noise && c.stationary; ++i) nrows_of[i] = noise_frames(c, noise[i].n);
  int64_t i0 = 0;
  const int wpr = (c.F + 63) / 64;
  while (i0 < n_clips) {
    int64_t i1 = i0;
    Sizer z;
    std::vector<char> seen(n_noise > 0 ? n_noise : 1, 0);
    while (i1 < n_clips) {
      Sizer zn = z;
      const bool new_noise = c.stationary && !seen[clips[i1].noise];
      if (new_noise) zn.add_noise(c, nrows_of[clips[i1].noise]);
      zn.add_clip(c, clips[i1]);
      if (i1 > i0 && (int64_t)zn.layout_of(c).total > max_ws) break;
      z = zn;
      if (new_noise) seen[clips[i1].noise] = 1;
      ++i1;
    }
    if (z.nu > INT32_MAX || z.nn > INT32_MAX) {
      *err = "sg_process_clips: more than 2^31 - 1 units in one sub-batch";
      return SG_E_UNSUPPORTED;
    }
    // local noise table
    std::vector<int32_t> loc(n_noise > 0 ? n_noise : 1, -1);
    std::vector<RgNoise> noises;
    int64_t noise_rows = 0;
    Plan P;  // (z.nu <= INT32_MAX: the int32 indices of the tile table cannot wrap)
    for (int64_t i = i0; i < i1; ++i) {
      int32_t nl = 0;
      if (c.stationary) {
        const int32_t g = clips[i].noise;
        if (loc[g] < 0) {
          RgNoise N{};
          N.off = noise[g].offset; N.n = noise[g].n; N.stride = noise[g].stride; N.C = noise[g].channels;
          N.in_x = noise[g].in_x; N.T = nrows_of[g]; N.prow = noise_rows; N.gidx = g;
          noise_rows += N.T;
          loc[g] = (int32_t)noises.size();
          noises.push_back(N);
        }
        nl = loc[g];
      }
      plan_clip(c, cs, pad, clips[i], nl, P);
    }
    // tile lists
    std::vector<RgTile> tiles;
    auto push = [&](int64_t idx, int64_t a, int64_t b) { tiles.push_back(RgTile{(int32_t)idx, 0, a, b}); };
    RgArgs A{};
    A.t_np = (int64_t)tiles.size();
    for (size_t k = 0; k < noises.size(); ++k)
      for (int64_t t = 0; t < noises[k].T; t += FPT) push((int64_t)k, t, std::min<int64_t>(noises[k].T, t + FPT));
    A.n_np = (int64_t)tiles.size() - A.t_np;
    A.t_nf = (int64_t)tiles.size();
    for (size_t k = 0; k < noises.size(); ++k)
      for (int f = 0; f < c.F; f += 64) push((int64_t)k, f, f + 64);
    A.n_nf = (int64_t)tiles.size() - A.t_nf;
    A.t_dec = (int64_t)tiles.size();
    for (size_t u = 0; u < P.units.size(); ++u)
      for (int64_t t = P.units[u].d0; t < P.units[u].d1; t += FPT) push((int64_t)u, t, std::min(P.units[u].d1, t + FPT));
    A.n_dec = (int64_t)tiles.size() - A.t_dec;
    A.t_iir = (int64_t)tiles.size();
    if (!c.stationary)
      for (size_t u = 0; u < P.units.size(); ++u)
        if (P.units[u].r1 > P.units[u].r0)
          for (int f = 0; f < c.F; f += 64) push((int64_t)u, f, f + 64);
    A.n_iir = (int64_t)tiles.size() - A.t_iir;
    A.t_fs = (int64_t)tiles.size();
    for (size_t u = 0; u < P.units.size(); ++u)
      for (int64_t r = P.units[u].r0; r < P.units[u].r1; r += RPT) push((int64_t)u, r, std::min(P.units[u].r1, r + RPT));
    A.n_fs = (int64_t)tiles.size() - A.t_fs;
    A.t_ap = (int64_t)tiles.size();
    for (size_t u = 0; u < P.units.size(); ++u)
      for (int64_t t = P.units[u].l0; t < P.units[u].l1; t += FPT) push((int64_t)u, t, std::min(P.units[u].l1, t + FPT));
    A.n_ap = (int64_t)tiles.size() - A.t_ap;
    A.t_ola = (int64_t)tiles.size();
    for (size_t u = 0; u < P.units.size(); ++u)
      for (int64_t p = P.units[u].k0; p < P.units[u].k1; p += 256) push((int64_t)u, p, std::min(P.units[u].k1, p + 256));
    A.n_ola = (int64_t)tiles.size() - A.t_ola;
    const int64_t nu = (int64_t)P.units.size(), nn = (int64_t)noises.size(), ntl = (int64_t)tiles.size();
    if (nu != z.nu || nn != z.nn || noise_rows != z.noise_rows || ntl != z.ntiles || P.drows != z.drows ||
        P.frows != z.frows || P.mrows != z.mrows || P.sframes != z.sframes) {
      *err = "sg_process_clips: internal error: sub-batch tables disagree with their size estimate";
      return SG_E_STATE;
    }
    Layout L = layout(c, nu, nn, noise_rows, P.drows, P.frows, P.mrows, P.sframes, ntl);
    if (S->ws_bytes < L.total) {
      if (S->ws) { (void)hipStreamSynchronize(st); (void)hipFree(S->ws); S->ws = nullptr; S->ws_bytes = 0; }
      if (hipMalloc(&S->ws, L.total) != hipSuccess) {
        S->ws = nullptr;
        char b[160];
        snprintf(b, sizeof b, "sg_process_clips: workspace allocation of %zu bytes failed", L.total);
        *err = b;
        return SG_E_NOMEM;
      }
      S->ws_bytes = L.total;
    }
    char* w = (char*)S->ws;
    // the three tables in one host buffer, one copy
    std::vector<char> host((size_t)nu * sizeof(RgUnit) + (size_t)nn * sizeof(RgNoise) + (size_t)ntl * sizeof(RgTile));
    size_t o = 0;
    if (nu) memcpy(host.data() + o, P.units.data(), nu * sizeof(RgUnit));
    o += nu * sizeof(RgUnit);
    if (nn) memcpy(host.data() + o, noises.data(), nn * sizeof(RgNoise));
    o += nn * sizeof(RgNoise);
    if (ntl) memcpy(host.data() + o, tiles.data(), ntl * sizeof(RgTile));
    if (!host.empty() && hipMemcpyAsync(w + L.tabs, host.data(), host.size(), hipMemcpyHostToDevice, st) != hipSuccess) {
      *err = "sg_process_clips: table upload failed";
      return SG_E_HIP;
    }
    if (c.stationary && nu && hipMemsetAsync(w + L.pmax, 0, (size_t)nu * c.FS * 8, st) != hipSuccess) {
      *err = "sg_process_clips: hipMemsetAsync failed";
      return SG_E_HIP;
    }
    A.x = x_dev; A.in_dtype = in_dtype; A.xn = noise_dev; A.noise_dtype = noise_dtype;
    A.out = out_dev; A.out_dtype = out_dtype;
    A.units = (const RgUnit*)(w + L.tabs);
    A.noises = (const RgNoise*)(w + L.tabs + nu * sizeof(RgUnit));
    A.tiles = (const RgTile*)(w + L.tabs + nu * sizeof(RgUnit) + nn * sizeof(RgNoise));
    A.tw = (const cx<double>*)c.tw64; A.wfull = c.wfull64;
    A.Pn = (double*)(w + L.Pn); A.T2n = (double*)(w + L.T2n); A.thr_all = S->thr;
    A.pmax = (unsigned long long*)(w + L.pmax); A.bits = (unsigned long long*)(w + L.bits);
    A.mag = (float*)(w + L.mag); A.fw = (float*)(w + L.fw); A.sig = (float*)(w + L.sig); A.R = (float*)(w + L.R);
    A.seg = (float*)(w + L.seg);
    A.n = c.n; A.W = c.W; A.H = c.H; A.F = c.F; A.FS = c.FS; A.padL = c.padL; A.wpr = wpr;
    A.mag_scale = c.mag_scale; A.top_db = c.top_db; A.n_std = c.n_std; A.prop = c.prop; A.iir_b = c.iir_b;
    A.nthresh = c.nthresh; A.slope = c.slope; A.ddof = c.ddof; A.nf = c.nf; A.nt = c.nt; A.stationary = c.stationary;
    A.ktot = (double)((int64_t)(c.nf + 1) * (c.nf + 1) * (int64_t)(c.nt + 1) * (c.nt + 1));

    auto grid = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, n)); };
    hipError_t e = hipSuccess;
    if (c.stationary) {
      { Prof pr(c, SG_STAGE_RG_NOISE_POWER, st); e = launch_fft(c, A, 0, A.n_np, st); }
      if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_NOISE_FINAL, st); hipLaunchKernelGGL(k_rg_noise_final, grid(A.n_nf), dim3(64), 0, st, A); e = hipGetLastError(); }
    }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_DECIDE, st); e = launch_fft(c, A, 1, A.n_dec, st); }
    if (e == hipSuccess && !c.stationary) { Prof pr(c, SG_STAGE_RG_IIR, st); hipLaunchKernelGGL(k_rg_iir, grid(A.n_iir), dim3(64), 0, st, A); e = hipGetLastError(); }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_FSMOOTH, st); hipLaunchKernelGGL(k_rg_fsmooth, grid(A.n_fs), dim3(256), 0, st, A); e = hipGetLastError(); }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_APPLY, st); e = launch_fft(c, A, 2, A.n_ap, st); }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_OLA, st); hipLaunchKernelGGL(k_rg_ola, grid(A.n_ola), dim3(256), 0, st, A); e = hipGetLastError(); }
    if (e != hipSuccess) {
      *err = std::string("sg_process_clips: launch failed: ") + hipGetErrorString(e);
      return SG_E_HIP;
    }
    ++S->last_batches;
    // the table buffer is pageable host memory: hipMemcpyAsync has staged it before returning, so it may go
    i0 = i1;
  }
  return SG_OK;
}
}  // namespace sg
