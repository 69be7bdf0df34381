// Padded batches of different-length rows (sg_process_rows): tables, kernels and the host side.  See rows.hpp and
// DESIGN section 12.
//
// Variant T throughout (torch.stft(center=True, pad_mode="constant"): frame t is centred on sample t H; the window is
// embedded in an n_fft frame; torch.istft's trimming and envelope).  Row i owns T_i = 1 + len_i / H frames; samples at
// or beyond len_i read as 0 and are never loaded.  The structure is ragged.hip's: every kernel reads a tile table
// (tile = {row or noise row, first, end} -- frames for the transforms and the frequency smoothing, bands for the
// statistics and the moving mean, positions for the overlap-add); one wavefront per workgroup for the transforms up to
// N = 512 (wave-private LDS buffer, fft_wave.hpp SY = 1), a 256-thread team from N = 1024 on; nothing waits on another
// workgroup, and the only cross-tile reduction is exact (band maxima as integer atomics on the bit patterns of
// non-negative doubles), so a row's result does not depend on the other rows, their order or the padding.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fft_wave.hpp"
#include "geom.hpp"
#include "thresh.hpp"
#include "rows.hpp"
#include "../../include/mi355gate_debug.h"

namespace sg {

// ---- tables ------------------------------------------------------------------------------------------------------
struct RwRow {
  int64_t x_off;       // element of the source (x; backward: grad_out) holding sample 0 of the row
  int64_t len;         // readable samples (forward: lengths[i]; backward: H * (lengths[i] / H))
  int64_t T;           // frames: 1 + lengths[i] / H
  int64_t Lout;        // positions that receive a value (forward: H * (lengths[i] / H); backward: lengths[i])
  int64_t full;        // positions written, [Lout, full) with zeros (forward: H * (L / H); backward: L)
  int64_t out_off;     // element of out receiving position 0
  int64_t frow;        // first row of this row's frames in the bits / magnitude / mask / segment fields
  int64_t mask_off;    // element of the caller's mask holding frame 0, band 0
  int32_t noise;       // local noise index (stationary)
  int32_t pad_;
};
struct RwNoise {
  int64_t off, len, T; // element of sample 0, readable samples, frames
  int64_t prow;        // first row in the noise power field
  int32_t in_x, pad_;  // 1: the row's own samples (xn = None)
};
struct RwTile {
  int32_t idx, pad_;
  int64_t a, b;
};

struct RwArgs {
  const void* x; int in_dtype;
  const void* xn; int noise_dtype;
  void* out; int out_dtype;
  const RwRow* rows;
  const RwNoise* noises;
  const RwTile* tiles;           // all tile lists, back to back
  int64_t t_np, n_np;            // noise power tiles (noise row, frames)
  int64_t t_nf, n_nf;            // noise final tiles (noise row, band block)
  int64_t t_dec, n_dec;          // frame tiles (row, frames)
  int64_t t_box, n_box;          // moving-mean tiles (row, band block)
  int64_t t_fs, n_fs;            // frequency smoothing tiles (row, frames)
  int64_t t_ap, n_ap;            // frame tiles of the apply stage
  int64_t t_ola, n_ola;          // output tiles (row, positions)
  const cx<double>* tw;
  const double* wfull;
  double* Pn;                    // [noise rows][FS] float64 noise power
  double* T2n;                   // [local noise][FS] compare constant from the threshold alone
  double* thr;                   // [local noise][FS] thresholds (dB)
  unsigned long long* pmax;      // [rows][FS] band maxima of the row's power (bit patterns)
  unsigned long long* bits;      // [frame rows][wpr]
  float* mag;                    // [frame rows][FS] (non-stationary)
  float* sig;                    // [frame rows][FS] (non-stationary raw mask)
  float* R;                      // [frame rows][FS] frequency-smoothed mask
  float* seg;                    // [frame rows][n]
  float* mask_out;               // forward: nullptr or the caller's float[B][T][FS]
  const float* mask_in;          // backward: the mask of the forward call
  int n, W, H, F, FS, padL, wpr;
  double mag_scale, top_db, n_std, prop, nthresh, slope;
  int ddof, nf, nt, stationary, kbox, bwd;
  double ktot;
};

// sigmoid(((A - S) / S - thresh) * slope) as kernels.hpp sigmoid_ratio computes it (that header holds non-template kernels)
__device__ __forceinline__ float rw_sigmoid_ratio(double av, double s, float nthresh, float slope) {
  const float ratio = (float)(av - s) / (float)s;
  return 1.0f / (1.0f + __expf(-(ratio - nthresh) * slope));
}

__device__ __forceinline__ double rw_nan_if_nonfinite(double P) { return (P <= 1.79769313486231570e308) ? P : (double)NAN; }

// threads per frame, as ragged.hip: one wavefront up to N = 512, the 256-thread workgroup from N = 1024 on
template <int N>
constexpr int rw_nt() { return N <= 512 ? 64 : 256; }
template <int N>
constexpr int rw_sy() { return rw_nt<N>() <= 64 ? 1 : rw_nt<N>(); }

// sum of w^2 over the row's OWN frames that cover output position p (torch.istft's envelope for a row of T frames)
__device__ __forceinline__ double rw_envelope(const RwArgs& A, int64_t T, int64_t p) {
  const int64_t e = p + A.padL;
  int64_t t_hi = e / A.H;
  if (t_hi > T - 1) t_hi = T - 1;
  int64_t t_lo = (e - A.n + A.H) / A.H;
  if (e - A.n + 1 <= 0) t_lo = 0;
  double norm = 0.0;
  for (int64_t t = t_lo; t <= t_hi; ++t) {
    const double w = A.wfull[(int)(e - t * A.H)];
    norm += w * w;
  }
  return norm;
}

// sample g of a source of `len` readable samples starting at element off: 0 outside [0, len), never loaded there.
// Backward: the source is grad_out divided by the row's envelope.
__device__ __forceinline__ double rw_sample(const RwArgs& A, const void* src, int dt, int64_t off, int64_t len, int64_t T,
                                            int64_t g) {
  if (g < 0 || g >= len) return 0.0;
  double v = load_sample(src, dt, off + g);
  if (A.bwd) {
    const double norm = rw_envelope(A, T, g);
    v = norm > 1e-10 ? v / norm : v;
  }
  return v;
}

// window * frame t (samples [t H - padL, t H - padL + n)) into the team's buffer, forward transform, in place
template <int N>
__device__ __forceinline__ void rw_frame_fft(const RwArgs& A, const void* src, int dt, int64_t off, int64_t len, int64_t T,
                                             int64_t t, cx<double>* buf, const cx<double>* tw, int lane) {
  constexpr int NT = rw_nt<N>(), SY = rw_sy<N>();
  const int64_t s0 = t * A.H - A.padL;
  for (int j = lane; j < N; j += NT) {
    const double v0 = rw_sample(A, src, dt, off, len, T, s0 + 2 * j);
    const double v1 = rw_sample(A, src, dt, off, len, T, s0 + 2 * j + 1);
    buf[lp<double>(j)] = {v0 * A.wfull[2 * j], v1 * A.wfull[2 * j + 1]};
  }
  team_sync<SY>();
  wave_fft<double, N, false, NT, SY>(buf, tw, lane);
}

// bin k (0..N) of the real transform held packed in buf
template <int N>
__device__ __forceinline__ cx<double> rw_bin(const cx<double>* buf, const cx<double>* tw, int k) {
  cx<double> a = buf[lp<double>(k == N ? 0 : k)];
  cx<double> b = buf[lp<double>((k == 0 || k == N) ? 0 : N - k)];
  return rfft_bin(a, b, tw[k == N ? 0 : k], k, N);
}

template <int N>
__device__ __forceinline__ void rw_stage(cx<double>* tw, const RwArgs& A) {
  stage_twiddles<rw_nt<N>(), N>(tw, A.tw, (int)threadIdx.x);
  __syncthreads();
}

// ---- stationary: noise statistics ----------------------------------------------------------------------------------
// power of every frame of every noise row (xn's rows, or the rows themselves when xn is None)
template <int N>
__global__ __launch_bounds__(rw_nt<N>()) void k_rw_noise_power(RwArgs A) {
  constexpr int NT = rw_nt<N>(), SY = rw_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_np) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const RwTile tl = A.tiles[A.t_np + blockIdx.x];
  const RwNoise S = A.noises[tl.idx];
  const void* src = S.in_x ? A.x : A.xn;
  const int dt = S.in_x ? A.in_dtype : A.noise_dtype;
  rw_stage<N>(tw, A);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rw_frame_fft<N>(A, src, dt, S.off, S.len, S.T, t, buf, tw, lane);
    double* row = A.Pn + (S.prow + t) * A.FS;
    for (int k = lane; k <= N; k += NT) {
      const cx<double> X = rw_bin<N>(buf, tw, k);
      row[k] = rw_nan_if_nonfinite(X.x * X.x + X.y * X.y);
    }
    team_sync<SY>();
  }
}

// one thread per (noise row, band): maximum, moments of the floored dB relative to it (k_row_decide's summation
// structure: d = max(dB - max_dB, -top_db), s1 = sum d, s2 = sum d^2, serial over the noise row's own frames),
// threshold, and the compare constant of the threshold alone (the floor of the gated row is a per-(row, band)
// override, k_rw_fsmooth)
__global__ __launch_bounds__(64) void k_rw_noise_final(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_nf) return;
  const RwTile tl = A.tiles[A.t_nf + blockIdx.x];
  const int f = (int)tl.a + (int)threadIdx.x;
  if (f >= A.F) return;
  const RwNoise S = A.noises[tl.idx];
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
  A.thr[(int64_t)tl.idx * A.FS + f] = th;
}

// ---- per frame: decision bits + band maxima (stationary) or magnitudes (non-stationary) ----------------------------
template <int N>
__global__ __launch_bounds__(rw_nt<N>()) void k_rw_decide(RwArgs A) {
  constexpr int NT = rw_nt<N>(), SY = rw_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const RwTile tl = A.tiles[A.t_dec + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  rw_stage<N>(tw, A);
  constexpr int M = N / NT + 1;
  double vmax[M];
#pragma unroll
  for (int m = 0; m < M; ++m) vmax[m] = 0.0;
  const double* T2 = A.T2n + (int64_t)U.noise * A.FS;
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rw_frame_fft<N>(A, A.x, A.in_dtype, U.x_off, U.len, U.T, t, buf, tw, lane);
    const int64_t row = U.frow + t;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      double P = 0.0;
      if (k <= N) {
        const cx<double> X = rw_bin<N>(buf, tw, k);
        P = rw_nan_if_nonfinite(X.x * X.x + X.y * X.y);
      }
      if (A.stationary) {
        vmax[m] = nanmax(vmax[m], P);
        const unsigned long long word = __ballot(k <= N && P > T2[k <= N ? k : 0]);
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

// ---- non-stationary: conv1d(|X|, ones(k), padding="same") / k over the row's OWN frames + temperature sigmoid -------
// one thread per (row, band).  torch places an even-length kernel with (k - 1) / 2 zeros on the left: the mean at frame
// t reads frames [t - (k - 1) / 2, t - (k - 1) / 2 + k), those outside [0, T_i) as 0.  Every window is summed afresh,
// ascending, in float64 (no sliding difference: a window of silence after loud frames sums to exactly 0, and 0 / 0 is
// the reference's NaN).
__global__ __launch_bounds__(64) void k_rw_box(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_box) return;
  const RwTile tl = A.tiles[A.t_box + blockIdx.x];
  const int f = (int)tl.a + (int)threadIdx.x;
  if (f >= A.F) return;
  const RwRow U = A.rows[tl.idx];
  const float* col = A.mag + U.frow * A.FS + f;
  float* out = A.sig + U.frow * A.FS + f;
  const int left = (A.kbox - 1) / 2;
  for (int64_t t = 0; t < U.T; ++t) {
    const int64_t ja = t - left < 0 ? 0 : t - left;
    const int64_t jb = t - left + A.kbox > U.T ? U.T : t - left + A.kbox;
    double s = 0.0;
    for (int64_t j = ja; j < jb; ++j) s += (double)col[j * A.FS];
    s = s / (double)A.kbox;
    out[t * A.FS] = rw_sigmoid_ratio((double)col[t * A.FS], s, (float)A.nthresh, (float)A.slope);
  }
}

// ---- mask smoothing along frequency: R[row][f] = sum_df (nf + 1 - |df|) raw[row][f + df] ----------------------------
// Stationary raw mask: the decision bit, with the -top_db floor applied per (row, band) from the row's band maximum
// (k_t2_rows): floor above the threshold -> every cell of the band passes; NaN maximum or threshold -> none does.
__global__ __launch_bounds__(256) void k_rw_fsmooth(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_fs) return;
  __shared__ unsigned char mode[2112];   // per band: 0 = decision bits, 1 = all pass, 2 = none passes (F <= 2049)
  const RwTile tl = A.tiles[A.t_fs + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  if (A.stationary) {
    for (int f = threadIdx.x; f < A.F; f += blockDim.x) {
      const double th = A.thr[(int64_t)U.noise * A.FS + f];
      const double t2 = A.T2n[(int64_t)U.noise * A.FS + f];   // < 0: 20 log10(eps) > thresh
      const double pm = __longlong_as_double((long long)A.pmax[(int64_t)tl.idx * A.FS + f]);
      const double fl = cell_db(pm, A.mag_scale) - A.top_db;
      mode[f] = (th != th || fl != fl) ? 2 : ((fl > th || t2 < 0.0) ? 1 : 0);
    }
  }
  __syncthreads();
  const int nf = A.nf;
  for (int64_t r = tl.a; r < tl.b; ++r) {
    const unsigned long long* brow = A.bits + (U.frow + r) * A.wpr;
    const float* srow = A.sig + (U.frow + r) * A.FS;
    float* out = A.R + (U.frow + r) * A.FS;
    for (int f = threadIdx.x; f < A.F; f += blockDim.x) {
      float acc = 0.f;
      for (int df = -nf; df <= nf; ++df) {
        const int g = f + df;
        if (g < 0 || g >= A.F) continue;
        float v;
        if (A.stationary) {
          const unsigned char md = mode[g];
          v = md == 1 ? 1.f : (md == 2 ? 0.f : (float)((brow[g >> 6] >> (g & 63)) & 1ull));
        } else {
          v = srow[g];
        }
        acc += (float)(nf + 1 - (df < 0 ? -df : df)) * v;
      }
      out[f] = acc;
    }
  }
}

// ---- every frame: time smoothing within [0, T_i), masked multiply, inverse transform, synthesis window ----------------
// Forward: mask = (p K + (1 - p) E) / ktot with E the triangle's weight inside the row's own [0, T_i) x [0, F) field
// (torchgate.py:241-249: prop_decrease first, then the zero-padded smoothing -- the value outside the field is 0, not
// 1 - p).  Backward: the mask of the forward call, the source grad_out / envelope (rw_sample).
template <int N>
__global__ __launch_bounds__(rw_nt<N>()) void k_rw_apply(RwArgs A) {
  constexpr int NT = rw_nt<N>(), SY = rw_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const RwTile tl = A.tiles[A.t_ap + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  rw_stage<N>(tw, A);
  const int nt = A.nt;
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rw_frame_fft<N>(A, A.x, A.in_dtype, U.x_off, U.len, U.T, t, buf, tw, lane);
    const int64_t ta = t - nt < 0 ? 0 : t - nt, tb = t + nt >= U.T ? U.T - 1 : t + nt;
    const double Et = (double)tri_valid(nt, t, U.T);
    const int64_t mrow = U.mask_off + t * A.FS;
    auto mask_at = [&](int k) -> double {
      if (A.bwd) return (double)A.mask_in[mrow + k];
      double K = 0.0;
      for (int64_t q = ta; q <= tb; ++q) {
        const int64_t d = q - t;
        K += (double)(nt + 1 - (d < 0 ? -d : d)) * (double)A.R[(U.frow + q) * A.FS + k];
      }
      const double m = (A.prop * K + (1.0 - A.prop) * Et * (double)tri_valid(A.nf, k, A.F)) / A.ktot;
      if (A.mask_out) A.mask_out[mrow + k] = (float)m;
      return m;
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
        const double mk = mask_at(k), mn = (k != N - k) ? mask_at(N - k) : mk;
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
    float2* srow = reinterpret_cast<float2*>(A.seg + (U.frow + t) * (int64_t)A.n);
    const double inv = 1.0 / (double)N;
    for (int j = lane; j < N; j += NT) {
      const cx<double> z = buf[lp<double>(j)];
      srow[j] = make_float2((float)(z.x * A.wfull[2 * j] * inv), (float)(z.y * A.wfull[2 * j + 1] * inv));
    }
    team_sync<SY>();
  }
}

// ---- overlap-add over the row's own frames.  Forward: out = sum seg / envelope on [0, Lout_i); backward: the plain
// sum (the adjoint of the framing) on [0, len_i).  Positions up to `full` are the zero tail. ----------------------------
__global__ __launch_bounds__(256) void k_rw_ola(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_ola) return;
  const RwTile tl = A.tiles[A.t_ola + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
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
      acc += (double)A.seg[(U.frow + t) * (int64_t)A.n + m];
      norm += A.wfull[m] * A.wfull[m];
    }
    val = (!A.bwd && norm > 1e-10) ? acc / norm : acc;
  }
  if (A.out_dtype == 1) ((double*)A.out)[U.out_off + p] = val;
  else store_sample(A.out, A.out_dtype, U.out_off + p, (float)val);
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct RwState {
  void* ws = nullptr;
  size_t ws_bytes = 0;
  int64_t last_batches = 0;
};

void rw_free(RwState* s) {
  if (!s) return;
  if (s->ws) (void)hipFree(s->ws);
  delete s;
}

int64_t rw_last_batches(const RwState* s) { return s ? s->last_batches : 0; }

namespace {
constexpr int FPT = 8;     // frames per transform tile
constexpr int RPT = 16;    // frames per smoothing tile

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

struct Layout {
  size_t tabs, Pn, T2n, thr, pmax, bits, mag, sig, R, seg, total;
};
// counts of a sub-batch: rows, noise rows, noise frames, frames, tiles
struct Sizer {
  int64_t nu = 0, nn = 0, noise_rows = 0, frows = 0, ntiles = 0;
  void add_noise(const RgCtx& c, int64_t T) {
    ++nn;
    noise_rows += T;
    ntiles += cdiv(T, FPT) + cdiv(c.F, 64);
  }
  // T frames, `full` written positions; backward: apply and overlap-add tiles only
  void add_row(const RgCtx& c, int64_t T, int64_t full, bool bwd) {
    ++nu;
    frows += T;
    ntiles += cdiv(T, FPT) + cdiv(full, 256);
    if (!bwd) ntiles += cdiv(T, FPT) + cdiv(T, RPT) + (c.stationary ? 0 : cdiv(c.F, 64));
  }
  Layout layout(const RgCtx& c, bool bwd) const {
    Layout L{};
    const int wpr = (c.F + 63) / 64;
    const bool st = c.stationary && !bwd, ns = !c.stationary && !bwd;
    size_t o = 0;
    auto take = [&](size_t b) { size_t r = o; o += al(b); return r; };
    L.tabs = take((size_t)nu * sizeof(RwRow) + (size_t)nn * sizeof(RwNoise) + (size_t)ntiles * sizeof(RwTile));
    L.Pn = take((size_t)noise_rows * c.FS * 8);
    L.T2n = take((size_t)nn * c.FS * 8);
    L.thr = take((size_t)nn * c.FS * 8);
    L.pmax = take(st ? (size_t)nu * c.FS * 8 : 0);
    L.bits = take(st ? (size_t)frows * wpr * 8 : 0);
    L.mag = take(ns ? (size_t)frows * c.FS * 4 : 0);
    L.sig = take(ns ? (size_t)frows * c.FS * 4 : 0);
    L.R = take(bwd ? 0 : (size_t)frows * c.FS * 4);
    L.seg = take((size_t)frows * c.n * 4);
    L.total = o;
    return L;
  }
};

template <int N>
hipError_t launch_fft_kernels(const RwArgs& A, int which, unsigned grid, hipStream_t st) {
  const size_t lds = (size_t)(N + lpn<double>(N)) * sizeof(cx<double>);
  const void* k = which == 0 ? reinterpret_cast<const void*>(k_rw_noise_power<N>)
                : which == 1 ? reinterpret_cast<const void*>(k_rw_decide<N>)
                             : reinterpret_cast<const void*>(k_rw_apply<N>);
  if (lds > 65536) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const dim3 blk(rw_nt<N>());
  if (which == 0) hipLaunchKernelGGL(k_rw_noise_power<N>, dim3(grid), blk, lds, st, A);
  else if (which == 1) hipLaunchKernelGGL(k_rw_decide<N>, dim3(grid), blk, lds, st, A);
  else hipLaunchKernelGGL(k_rw_apply<N>, dim3(grid), blk, lds, st, A);
  return hipGetLastError();
}

hipError_t launch_fft(const RgCtx& c, const RwArgs& A, int which, int64_t ntiles, hipStream_t st) {
  const unsigned grid = (unsigned)std::max<int64_t>(1, ntiles);
  switch (c.N) {
    case 128: return launch_fft_kernels<128>(A, which, grid, st);
    case 256: return launch_fft_kernels<256>(A, which, grid, st);
    case 512: return launch_fft_kernels<512>(A, which, grid, st);
    case 1024: return launch_fft_kernels<1024>(A, which, grid, st);
    case 2048: return launch_fft_kernels<2048>(A, which, grid, st);
  }
  return hipErrorInvalidValue;
}

struct Prof {
  const RgCtx& c;
  void* tok;
  Prof(const RgCtx& c_, int stage, hipStream_t st) : c(c_), tok(c_.prof_begin ? c_.prof_begin(c_.hook_ctx, stage, st) : nullptr) {}
  ~Prof() { if (c.prof_end) c.prof_end(tok); }
};

bool geom_ok(const RgCtx& c, const char* who, std::string* err) {
  if ((c.N != 128 && c.N != 256 && c.N != 512 && c.N != 1024 && c.N != 2048) || c.n != 2 * c.N || c.padL != c.N) {
    *err = std::string(who) + ": n_fft must be a power of two from 256 to 4096";
    return false;
  }
  return true;
}

int check_lengths(const RgCtx& c, const char* who, const char* what, const int64_t* lengths, int64_t B, int64_t L,
                  std::string* err) {
  for (int64_t i = 0; lengths && i < B; ++i) {
    if (lengths[i] < 2 * (int64_t)c.W || lengths[i] > L) {
      char b[200];
      snprintf(b, sizeof b, "%s: %s[%lld] = %lld must lie in [%d, %lld] (2 * win_length .. row length)", who, what,
               (long long)i, (long long)lengths[i], 2 * c.W, (long long)L);
      *err = b;
      return SG_E_INVALID;
    }
  }
  return SG_OK;
}

// one call of either direction: rows [0, B) packed greedily into sub-batches under the budget
struct Call {
  bool bwd;
  const void* x; int dtype; int64_t B, L, x_stride; const int64_t* lengths;
  const void* xn; int64_t Bn, Ln, xn_stride; const int64_t* xn_lengths;
  void* out; int out_dtype; int64_t out_stride;
  float* mask_out; const float* mask_in;
};

int run(RwState** sp, const RgCtx& c, int kbox, const Call& q, int64_t max_ws, hipStream_t st, const char* who,
        std::string* err) {
  if (!*sp) *sp = new RwState();
  RwState* S = *sp;
  S->last_batches = 0;
  if (max_ws <= 0) max_ws = (int64_t)4 << 30;
  const int64_t H = c.H;
  const int64_t Tfull = 1 + q.L / H, Lq = H * (q.L / H);
  const bool stat = c.stationary && !q.bwd;
  const int noise_mode = !stat ? 0 : (!q.xn ? 1 : (q.Bn == 1 ? 2 : 3));   // 1: the row itself, 2: one shared row, 3: per row
  auto len_of = [&](int64_t i) { return q.lengths ? q.lengths[i] : q.L; };
  auto nlen_of = [&](int64_t i) { return q.xn_lengths ? q.xn_lengths[i] : q.Ln; };
  if (q.mask_out && hipMemsetAsync(q.mask_out, 0, (size_t)q.B * Tfull * c.FS * 4, st) != hipSuccess) {
    *err = std::string(who) + ": hipMemsetAsync failed";
    return SG_E_HIP;
  }
  const int wpr = (c.F + 63) / 64;
  int64_t i0 = 0;
  while (i0 < q.B) {
    // rows in order, greedily, under the budget (a row that alone exceeds it is a sub-batch of its own)
    int64_t i1 = i0;
    Sizer z;
    if (noise_mode == 2) z.add_noise(c, 1 + nlen_of(0) / H);
    while (i1 < q.B) {
      Sizer zn = z;
      if (noise_mode == 1) zn.add_noise(c, 1 + len_of(i1) / H);
      if (noise_mode == 3) zn.add_noise(c, 1 + nlen_of(i1) / H);
      zn.add_row(c, 1 + len_of(i1) / H, q.bwd ? q.L : Lq, q.bwd);
      if (i1 > i0 && (int64_t)zn.layout(c, q.bwd).total > max_ws) break;
      if (zn.nu > INT32_MAX - 1) break;
      z = zn;
      ++i1;
    }
    std::vector<RwRow> rows;
    std::vector<RwNoise> noises;
    int64_t noise_rows = 0, frows = 0;
    auto push_noise = [&](int64_t off, int64_t len, int in_x) {
      RwNoise Nn{};
      Nn.off = off; Nn.len = len; Nn.T = 1 + len / H; Nn.prow = noise_rows; Nn.in_x = in_x;
      noise_rows += Nn.T;
      noises.push_back(Nn);
    };
    if (noise_mode == 2) push_noise(0, nlen_of(0), 0);
    for (int64_t i = i0; i < i1; ++i) {
      const int64_t len = len_of(i);
      RwRow U{};
      U.x_off = i * q.x_stride;
      U.T = 1 + len / H;
      U.len = q.bwd ? H * (len / H) : len;
      U.Lout = q.bwd ? len : H * (len / H);
      U.full = q.bwd ? q.L : Lq;
      U.out_off = i * q.out_stride;
      U.frow = frows; frows += U.T;
      U.mask_off = i * Tfull * c.FS;
      U.noise = 0;
      if (noise_mode == 1) { U.noise = (int32_t)noises.size(); push_noise(i * q.x_stride, len, 1); }
      if (noise_mode == 3) { U.noise = (int32_t)noises.size(); push_noise(i * q.xn_stride, nlen_of(i), 0); }
      rows.push_back(U);
    }
    // tile lists
    std::vector<RwTile> tiles;
    auto push = [&](int64_t idx, int64_t a, int64_t b) { tiles.push_back(RwTile{(int32_t)idx, 0, a, b}); };
    RwArgs A{};
    A.t_np = (int64_t)tiles.size();
    for (size_t k = 0; k < noises.size(); ++k)
      for (int64_t t = 0; t < noises[k].T; t += FPT) push((int64_t)k, t, std::min<int64_t>(noises[k].T, t + FPT));
    A.n_np = (int64_t)tiles.size() - A.t_np;
    A.t_nf = (int64_t)tiles.size();
    for (size_t k = 0; k < noises.size(); ++k)
      for (int f = 0; f < c.F; f += 64) push((int64_t)k, f, f + 64);
    A.n_nf = (int64_t)tiles.size() - A.t_nf;
    A.t_dec = (int64_t)tiles.size();
    if (!q.bwd)
      for (size_t u = 0; u < rows.size(); ++u)
        for (int64_t t = 0; t < rows[u].T; t += FPT) push((int64_t)u, t, std::min(rows[u].T, t + FPT));
    A.n_dec = (int64_t)tiles.size() - A.t_dec;
    A.t_box = (int64_t)tiles.size();
    if (!q.bwd && !c.stationary)
      for (size_t u = 0; u < rows.size(); ++u)
        for (int f = 0; f < c.F; f += 64) push((int64_t)u, f, f + 64);
    A.n_box = (int64_t)tiles.size() - A.t_box;
    A.t_fs = (int64_t)tiles.size();
    if (!q.bwd)
      for (size_t u = 0; u < rows.size(); ++u)
        for (int64_t r = 0; r < rows[u].T; r += RPT) push((int64_t)u, r, std::min(rows[u].T, r + RPT));
    A.n_fs = (int64_t)tiles.size() - A.t_fs;
    A.t_ap = (int64_t)tiles.size();
    for (size_t u = 0; u < rows.size(); ++u)
      for (int64_t t = 0; t < rows[u].T; t += FPT) push((int64_t)u, t, std::min(rows[u].T, t + FPT));
    A.n_ap = (int64_t)tiles.size() - A.t_ap;
    A.t_ola = (int64_t)tiles.size();
    for (size_t u = 0; u < rows.size(); ++u)
      for (int64_t p = 0; p < rows[u].full; p += 256) push((int64_t)u, p, std::min(rows[u].full, p + 256));
    A.n_ola = (int64_t)tiles.size() - A.t_ola;
    const int64_t nu = (int64_t)rows.size(), nn = (int64_t)noises.size(), ntl = (int64_t)tiles.size();
    if (nu != z.nu || nn != z.nn || noise_rows != z.noise_rows || frows != z.frows || ntl != z.ntiles) {
      *err = std::string(who) + ": internal error: sub-batch tables disagree with their size estimate";
      return SG_E_STATE;
    }
    const Layout Ly = z.layout(c, q.bwd);
    if (S->ws_bytes < Ly.total) {
      if (S->ws) { (void)hipStreamSynchronize(st); (void)hipFree(S->ws); S->ws = nullptr; S->ws_bytes = 0; }
      if (hipMalloc(&S->ws, Ly.total) != hipSuccess) {
        S->ws = nullptr;
        char b[160];
        snprintf(b, sizeof b, "%s: workspace allocation of %zu bytes failed", who, Ly.total);
        *err = b;
        return SG_E_NOMEM;
      }
      S->ws_bytes = Ly.total;
    }
    char* w = (char*)S->ws;
    // the three tables in one host buffer, one copy
    std::vector<char> host((size_t)nu * sizeof(RwRow) + (size_t)nn * sizeof(RwNoise) + (size_t)ntl * sizeof(RwTile));
    size_t o = 0;
    if (nu) memcpy(host.data() + o, rows.data(), nu * sizeof(RwRow));
    o += nu * sizeof(RwRow);
    if (nn) memcpy(host.data() + o, noises.data(), nn * sizeof(RwNoise));
    o += nn * sizeof(RwNoise);
    if (ntl) memcpy(host.data() + o, tiles.data(), ntl * sizeof(RwTile));
    if (!host.empty() && hipMemcpyAsync(w + Ly.tabs, host.data(), host.size(), hipMemcpyHostToDevice, st) != hipSuccess) {
      *err = std::string(who) + ": table upload failed";
      return SG_E_HIP;
    }
    if (stat && hipMemsetAsync(w + Ly.pmax, 0, (size_t)nu * c.FS * 8, st) != hipSuccess) {
      *err = std::string(who) + ": hipMemsetAsync failed";
      return SG_E_HIP;
    }
    A.x = q.x; A.in_dtype = q.dtype; A.xn = q.xn; A.noise_dtype = q.dtype;
    A.out = q.out; A.out_dtype = q.out_dtype;
    A.rows = (const RwRow*)(w + Ly.tabs);
    A.noises = (const RwNoise*)(w + Ly.tabs + nu * sizeof(RwRow));
    A.tiles = (const RwTile*)(w + Ly.tabs + nu * sizeof(RwRow) + nn * sizeof(RwNoise));
    A.tw = (const cx<double>*)c.tw64; A.wfull = c.wfull64;
    A.Pn = (double*)(w + Ly.Pn); A.T2n = (double*)(w + Ly.T2n); A.thr = (double*)(w + Ly.thr);
    A.pmax = (unsigned long long*)(w + Ly.pmax); A.bits = (unsigned long long*)(w + Ly.bits);
    A.mag = (float*)(w + Ly.mag); A.sig = (float*)(w + Ly.sig); A.R = (float*)(w + Ly.R); A.seg = (float*)(w + Ly.seg);
    A.mask_out = q.mask_out; A.mask_in = q.mask_in;
    A.n = c.n; A.W = c.W; A.H = c.H; A.F = c.F; A.FS = c.FS; A.padL = c.padL; A.wpr = wpr;
    A.mag_scale = c.mag_scale; A.top_db = c.top_db; A.n_std = c.n_std; A.prop = c.prop;
    A.nthresh = c.nthresh; A.slope = c.slope; A.ddof = c.ddof; A.nf = c.nf; A.nt = c.nt; A.stationary = c.stationary;
    A.kbox = kbox; A.bwd = q.bwd ? 1 : 0;
    A.ktot = (double)((int64_t)(c.nf + 1) * (c.nf + 1) * (int64_t)(c.nt + 1) * (c.nt + 1));

    auto grid = [](int64_t n) { return dim3((unsigned)std::max<int64_t>(1, n)); };
    hipError_t e = hipSuccess;
    if (stat) {
      { Prof pr(c, SG_STAGE_RG_NOISE_POWER, st); e = launch_fft(c, A, 0, A.n_np, st); }
      if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_NOISE_FINAL, st); hipLaunchKernelGGL(k_rw_noise_final, grid(A.n_nf), dim3(64), 0, st, A); e = hipGetLastError(); }
    }
    if (!q.bwd) {
      if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_DECIDE, st); e = launch_fft(c, A, 1, A.n_dec, st); }
      // (the stage table is pinned at 27 entries: the moving mean books under the slot of the clips path's recurrence)
      if (e == hipSuccess && !c.stationary) { Prof pr(c, SG_STAGE_RG_IIR, st); hipLaunchKernelGGL(k_rw_box, grid(A.n_box), dim3(64), 0, st, A); e = hipGetLastError(); }
      if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_FSMOOTH, st); hipLaunchKernelGGL(k_rw_fsmooth, grid(A.n_fs), dim3(256), 0, st, A); e = hipGetLastError(); }
    }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_APPLY, st); e = launch_fft(c, A, 2, A.n_ap, st); }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_OLA, st); hipLaunchKernelGGL(k_rw_ola, grid(A.n_ola), dim3(256), 0, st, A); e = hipGetLastError(); }
    if (e != hipSuccess) {
      *err = std::string(who) + ": launch failed: " + hipGetErrorString(e);
      return SG_E_HIP;
    }
    ++S->last_batches;
    // the table buffer is pageable host memory: hipMemcpyAsync has staged it before returning, so it may go
    i0 = i1;
  }
  return SG_OK;
}
}  // namespace

int rw_process(RwState** sp, const RgCtx& c, int kbox, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
               const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
               const int64_t* xn_lengths, void* out_dev, int out_dtype, int64_t out_stride, float* mask_out,
               int64_t max_ws, hipStream_t st, std::string* err) {
  const char* who = "sg_process_rows";
  if (!geom_ok(c, who, err)) return SG_E_UNSUPPORTED;
  int rc = check_lengths(c, who, "lengths", lengths, B, L, err);
  if (rc) return rc;
  const bool use_xn = xn_dev && c.stationary;
  if (use_xn && (rc = check_lengths(c, who, "xn_lengths", xn_lengths, Bn, Ln, err))) return rc;
  if (!c.stationary && kbox < 1) { *err = std::string(who) + ": n_movemean must be at least 1"; return SG_E_INVALID; }
  Call q{};
  q.bwd = false;
  q.x = x_dev; q.dtype = dtype; q.B = B; q.L = L; q.x_stride = x_stride; q.lengths = lengths;
  q.xn = use_xn ? xn_dev : nullptr; q.Bn = Bn; q.Ln = Ln; q.xn_stride = xn_stride; q.xn_lengths = use_xn ? xn_lengths : nullptr;
  q.out = out_dev; q.out_dtype = out_dtype; q.out_stride = out_stride;
  q.mask_out = mask_out; q.mask_in = nullptr;
  return run(sp, c, kbox, q, max_ws, st, who, err);
}

int rw_backward(RwState** sp, const RgCtx& c, const void* go_dev, int dtype, int64_t B, int64_t L, int64_t go_stride,
                const int64_t* lengths, const float* mask, void* gx_dev, int64_t gx_stride, int64_t max_ws,
                hipStream_t st, std::string* err) {
  const char* who = "sg_process_rows_backward";
  if (!geom_ok(c, who, err)) return SG_E_UNSUPPORTED;
  int rc = check_lengths(c, who, "lengths", lengths, B, L, err);
  if (rc) return rc;
  Call q{};
  q.bwd = true;
  q.x = go_dev; q.dtype = dtype; q.B = B; q.L = L; q.x_stride = go_stride; q.lengths = lengths;
  q.out = gx_dev; q.out_dtype = dtype; q.out_stride = gx_stride;
  q.mask_in = mask;
  return run(sp, c, 0, q, max_ws, st, who, err);
}
}  // namespace sg
