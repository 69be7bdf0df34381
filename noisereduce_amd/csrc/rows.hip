// Padded batches of different-length rows (sg_process_rows, sg_gate_spectrum_rows, sg_gate_features_rows): kernels and
// the host side.  See rows.hpp and DESIGN sections 12 and 14.  The row / noise / argument tables and the frame loader
// are rows_kernels.hpp's, shared with rows_feat.hip, which holds the two feature kernels (in this
// file they changed the code the compiler builds for the kernels below); run() launches them through rw_feat_launch.
//
// Variant T throughout (torch.stft(center=True, pad_mode="constant"): frame t is centred on sample t H; the window is
// embedded in an n_fft frame; torch.istft's trimming and envelope).  Row i owns T_i = 1 + len_i / H frames; samples at
// or beyond len_i read as 0 and are never loaded.  Every kernel reads a tile table (tile = {row or noise row, first,
// end} -- frames for the transforms and the frequency smoothing, bands for the statistics and the moving mean, positions
// for the overlap-add).  What a frame goes through is tile_core.hpp's, shared with ragged.hip and stream.hip; this file
// holds what only the rows have: the loader with the backward pass's envelope division, the moving mean, the mask that
// is returned to (forward) or taken from (backward) the caller.  Nothing waits on another workgroup, and the only
// cross-tile reduction is exact (band maxima as integer atomics on the bit patterns of non-negative doubles), so a row's
// result does not depend on the other rows, their order or the padding.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tile_core.hpp"
#include "rows.hpp"
#include "rows_kernels.hpp"
#include "../../include/mi355gate_debug.h"

namespace sg {

// ---- stationary: noise statistics ----------------------------------------------------------------------------------
// power of every frame of every noise row (xn's rows, or the rows themselves when xn is None)
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_rw_noise_power(RwArgs A) {
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_np) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_np + blockIdx.x];
  const RwNoise S = A.noises[tl.idx];
  const void* src = S.in_x ? A.x : A.xn;
  const int dt = S.in_x ? A.in_dtype : A.noise_dtype;
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rw_frame_fft<N>(A, src, dt, S.off, S.len, S.T, t, buf, tw, lane);
    double* row = A.Pn + (S.prow + t) * A.c.FS;
    for (int k = lane; k <= N; k += NT) row[k] = bin_power<N>(buf, tw, k);
    team_sync<SY>();
  }
}

// one thread per (noise row, band): the threshold over the noise row's own frames, and the compare constant of the
// threshold alone (the floor of the gated row is a per-(row, band) override, k_rw_fsmooth)
__global__ __launch_bounds__(64) void k_rw_noise_final(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_nf) return;
  const Tile tl = A.tiles[A.t_nf + blockIdx.x];
  const int f = (int)tl.a + (int)threadIdx.x;
  if (f >= A.c.F) return;
  const RwNoise S = A.noises[tl.idx];
  const double th = noise_band_threshold(A.c, A.Pn + S.prow * A.c.FS + f, S.T);
  A.T2n[(int64_t)tl.idx * A.c.FS + f] = thresh_to_t2(th, A.c.mag_scale);
  A.thr[(int64_t)tl.idx * A.c.FS + f] = th;
}

// ---- per frame: decision bits + band maxima (stationary) or magnitudes (non-stationary) ----------------------------
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_rw_decide(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_dec + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  double vmax[tile_bins<N>()];
#pragma unroll
  for (int m = 0; m < tile_bins<N>(); ++m) vmax[m] = 0.0;
  const double* T2 = A.T2n + (int64_t)U.noise * A.c.FS;
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rw_frame_fft<N>(A, A.x, A.in_dtype, U.x_off, U.len, U.T, t, buf, tw, lane);
    const int64_t row = U.frow + t;
    decide_frame<N>(A.c, buf, tw, lane, T2, A.bits + row * A.c.wpr, A.mag + row * A.c.FS, vmax);
    team_sync<tile_sy<N>()>();
  }
  if (A.c.stationary) merge_band_maxima<N>(A.pmax + (int64_t)tl.idx * A.c.FS, lane, vmax);
}

// ---- non-stationary: conv1d(|X|, ones(k), padding="same") / k over the row's OWN frames + temperature sigmoid -------
// one thread per (row, band).  torch places an even-length kernel with (k - 1) / 2 zeros on the left: the mean at frame
// t reads frames [t - (k - 1) / 2, t - (k - 1) / 2 + k), those outside [0, T_i) as 0.  Every window is summed afresh,
// ascending, in float64 (no sliding difference: a window of silence after loud frames sums to exactly 0, and 0 / 0 is
// the reference's NaN).
__global__ __launch_bounds__(64) void k_rw_box(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_box) return;
  const Tile tl = A.tiles[A.t_box + blockIdx.x];
  const int f = (int)tl.a + (int)threadIdx.x;
  if (f >= A.c.F) return;
  const int FS = A.c.FS;
  const RwRow U = A.rows[tl.idx];
  const float* col = A.mag + U.frow * FS + f;
  float* out = A.sig + U.frow * FS + f;
  const int left = (A.kbox - 1) / 2;
  for (int64_t t = 0; t < U.T; ++t) {
    const int64_t ja = t - left < 0 ? 0 : t - left;
    const int64_t jb = t - left + A.kbox > U.T ? U.T : t - left + A.kbox;
    double s = 0.0;
    for (int64_t j = ja; j < jb; ++j) s += (double)col[j * FS];
    s = s / (double)A.kbox;
    out[t * FS] = sigmoid_ratio((double)col[t * FS], s, (float)A.c.nthresh, (float)A.c.slope);
  }
}

// ---- mask smoothing along frequency (fsmooth_row) -------------------------------------------------------------------
// Stationary raw mask: the decision bit, with the -top_db floor applied per (row, band) from the row's band maximum
// (band_mode).
__global__ __launch_bounds__(256) void k_rw_fsmooth(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_fs) return;
  __shared__ unsigned char mode[2112];   // band_mode per band (F <= 2049)
  const Tile tl = A.tiles[A.t_fs + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  const int FS = A.c.FS;
  if (A.c.stationary) {
    for (int f = threadIdx.x; f < A.c.F; f += blockDim.x) {
      const double pm = __longlong_as_double((long long)A.pmax[(int64_t)tl.idx * FS + f]);
      mode[f] = band_mode(pm, A.thr[(int64_t)U.noise * FS + f], A.T2n[(int64_t)U.noise * FS + f], A.c.mag_scale, A.c.top_db);
    }
  }
  __syncthreads();
  for (int64_t r = tl.a; r < tl.b; ++r) {
    const unsigned long long* brow = A.bits + (U.frow + r) * A.c.wpr;
    const float* srow = A.sig + (U.frow + r) * FS;
    fsmooth_row(A.R + (U.frow + r) * FS, A.c.F, A.c.nf, [&](int g) -> float {
      if (!A.c.stationary) return srow[g];
      const unsigned char md = mode[g];
      return md == 1 ? 1.f : (md == 2 ? 0.f : bit_at(brow, g));
    });
  }
}

// ---- every frame: time smoothing within [0, T_i), masked multiply, inverse transform, synthesis window ----------------
// Forward: the stationary mask formula in both modes, over the row's own [0, T_i) x [0, F) field (torchgate.py:241-249:
// prop_decrease first, then the zero-padded smoothing).  Backward: the mask of the forward call, the source
// grad_out / envelope (rw_sample).
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_rw_apply(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_ap + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rw_frame_fft<N>(A, A.x, A.in_dtype, U.x_off, U.len, U.T, t, buf, tw, lane);
    const TimeTaps tp = time_taps(t, A.c.nt, U.T);
    const int64_t mrow = U.mask_off + t * A.c.FS;
    auto mask_at = [&](int k) -> double {
      if (A.bwd) return (double)A.mask_in[mrow + k];
      const double K = time_smooth(A.R, A.c.FS, [&](int64_t q) { return U.frow + q; }, tp, t, A.c.nt, k);
      const double m = mask_stationary(A.c, K, tp.Et, k);
      if (A.mask_out) A.mask_out[mrow + k] = (float)m;
      return m;
    };
    mask_and_invert<N>(buf, tw, lane, mask_at, A.c.wfull, A.seg + (U.frow + t) * (int64_t)A.c.n);
  }
}

// ---- the gated spectrogram of a padded batch (sg_gate_spectrum_rows): k_rw_apply's mask, the bins stored instead of
// inverted.  The tiles cover [0, T) of every row: frames at or beyond T_i store zeros and load nothing (no memset of the
// output).  out: [B][T][F] complex of out_dtype, row i's frame 0 at complex element out_off; consecutive lanes store
// consecutive bins.  The bins are multiplied by the mask AS RETURNED (rounded to float32), as sg_gate_spectrum does:
// k_rw_spec_bwd is then the adjoint of exactly this map, and a complex128 result is X * mask to float64 rounding.
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_rw_spec(RwArgs A) {
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_ap + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    const int64_t srow = U.out_off + t * A.c.F;
    if (t >= U.T) {
      for (int k = lane; k <= N; k += NT) {
        if (A.out_dtype == 1) ((double2*)A.out)[srow + k] = make_double2(0.0, 0.0);
        else ((float2*)A.out)[srow + k] = make_float2(0.f, 0.f);
      }
      continue;
    }
    rw_frame_fft<N>(A, A.x, A.in_dtype, U.x_off, U.len, U.T, t, buf, tw, lane);
    const TimeTaps tp = time_taps(t, A.c.nt, U.T);
    const int64_t mrow = U.mask_off + t * A.c.FS;
    for (int k = lane; k <= N; k += NT) {
      const double K = time_smooth(A.R, A.c.FS, [&](int64_t q) { return U.frow + q; }, tp, t, A.c.nt, k);
      const float m = (float)mask_stationary(A.c, K, tp.Et, k);
      if (A.mask_out) A.mask_out[mrow + k] = m;
      const cx<double> X = packed_bin<N>(buf, tw, k);
      if (A.out_dtype == 1) ((double2*)A.out)[srow + k] = make_double2(X.x * (double)m, X.y * (double)m);
      else ((float2*)A.out)[srow + k] = make_float2((float)(X.x * (double)m), (float)(X.y * (double)m));
    }
    team_sync<SY>();
  }
}

// ---- its adjoint with the mask fixed (sg_gate_spectrum_rows_backward): frame t < T_i of row i from grad [B][T][F]
// complex of in_dtype (frame 0 at complex element x_off) and the forward's mask -> window * un-normalised inverse of the
// merged mask .* grad into seg (mask_and_adjoint).  Frames at or beyond T_i are not in the tile list: never read.
// k_rw_ola's plain sum follows.
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_rw_spec_bwd(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_ap + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    const int64_t grow = U.x_off + t * A.c.F;
    const float* mrow = A.mask_in + U.mask_off + t * A.c.FS;
    auto grad_at = [&](int k) -> cx<double> {
      if (A.in_dtype == 1) { const double2 g = ((const double2*)A.x)[grow + k]; return {g.x, g.y}; }
      const float2 g = ((const float2*)A.x)[grow + k];
      return {(double)g.x, (double)g.y};
    };
    mask_and_adjoint<N>(buf, tw, lane, grad_at, [&](int k) -> double { return (double)mrow[k]; }, A.c.wfull,
                        A.seg + (U.frow + t) * (int64_t)A.c.n);
  }
}

// ---- overlap-add over the row's own frames.  Forward: out = sum seg / envelope on [0, Lout_i); backward (of the
// waveform and of the spectrogram alike): the plain sum (the adjoint of the framing) on [0, len_i).  Positions up to
// `full` are the zero tail. --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rw_ola(RwArgs A) {
  if ((int64_t)blockIdx.x >= A.n_ola) return;
  const Tile tl = A.tiles[A.t_ola + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  const int64_t p = tl.a + threadIdx.x;
  if (p >= tl.b) return;
  double val = 0.0;
  if (p < U.Lout) {
    double acc, norm;
    ola_sum(A.c, A.seg, [&](int64_t t) { return U.frow + t; }, p + A.c.padL, U.T, &acc, &norm);
    val = (!A.bwd && norm > 1e-10) ? acc / norm : acc;
  }
  if (A.out_dtype == 1) ((double*)A.out)[U.out_off + p] = val;
  else store_sample(A.out, A.out_dtype, U.out_off + p, (float)val);
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct RwState {
  host::DevBuf ws;
  int64_t last_batches = 0;
};

void rw_free(RwState* s) { delete s; }

int64_t rw_last_batches(const RwState* s) { return s ? s->last_batches : 0; }

namespace {
constexpr int FPT = 8;     // frames per transform tile
constexpr int RPT = 16;    // frames per smoothing tile

struct Layout {
  size_t tabs, Pn, T2n, thr, pmax, bits, mag, sig, R, seg, total;
};
// counts of a sub-batch: rows, noise rows, noise frames, frames, tiles
struct Sizer {
  int64_t nu = 0, nn = 0, noise_rows = 0, frows = 0, ntiles = 0;
  void add_noise(const RgCtx& c, int64_t T) {
    ++nn;
    noise_rows += T;
    ntiles += tile_cdiv(T, FPT) + tile_cdiv(c.F, 64);
  }
  // T frames, `full` written positions; backward: apply and overlap-add tiles only.  Tap: frames the apply stage's
  // tiles cover (the spectrum forward stores every frame of the padded row, and has no overlap-add: full = 0)
  void add_row(const RgCtx& c, int64_t T, int64_t full, bool bwd, int64_t Tap) {
    ++nu;
    frows += T;
    ntiles += tile_cdiv(Tap, FPT) + tile_cdiv(full, 256);
    if (!bwd) ntiles += tile_cdiv(T, FPT) + tile_cdiv(T, RPT) + (c.stationary ? 0 : tile_cdiv(c.F, 64));
  }
  // no_seg: the spectrum forward keeps no frame segments
  Layout layout(const RgCtx& c, bool bwd, bool no_seg) const {
    Layout L{};
    const int wpr = (c.F + 63) / 64;
    const bool st = c.stationary && !bwd, ns = !c.stationary && !bwd;
    size_t o = 0;
    auto take = [&](size_t b) { size_t r = o; o += align256(b); return r; };
    L.tabs = take((size_t)nu * sizeof(RwRow) + (size_t)nn * sizeof(RwNoise) + (size_t)ntiles * sizeof(Tile));
    L.Pn = take((size_t)noise_rows * c.FS * 8);
    L.T2n = take((size_t)nn * c.FS * 8);
    L.thr = take((size_t)nn * c.FS * 8);
    L.pmax = take(st ? (size_t)nu * c.FS * 8 : 0);
    L.bits = take(st ? (size_t)frows * wpr * 8 : 0);
    L.mag = take(ns ? (size_t)frows * c.FS * 4 : 0);
    L.sig = take(ns ? (size_t)frows * c.FS * 4 : 0);
    L.R = take(bwd ? 0 : (size_t)frows * c.FS * 4);
    L.seg = take(no_seg ? 0 : (size_t)frows * c.n * 4);
    L.total = o;
    return L;
  }
};

bool geom_ok(const RgCtx& c, const char* who, std::string* err) {
  if (!tile_geom_ok(c.N) || c.n != 2 * c.N || c.padL != c.N) {
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

// one call of either direction: rows [0, B) packed greedily into sub-batches under the budget.  spec: the gated
// spectrogram -- forward: out is [B][T][F] complex of out_dtype, out_stride = T * F; backward: x is the gradient in that
// layout, x_stride = T * F.  feat: the filterbank features -- forward: out is [B][T][M] of out_dtype, out_stride = T * M;
// backward: x is the samples again and Q.grad the gradient in that layout
struct Call {
  bool bwd, spec, feat;
  RwFeat Q;
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
  const bool spec_fwd = (q.spec || q.feat) && !q.bwd;   // a frame sink: no segments, no overlap-add, tiles over [0, T)
  const int noise_mode = !stat ? 0 : (!q.xn ? 1 : (q.Bn == 1 ? 2 : 3));   // 1: the row itself, 2: one shared row, 3: per row
  auto len_of = [&](int64_t i) { return q.lengths ? q.lengths[i] : q.L; };
  auto nlen_of = [&](int64_t i) { return q.xn_lengths ? q.xn_lengths[i] : q.Ln; };
  if (q.mask_out && hipMemsetAsync(q.mask_out, 0, (size_t)q.B * Tfull * c.FS * 4, st) != hipSuccess) {
    *err = std::string(who) + ": hipMemsetAsync failed";
    return SG_E_HIP;
  }
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
      zn.add_row(c, 1 + len_of(i1) / H, spec_fwd ? 0 : (q.bwd ? q.L : Lq), q.bwd, spec_fwd ? Tfull : 1 + len_of(i1) / H);
      if (i1 > i0 && (int64_t)zn.layout(c, q.bwd, spec_fwd).total > max_ws) break;
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
      U.len = (q.bwd && !q.feat) ? H * (len / H) : len;   // (the features' backward reads the samples, not grad_out)
      U.Lout = spec_fwd ? 0 : (q.bwd ? len : H * (len / H));
      U.full = spec_fwd ? 0 : (q.bwd ? q.L : Lq);
      U.out_off = i * q.out_stride;
      U.frow = frows; frows += U.T;
      U.mask_off = i * Tfull * c.FS;
      U.noise = 0;
      if (noise_mode == 1) { U.noise = (int32_t)noises.size(); push_noise(i * q.x_stride, len, 1); }
      if (noise_mode == 3) { U.noise = (int32_t)noises.size(); push_noise(i * q.xn_stride, nlen_of(i), 0); }
      rows.push_back(U);
    }
    // tile lists (backward: apply and overlap-add only)
    TileList tl;
    RwArgs A{};
    const int64_t nu = (int64_t)rows.size(), nn = (int64_t)noises.size(), nfwd = q.bwd ? 0 : nu;
    A.t_np = tl.begin_stage();
    for (int64_t k = 0; k < nn; ++k) tl.push_ranges(k, 0, noises[k].T, FPT);
    A.n_np = tl.count_since(A.t_np);
    A.t_nf = tl.begin_stage();
    for (int64_t k = 0; k < nn; ++k) tl.push_ranges(k, 0, c.F, 64, false);
    A.n_nf = tl.count_since(A.t_nf);
    A.t_dec = tl.begin_stage();
    for (int64_t u = 0; u < nfwd; ++u) tl.push_ranges(u, 0, rows[u].T, FPT);
    A.n_dec = tl.count_since(A.t_dec);
    A.t_box = tl.begin_stage();
    for (int64_t u = 0; u < nfwd && !c.stationary; ++u) tl.push_ranges(u, 0, c.F, 64, false);
    A.n_box = tl.count_since(A.t_box);
    A.t_fs = tl.begin_stage();
    for (int64_t u = 0; u < nfwd; ++u) tl.push_ranges(u, 0, rows[u].T, RPT);
    A.n_fs = tl.count_since(A.t_fs);
    A.t_ap = tl.begin_stage();
    for (int64_t u = 0; u < nu; ++u) tl.push_ranges(u, 0, spec_fwd ? Tfull : rows[u].T, FPT);
    A.n_ap = tl.count_since(A.t_ap);
    A.t_ola = tl.begin_stage();
    for (int64_t u = 0; u < nu; ++u) tl.push_ranges(u, 0, rows[u].full, 256);
    A.n_ola = tl.count_since(A.t_ola);
    const int64_t ntl = tl.size();
    if (nu != z.nu || nn != z.nn || noise_rows != z.noise_rows || frows != z.frows || ntl != z.ntiles) {
      *err = std::string(who) + ": internal error: sub-batch tables disagree with their size estimate";
      return SG_E_STATE;
    }
    const Layout Ly = z.layout(c, q.bwd, spec_fwd);
    int rc = grow_device_buffer(S->ws, Ly.total, st, who, "workspace", err);
    if (rc) return rc;
    char* w = S->ws.as<char>();
    const size_t ub = nu * sizeof(RwRow), nb = nn * sizeof(RwNoise), tb = ntl * sizeof(Tile);
    if (upload_tables(w + Ly.tabs, st, {{rows.data(), ub, ub}, {noises.data(), nb, nb}, {tl.tiles.data(), tb, tb}}) != hipSuccess) {
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
    A.noises = (const RwNoise*)(w + Ly.tabs + ub);
    A.tiles = (const Tile*)(w + Ly.tabs + ub + nb);
    A.Pn = (double*)(w + Ly.Pn); A.T2n = (double*)(w + Ly.T2n); A.thr = (double*)(w + Ly.thr);
    A.pmax = (unsigned long long*)(w + Ly.pmax); A.bits = (unsigned long long*)(w + Ly.bits);
    A.mag = (float*)(w + Ly.mag); A.sig = (float*)(w + Ly.sig); A.R = (float*)(w + Ly.R); A.seg = (float*)(w + Ly.seg);
    A.mask_out = q.mask_out; A.mask_in = q.mask_in;
    A.kbox = kbox; A.bwd = q.bwd ? 1 : 0;
    A.c = fill_consts(c);

    hipError_t e = hipSuccess;
    if (stat) {
      { Prof pr(c, SG_STAGE_RG_NOISE_POWER, st); e = dispatch_N(c.N, [&](auto n) { return launch_tile_kernel<n()>(k_rw_noise_power<n()>, A.n_np, st, A); }); }
      if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_NOISE_FINAL, st); e = launch_flat_kernel(k_rw_noise_final, A.n_nf, 64, st, A); }
    }
    if (!q.bwd) {
      if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_DECIDE, st); e = dispatch_N(c.N, [&](auto n) { return launch_tile_kernel<n()>(k_rw_decide<n()>, A.n_dec, st, A); }); }
      // (the stage table is pinned at 27 entries: the moving mean books under the slot of the clips path's recurrence)
      if (e == hipSuccess && !c.stationary) { Prof pr(c, SG_STAGE_RG_IIR, st); e = launch_flat_kernel(k_rw_box, A.n_box, 64, st, A); }
      if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_FSMOOTH, st); e = launch_flat_kernel(k_rw_fsmooth, A.n_fs, 256, st, A); }
    }
    if (e == hipSuccess) {
      Prof pr(c, SG_STAGE_RG_APPLY, st);
      if (q.feat) e = rw_feat_launch(c.N, q.bwd, A, q.Q, st);
      else if (spec_fwd) e = dispatch_N(c.N, [&](auto n) { return launch_tile_kernel<n()>(k_rw_spec<n()>, A.n_ap, st, A); });
      else if (q.spec) e = dispatch_N(c.N, [&](auto n) { return launch_tile_kernel<n()>(k_rw_spec_bwd<n()>, A.n_ap, st, A); });
      else e = dispatch_N(c.N, [&](auto n) { return launch_tile_kernel<n()>(k_rw_apply<n()>, A.n_ap, st, A); });
    }
    if (e == hipSuccess && !spec_fwd) { Prof pr(c, SG_STAGE_RG_OLA, st); e = launch_flat_kernel(k_rw_ola, A.n_ola, 256, st, A); }
    if (e != hipSuccess) {
      *err = std::string(who) + ": launch failed: " + hipGetErrorString(e);
      return SG_E_HIP;
    }
    ++S->last_batches;
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
  q.bwd = false; q.spec = false;
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
  q.bwd = true; q.spec = false;
  q.x = go_dev; q.dtype = dtype; q.B = B; q.L = L; q.x_stride = go_stride; q.lengths = lengths;
  q.out = gx_dev; q.out_dtype = dtype; q.out_stride = gx_stride;
  q.mask_in = mask;
  return run(sp, c, 0, q, max_ws, st, who, err);
}

int rw_spectrum(RwState** sp, const RgCtx& c, int kbox, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride,
                const int64_t* xn_lengths, void* spec_dev, float* mask_out, int64_t max_ws, hipStream_t st,
                std::string* err) {
  const char* who = "sg_gate_spectrum_rows";
  if (!geom_ok(c, who, err)) return SG_E_UNSUPPORTED;
  int rc = check_lengths(c, who, "lengths", lengths, B, L, err);
  if (rc) return rc;
  const bool use_xn = xn_dev && c.stationary;
  if (use_xn && (rc = check_lengths(c, who, "xn_lengths", xn_lengths, Bn, Ln, err))) return rc;
  if (!c.stationary && kbox < 1) { *err = std::string(who) + ": n_movemean must be at least 1"; return SG_E_INVALID; }
  Call q{};
  q.bwd = false; q.spec = true;
  q.x = x_dev; q.dtype = dtype; q.B = B; q.L = L; q.x_stride = x_stride; q.lengths = lengths;
  q.xn = use_xn ? xn_dev : nullptr; q.Bn = Bn; q.Ln = Ln; q.xn_stride = xn_stride; q.xn_lengths = use_xn ? xn_lengths : nullptr;
  q.out = spec_dev; q.out_dtype = dtype; q.out_stride = (1 + L / c.H) * (int64_t)c.F;
  q.mask_out = mask_out; q.mask_in = nullptr;
  return run(sp, c, kbox, q, max_ws, st, who, err);
}

int rw_spectrum_backward(RwState** sp, const RgCtx& c, const void* gs_dev, int dtype, int64_t B, int64_t L,
                         const int64_t* lengths, const float* mask, void* gx_dev, int64_t gx_stride, int64_t max_ws,
                         hipStream_t st, std::string* err) {
  const char* who = "sg_gate_spectrum_rows_backward";
  if (!geom_ok(c, who, err)) return SG_E_UNSUPPORTED;
  int rc = check_lengths(c, who, "lengths", lengths, B, L, err);
  if (rc) return rc;
  Call q{};
  q.bwd = true; q.spec = true;
  q.x = gs_dev; q.dtype = dtype; q.B = B; q.L = L; q.x_stride = (1 + L / c.H) * (int64_t)c.F; q.lengths = lengths;
  q.out = gx_dev; q.out_dtype = dtype; q.out_stride = gx_stride;
  q.mask_in = mask;
  return run(sp, c, 0, q, max_ws, st, who, err);
}
namespace {
int feat_args(const RgCtx& c, const char* who, const FeatBank& bank, int power, std::string* err) {
  if (!geom_ok(c, who, err)) return SG_E_UNSUPPORTED;
  if (power != 1 && power != 2) { *err = std::string(who) + ": power must be 1 or 2"; return SG_E_INVALID; }
  if (bank.M < 1 || bank.M > FEAT_MAX_FILTERS || !bank.fb || !bank.fbT || !bank.khull || !bank.mhull) {
    *err = std::string(who) + ": no filterbank set (sg_set_filterbank)";
    return SG_E_INVALID;
  }
  return SG_OK;
}
}  // namespace

int rw_features(RwState** sp, const RgCtx& c, int kbox, const FeatBank& bank, const void* x_dev, int dtype, int64_t B,
                int64_t L, int64_t x_stride, const int64_t* lengths, const void* xn_dev, int64_t Bn, int64_t Ln,
                int64_t xn_stride, const int64_t* xn_lengths, int power, int take_log, double eps, void* feat_dev,
                float* mask_out, int64_t max_ws, hipStream_t st, std::string* err) {
  const char* who = "sg_gate_features_rows";
  int rc = feat_args(c, who, bank, power, err);
  if (rc) return rc;
  if ((rc = check_lengths(c, who, "lengths", lengths, B, L, err))) return rc;
  const bool use_xn = xn_dev && c.stationary;
  if (use_xn && (rc = check_lengths(c, who, "xn_lengths", xn_lengths, Bn, Ln, err))) return rc;
  if (!c.stationary && kbox < 1) { *err = std::string(who) + ": n_movemean must be at least 1"; return SG_E_INVALID; }
  Call q{};
  q.bwd = false; q.spec = false; q.feat = true;
  q.Q = RwFeat{bank, nullptr, eps, take_log ? std::log(eps) : 0.0, power, take_log ? 1 : 0};
  q.x = x_dev; q.dtype = dtype; q.B = B; q.L = L; q.x_stride = x_stride; q.lengths = lengths;
  q.xn = use_xn ? xn_dev : nullptr; q.Bn = Bn; q.Ln = Ln; q.xn_stride = xn_stride; q.xn_lengths = use_xn ? xn_lengths : nullptr;
  q.out = feat_dev; q.out_dtype = dtype; q.out_stride = (1 + L / c.H) * (int64_t)bank.M;
  q.mask_out = mask_out; q.mask_in = nullptr;
  return run(sp, c, kbox, q, max_ws, st, who, err);
}

int rw_features_backward(RwState** sp, const RgCtx& c, const FeatBank& bank, const void* x_dev, int dtype, int64_t B,
                         int64_t L, int64_t x_stride, const int64_t* lengths, const void* grad_feat_dev, const float* mask,
                         int power, int take_log, double eps, void* gx_dev, int64_t gx_stride, int64_t max_ws,
                         hipStream_t st, std::string* err) {
  const char* who = "sg_gate_features_rows_backward";
  int rc = feat_args(c, who, bank, power, err);
  if (rc) return rc;
  if ((rc = check_lengths(c, who, "lengths", lengths, B, L, err))) return rc;
  Call q{};
  q.bwd = true; q.spec = false; q.feat = true;
  q.Q = RwFeat{bank, grad_feat_dev, eps, 0.0, power, take_log ? 1 : 0};
  q.x = x_dev; q.dtype = dtype; q.B = B; q.L = L; q.x_stride = x_stride; q.lengths = lengths;
  q.out = gx_dev; q.out_dtype = dtype; q.out_stride = gx_stride;
  q.mask_in = mask;
  return run(sp, c, 0, q, max_ws, st, who, err);
}
}  // namespace sg
