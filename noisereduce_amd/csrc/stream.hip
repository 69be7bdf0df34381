// Banks of live streams (sg_stream_push): tables, kernels and the host side.  See stream.hpp and DESIGN section 13.
//
// Four launches per step, each driven by a tile table built on the host (one upload per step):
//   k_st_decide   one workgroup per (stream, channel) with newly decidable frames, frames IN ORDER: float64 transform,
//                 running band maximum (a prefix maximum: frame t's floor never sees frame t + 1), final raw-mask bits
//   k_st_fsmooth  frequency smoothing of the bit rows the step's applied frames read
//   k_st_apply    time smoothing, prop_decrease, masked multiply, inverse transform (the frame is transformed again from
//                 the ring / the caller's block)
//   k_st_finish   overlap-add of the newly final samples into the caller's output + partial sums of the samples still
//                 open (carry), then the state update: block -> ring, band maxima of flushed streams cleared
// A non-stationary bank (sg_stream_create_nonstationary) runs the same four launches with k_sn_decide in the first place:
// float64 transform, A = |X|, the forward one-pole pass carried per band, the A / fwd rows of the last L + 1 frames kept,
// and for every frame that has L frames after it (or the stream's end, at a flush) the backward pass over those L + 1
// rows and the sigmoid into a ring of float mask rows, which k_st_fsmooth<true> / k_st_apply<N, true> read instead of bits.
// A box bank (a handle of variant T) is a non-stationary bank with k_sb_decide in the first place: the
// level of a frame is TorchGate's moving mean over the K rows of A around it (no forward pass, no fwd rows), the sigmoid rows
// go to the same mk ring, k_st_fsmooth<true> is unchanged and k_st_apply / k_st_feat take their BX form, TorchGate's mask
// formula on those rows.
// An adaptive bank (sg_stream_create_adaptive) is a stationary bank without a noise profile: k_sa_decide takes the first
// place and learns the threshold of every band from the stream itself, a running weighted mean and deviation of the
// floored dB values carried per band (nst), evaluated frame by frame before the compare.  The other three launches are the
// stationary ones.
// What a frame goes through is tile_core.hpp's, shared with ragged.hip and rows.hip; this file holds what only a stream
// has: the ring / block loader, the decisions against a RUNNING band maximum, the carried recurrence, the carry of the
// overlap-add and the state update.
// An exact bank (sg_stream_create_ex, exact != 0) runs the same four launches in their exact instantiations: the segment
// rows are float64 (k_st_apply<N, NS, true>: double2 stores, the float form's lane-to-sample mapping), k_st_finish<true>
// sums them and stores the float64 value through geom.hpp's store_sample(double) -- float64 as is, float32 rounded once,
// int16 / int32 truncated toward zero, NaN -> 0.  A non-stationary exact bank also keeps the sigmoid ring mk and the
// smoothed rows R in float64 (k_sn_decide<N, true>: the sigmoid in float64; k_st_fsmooth<true, true>); a stationary or
// adaptive one keeps float R, which holds small integers there and is exact already.
// State transfer (sg_stream_export / sg_stream_import) is two more kernels, k_st_export and k_st_import, outside the step: one
// launch per call copies the live part of the listed slots' state to / from a canonical payload.
// A spectrum step (sg_stream_push_spectrum) is the same four launches with k_st_apply<N, NS, EX, true> in the third place:
// it also stores every applied frame's gated spectrum Y = Z * mask (and, on request, the mask row) to the caller's buffers
// on its way to the inverse transform.  No state, workspace or stage of its own.
// A feature step (sg_stream_push_features) puts k_st_feat<N, NS, EX> in the third place instead: the same frame, mask and
// inverse, with the powers |s Y|^power of the frame's bins written to an LDS row of their own and reduced over the bank's
// filterbank (sg_stream_set_filterbank; feat_sum.hpp's filter sum, shared with rows_feat.hip) before the next frame reuses
// the row.  What it needs beyond StArgs is a second kernel argument: StArgs does not move.
// Nothing waits on another workgroup.  No workgroup reads state that another workgroup of the same launch writes: the
// ring is only written by k_st_finish (which does not read it), the carry is double buffered, the bit rows of a unit are
// written by its one decide workgroup.  One fixed evaluation order per frame and per output sample: a stream's output
// does not depend on the block split, the slot, or the other streams of the step.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "tile_core.hpp"
#include "feat_sum.hpp"
#include "feat_tables.hpp"
#include "stream.hpp"
#include "../../include/mi355gate_debug.h"

namespace sg {

// ---- tables ------------------------------------------------------------------------------------------------------
// What k_st_feat needs beyond StArgs, as a second kernel argument (as RwFeat is k_rw_feat's).
struct StFeat {
  FeatBank bank;          // the bank's own filterbank (sg_stream_set_filterbank)
  void* feat;             // [unit][frame][M] of dtype
  void* fmask;            // final mask rows [unit][frame][F] of dtype, or null
  const StFeatUnit* fu;   // [unit]
  double eps;
  double scale;           // s of |s Z mask|^power: mag_scale (the spectrum step's factor) or the caller's
  int32_t dtype, power, take_log;
};

struct StArgs {
  const void* x; int in_dtype;
  void* out; int out_dtype;
  const StUnit* units;
  const Tile* tiles;
  int64_t t_dec, n_dec, t_fs, n_fs, t_ap, n_ap, t_fin, n_fin;
  double* ring;
  unsigned long long* bits;
  double* rmax;
  double* carry;
  const double* thr;
  const double* T2;
  void* R;         // smoothed rows: float, double in a non-stationary exact bank
  void* seg;       // segment rows: float, double in an exact bank
  int RC, RB;
  // non-stationary banks
  double* fst;     // [unit][FS] forward state fwd[f, td]
  double* fa;      // [unit][RF][2][FS] A and fwd rows of the last transformed frames, frame t at t % RF (box bank: [unit][RF][FS], A alone)
  void* mk;        // [unit][RB][FS] raw (sigmoid) mask rows, frame t at t % RB: float, double in an exact bank
  int RF, L;
  // adaptive banks
  double* nst;     // [unit][3][FS] weight sum Wn, mean mu and weighted squared deviations M2 of the floored dB values
  double lam;      // forgetting factor per frame, (0, 1]
  int64_t learn;   // frames that update the statistics (negative: all of them)
  TileConsts c;
  // spectrum steps (k_st_apply<.., true> alone reads these; they come last so that nothing above moves)
  void* spec;        // gated spectra: float2, double2 for spec_dtype == SG_F64
  void* smask;       // final mask rows in the real type of spec_dtype, or null
  const StSpec* sp;  // [unit]
  int spec_dtype;
  // box banks (k_sb_decide alone reads these): frames of the moving mean, and how many of them lie behind the decided one
  int K, Lb;
};

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
  const int64_t s0 = t * A.c.H - A.c.padL;
  frame_fft<N>(buf, tw, lane, [&](int jj) -> double { return jj < A.c.W ? st_sample(A, U, s0 + jj) * A.c.wfull[jj] : 0.0; });
}

// ---- thresholds of slots: dB -> compare constant on the raw power ------------------------------------------------------
__global__ __launch_bounds__(64) void k_st_thresh(const double* src, const int32_t* slots, double* thr, double* T2, int F, int FS,
                                                  double mag_scale) {
  const int64_t s = slots[blockIdx.x];
  for (int f = threadIdx.x; f < F; f += 64) {
    const double th = src[f];
    thr[s * FS + f] = th;
    T2[s * FS + f] = thresh_to_t2(th, mag_scale);
  }
}

// ---- decide: the unit's new frames in order ------------------------------------------------------------------------
// Not tile_core's decide_frame: the band maximum is a RUNNING one, so the floor's band mode is carried per band and
// re-evaluated whenever the maximum moves, and the stored bit is final (the offline paths apply the mode in *_fsmooth).
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_st_decide(StArgs A) {
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_dec + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  constexpr int M = tile_bins<N>();
  const double* T2 = A.T2 + (int64_t)U.slot * A.c.FS;
  const double* thr = A.thr + (int64_t)U.slot * A.c.FS;
  double* rmax = A.rmax + (int64_t)U.state * A.c.FS;
  double rm[M];
  int md[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int k = lane + NT * m;
    rm[m] = 0.0;
    md[m] = 2;
    if (k <= N) {
      rm[m] = rmax[k];
      md[m] = band_mode(rm[m], thr[k], T2[k], A.c.mag_scale, A.c.top_db);
    }
  }
  for (int64_t t = tl.a; t < tl.b; ++t) {
    st_frame_fft<N>(A, U, t, buf, tw, lane);
    unsigned long long* row = A.bits + ((int64_t)U.state * A.RB + t % A.RB) * A.c.wpr;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      bool pass = false;
      if (k <= N) {
        const double P = bin_power<N>(buf, tw, k);
        if (P != P || P > rm[m]) {   // the maximum moves: so may the band's floor
          rm[m] = nanmax(rm[m], P);
          md[m] = band_mode(rm[m], thr[k], T2[k], A.c.mag_scale, A.c.top_db);
        }
        pass = md[m] == 1 || (md[m] == 0 && P > T2[k]);
      }
      store_ballot(row, A.c.wpr, lane, k, pass);
    }
    team_sync<SY>();
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int k = lane + NT * m;
    if (k <= N) rmax[k] = rm[m];
  }
}

// ---- adaptive decide: the threshold of a band is learnt from the stream's own frames -----------------------------------
// Per band, frames in order (the recurrence IS the definition; West's weighted incremental moments):
//   rmax = max(rmax, dB)   x = max(dB, rmax - top_db)
//   while learning:  Wn = lam Wn + 1,  d = x - mu,  mu += d / Wn,  M2 = lam M2 + d (x - mu)
//   thr = mu + n_std sqrt(M2 / Wn)   pass = x > thr
// Frame t is part of its own threshold.  The compare is in dB: the threshold moves with every frame, so there is no compare
// constant on the raw power and no band mode.  The running maximum lives in registers as its dB value; the state keeps the
// power that gave it (what k_st_decide keeps), written when the maximum moves and turned into dB again at the next entry:
// cell_db of the same double, so the same bits whatever the block split.  (A fourth register array for the power costs
// n_fft = 1024 its registers: the one-wavefront team then spills.)  A constant band has d = 0 exactly: mu and M2 stay exact
// and the compare is exactly false, which S2 / n - mean^2 would leave to rounding.  Wn depends on the frame only; it is
// stored per band so that a unit's state is self-contained.  The moments are evaluated without contraction: one rounding
// per operation of the recurrence as written.
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_sa_decide(StArgs A) {
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_dec + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  constexpr int M = tile_bins<N>();
  const int FS = A.c.FS;
  double* rmax = A.rmax + (int64_t)U.state * FS;
  double* nst = A.nst + (int64_t)U.state * 3 * FS;
  double rd[M], mu[M], m2[M];
  double wn = nst[lane];   // (lane < NT <= N: a band of the unit)
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int k = lane + NT * m;
    rd[m] = mu[m] = m2[m] = 0.0;
    if (k <= N) {
      rd[m] = cell_db(rmax[k], A.c.mag_scale);
      mu[m] = nst[FS + k];
      m2[m] = nst[2 * FS + k];
    }
  }
  for (int64_t t = tl.a; t < tl.b; ++t) {
    st_frame_fft<N>(A, U, t, buf, tw, lane);
    unsigned long long* row = A.bits + ((int64_t)U.state * A.RB + t % A.RB) * A.c.wpr;
    const bool learn = A.learn < 0 || t < A.learn;
    if (learn) wn = A.lam * wn + 1.0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      bool pass = false;
      if (k <= N) {
        const double P = bin_power<N>(buf, tw, k);
        const double db = cell_db(P, A.c.mag_scale);
        if (db != db || db > rd[m]) {   // the maximum moves (NaN-sticky): its power goes to the state at once
          rd[m] = nanmax(rd[m], db);
          rmax[k] = (rd[m] != rd[m]) ? (double)NAN : P;
        }
        {
#pragma clang fp contract(off)
          const double x = nanmax(db, rd[m] - A.c.top_db);
          if (learn) {
            const double d = x - mu[m];
            mu[m] = mu[m] + d / wn;
            m2[m] = A.lam * m2[m] + d * (x - mu[m]);
          }
          const double thr = mu[m] + A.c.n_std * sqrt(m2[m] / wn);
          pass = x > thr;
        }
      }
      store_ballot(row, A.c.wpr, lane, k, pass);
    }
    team_sync<SY>();
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int k = lane + NT * m;
    if (k <= N) {
      nst[k] = wn;
      nst[FS + k] = mu[m];
      nst[2 * FS + k] = m2[m];
    }
  }
}

// ---- non-stationary decide: forward pass over the unit's new frames, backward pass + sigmoid of the decidable ones ------
// Band k belongs to one thread for the whole launch: the A / fwd rows it reads in the second loop are its own stores of
// the first loop or of an earlier step, so no barrier separates the two.  S_L[f, t] = the reference's forward-backward
// smoother of frames 0 .. e, e = min(t + L, last frame): seeded with fwd[e], then k = e .. t in that order whatever the
// block split.  The sigmoid is the offline kernels' (geom.hpp sigmoid_ratio): S = 0 gives 0 / 0 = NaN as there.
// EX: the rows of an exact bank, float64, the sigmoid evaluated in float64 as the reference does (exact.hpp's form).
template <int N, bool EX>
__global__ __launch_bounds__(tile_nt<N>()) void k_sn_decide(StArgs A) {
  using MT = typename std::conditional<EX, double, float>::type;
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_dec + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  constexpr int M = tile_bins<N>();
  const int FS = A.c.FS;
  const double b = A.c.iir_b, c = 1.0 - A.c.iir_b;
  const float nthresh = (float)A.c.nthresh, slope = (float)A.c.slope;
  double* fst = A.fst + (int64_t)U.state * FS;
  double* fa = A.fa + (int64_t)U.state * A.RF * 2 * FS;
  double fw[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int k = lane + NT * m;
    fw[m] = (k <= N && U.td0 >= 0) ? fst[k] : 0.0;
  }
  for (int64_t t = U.td0 + 1; t <= U.td1; ++t) {
    st_frame_fft<N>(A, U, t, buf, tw, lane);
    double* row = fa + (t % A.RF) * 2 * FS;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      if (k <= N) {
        const double a = sqrt(bin_power<N>(buf, tw, k));
        if (t == 0) fw[m] = a;   // fwd[f, -1] = A[f, 0]
        fw[m] = b * a + c * fw[m];
        row[k] = a;
        row[FS + k] = fw[m];
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
    MT* mrow = (MT*)A.mk + ((int64_t)U.state * A.RB + t % A.RB) * FS;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      if (k <= N) {
        double s = fa[((e % A.RF) * 2 + 1) * FS + k];
        for (int64_t q = e; q >= t; --q) s = b * fa[((q % A.RF) * 2 + 1) * FS + k] + c * s;
        const double a = fa[(t % A.RF) * 2 * FS + k];
        if constexpr (EX) mrow[k] = 1.0 / (1.0 + exp(-((a - s) / s - A.c.nthresh) * A.c.slope));
        else mrow[k] = sigmoid_ratio(a, s, nthresh, slope);
      }
    }
  }
}

// ---- box decide: TorchGate's non-stationary gate, the level a moving mean over K frames --------------------------------
// The first loop is k_sn_decide's without the forward pass: a row of the fa ring is the FS magnitudes A = |X| of one frame
// (no fwd half, no fst).  The level of frame t is rows.hip's k_rw_box on the ring: S = (1 / K) sum of A[q], q ascending over
// [t - Lb, t - Lb + K) cut to [0, last frame], every window summed afresh in float64 -- frames outside the stream count as
// 0, the divisor stays K (conv1d(|X|, ones(K) / K, padding="same")).  A push decides t once t + L = t - Lb + K - 1 is in, so
// only a flush cuts the window at its upper end (U.td1 is the stream's last frame then).  The ring keeps rows (ts - Lb, td]
// (stream_plan.hpp's RF): frame ts0 + 1 still finds its Lb rows behind it, whatever the block split.  Band k belongs to one
// thread for the whole launch, as in k_sn_decide: no barrier between the loops.
template <int N, bool EX>
__global__ __launch_bounds__(tile_nt<N>()) void k_sb_decide(StArgs A) {
  using MT = typename std::conditional<EX, double, float>::type;
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_dec + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  constexpr int M = tile_bins<N>();
  const int FS = A.c.FS;
  const float nthresh = (float)A.c.nthresh, slope = (float)A.c.slope;
  double* fa = A.fa + (int64_t)U.state * A.RF * FS;
  for (int64_t t = U.td0 + 1; t <= U.td1; ++t) {
    st_frame_fft<N>(A, U, t, buf, tw, lane);
    double* row = fa + (t % A.RF) * FS;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      if (k <= N) row[k] = sqrt(bin_power<N>(buf, tw, k));
    }
    team_sync<SY>();
  }
  const double kbox = (double)A.K;
  for (int64_t t = U.ts0 + 1; t <= U.ts1; ++t) {
    const int64_t ja = t - A.Lb < 0 ? 0 : t - A.Lb;
    const int64_t jb = t - A.Lb + A.K > U.td1 + 1 ? U.td1 + 1 : t - A.Lb + A.K;
    const int r0 = (int)(ja % A.RF), nq = (int)(jb - ja);
    const double* arow = fa + (t % A.RF) * FS;
    MT* mrow = (MT*)A.mk + ((int64_t)U.state * A.RB + t % A.RB) * FS;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const int k = lane + NT * m;
      if (k <= N) {
        double s = 0.0;
        int r = r0;
        for (int q = 0; q < nq; ++q) {
          s += fa[(int64_t)r * FS + k];
          if (++r == A.RF) r = 0;
        }
        s = s / kbox;
        const double a = arow[k];
        if constexpr (EX) mrow[k] = 1.0 / (1.0 + exp(-((a - s) / s - A.c.nthresh) * A.c.slope));
        else mrow[k] = sigmoid_ratio(a, s, nthresh, slope);
      }
    }
  }
}

// ---- mask smoothing along frequency (fsmooth_row) -------------------------------------------------------------------
// NS: the raw mask is a row of floats (the sigmoid) instead of a row of final bits; EX (with NS): a row of doubles,
// summed in double in the same ascending df order
template <bool NS, bool EX>
__global__ __launch_bounds__(256) void k_st_fsmooth(StArgs A) {
  using RT = typename std::conditional<EX, double, float>::type;
  if ((int64_t)blockIdx.x >= A.n_fs) return;
  const Tile tl = A.tiles[A.t_fs + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  for (int64_t r = tl.a; r < tl.b; ++r) {
    const unsigned long long* brow = NS ? nullptr : A.bits + ((int64_t)U.state * A.RB + r % A.RB) * A.c.wpr;
    const RT* frow = NS ? (const RT*)A.mk + ((int64_t)U.state * A.RB + r % A.RB) * A.c.FS : nullptr;
    fsmooth_row((RT*)A.R + (U.mrow + r - U.r0) * A.c.FS, A.c.F, A.c.nf,
                [&](int g) -> RT { return NS ? frow[g] : (RT)bit_at(brow, g); });
  }
}

// ---- applied frames: time smoothing, masked multiply, inverse transform ------------------------------------------------
// EX: float64 segment rows; float64 smoothed rows too where the raw mask is the sigmoid (NS)
// SP: the frame's gated spectrum goes to the caller as well.  Y[t, k] = X[k] * mask * mag_scale is the product that is
// merged and inverted, in scipy.signal.stft's scaling (1 / sum(window): the inverse folds that factor into its window,
// the store applies it), rounded once to spec's type; the mask value is the float64 one of that product.  Bins 0 and
// n_fft / 2 carry an imaginary part of +0.0.  A lane's bins are lane + NT i and N - (lane + NT i): consecutive lanes
// store consecutive float2 / double2 of the row in both halves.
// BX (with NS): a box bank.  Its rows are sigmoid rows as any non-stationary bank's, its mask is TorchGate's:
// mask_stationary's formula on them, prop_decrease first, then the zero-padded smoothing.
// A box bank's mask, split, product and merge are evaluated WITHOUT contraction (mask_box, mask_and_invert_pinned: the
// arithmetic of tile_core.hpp's mask_stationary and mask_and_invert, one rounding per operation as written).  Under
// contraction the compiler fuses a product into a following addition when the product has no other use: Y = X * mask has one
// use in k_st_apply and two in k_st_feat (the merge and the feature callback), and a * b + c * d leaves it the choice of the
// product.  An exact bank keeps its segments in float64, so its push and push_features audio then differed in the last bit
// (4.4e-16 of peak on 3626 of 6733 samples, measured), which the contract of a stream forbids.  tile_core.hpp's own
// functions stay as they are: every existing kernel keeps its bits.
__device__ __forceinline__ double mask_box(const TileConsts& C, double K, double Et, int k) {
#pragma clang fp contract(off)
  return (C.prop * K + (1.0 - C.prop) * Et * (double)tri_valid(C.nf, k, C.F)) / C.ktot;
}
template <int N, class ST, class MaskAt, class Emit = NoEmit>
__device__ __forceinline__ void mask_and_invert_pinned(cx<double>* buf, const cx<double>* tw, int lane, MaskAt&& mask_at,
                                                       const double* wfull, ST* seg_row, Emit&& emit = Emit()) {
#pragma clang fp contract(off)
  constexpr int NT = tile_nt<N>();
  for (int k = lane; k <= N / 2; k += NT) {
    if (k == 0) {
      const cx<double> a = buf[lp<double>(0)];
      const double m0 = mask_at(0), mN = mask_at(N);
      const double y0 = (a.x + a.y) * m0, yN = (a.x - a.y) * mN;
      emit(0, cx<double>{y0, 0.0}, m0);
      emit(N, cx<double>{yN, 0.0}, mN);
      buf[lp<double>(0)] = {0.5 * (y0 + yN), 0.5 * (y0 - yN)};
    } else {
      const cx<double> a = buf[lp<double>(k)], b = buf[lp<double>(N - k)], w = tw[k];
      const cx<double> E = {(a.x + b.x) * 0.5, (a.y - b.y) * 0.5};
      const cx<double> O = {(a.y + b.y) * 0.5, (b.x - a.x) * 0.5};
      const cx<double> wO = {w.x * O.x - w.y * O.y, w.x * O.y + w.y * O.x};
      const double mk = mask_at(k), mn = (k != N - k) ? mask_at(N - k) : mk;
      const cx<double> Yk = {(E.x + wO.x) * mk, (E.y + wO.y) * mk};
      const cx<double> Yn = {(E.x - wO.x) * mn, (-E.y + wO.y) * mn};
      emit(k, Yk, mk);
      if (k != N - k) emit(N - k, Yn, mn);
      const cx<double> Ep = {(Yk.x + Yn.x) * 0.5, (Yk.y - Yn.y) * 0.5};
      const cx<double> D = {(Yk.x - Yn.x) * 0.5, (Yk.y + Yn.y) * 0.5};
      const cx<double> Op = {D.x * w.x + D.y * w.y, D.y * w.x - D.x * w.y};   // D * conj(w)
      buf[lp<double>(k)] = {Ep.x - Op.y, Ep.y + Op.x};
      if (k != N - k) buf[lp<double>(N - k)] = {Ep.x + Op.y, -Ep.y + Op.x};
    }
  }
  invert_and_window<N, ST>(buf, tw, lane, wfull, 1.0 / (double)N, seg_row);
}
template <int N, bool NS, bool EX, bool SP = false, bool BX = false>
__global__ __launch_bounds__(tile_nt<N>()) void k_st_apply(StArgs A) {
  using ST = typename std::conditional<EX, double, float>::type;
  using RT = typename std::conditional<EX && NS, double, float>::type;
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_ap + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    st_frame_fft<N>(A, U, t, buf, tw, lane);
    const TimeTaps tp = time_taps(t, A.c.nt, U.Tend);
    auto mask_at = [&](int k) -> double {
      const double K = time_smooth((const RT*)A.R, A.c.FS, [&](int64_t q) { return U.mrow + q - U.r0; }, tp, t, A.c.nt, k);
      if constexpr (BX) return mask_box(A.c, K, tp.Et, k);
      return NS ? mask_nonstationary(A.c, K) : mask_stationary(A.c, K, tp.Et, k);
    };
    ST* seg_row = (ST*)A.seg + (U.srow + t - (U.ta0 + 1)) * (int64_t)A.c.n;
    if constexpr (SP) {
      const StSpec S = A.sp[tl.idx];
      const int64_t row = (t - (U.ta0 + 1)) * (int64_t)A.c.F;
      const bool wide = A.spec_dtype == SG_F64;
      mask_and_invert<N>(buf, tw, lane, mask_at, A.c.wfull, seg_row, [&](int k, cx<double> Y, double m) {
        const double re = Y.x * A.c.mag_scale, im = (k == 0 || k == N) ? 0.0 : Y.y * A.c.mag_scale;
        if (wide) reinterpret_cast<double2*>(A.spec)[S.spec_off + row + k] = make_double2(re, im);
        else reinterpret_cast<float2*>(A.spec)[S.spec_off + row + k] = make_float2((float)re, (float)im);
        if (A.smask) {
          if (wide) reinterpret_cast<double*>(A.smask)[S.mask_off + row + k] = m;
          else reinterpret_cast<float*>(A.smask)[S.mask_off + row + k] = (float)m;
        }
      });
    } else if constexpr (BX) {
      mask_and_invert_pinned<N>(buf, tw, lane, mask_at, A.c.wfull, seg_row);
    } else {
      mask_and_invert<N>(buf, tw, lane, mask_at, A.c.wfull, seg_row);
    }
  }
}

// ---- applied frames of a feature step: k_st_apply's frame, mask and inverse, plus the filterbank features ---------------
// The callback of mask_and_invert sees every band's product Y[k] = X[k] * mask once and writes p[k] = |s Y[k]|^power
// (feat_power: the real and imaginary parts are scaled first, as the spectrum step scales them at its store, then
// squared) into prow, an LDS row of N + 1 doubles behind the frame buffer -- the frame itself has to survive for the
// inverse, so the powers cannot go into buf as in k_rw_feat.  The inverse's closing team_sync makes the row visible to
// the team; then lane m, m + NT, ... sums filter m over its hull (feat_filter_sum: ascending k, float64) and stores it,
// consecutive lanes consecutive filters, rounded once to the output type.  A second team_sync keeps the next frame's
// powers off the row until every lane has read it.  Power, log and the output type are run-time switches (uniform
// branches).  LDS: launch_tile_kernel's + (N + 1) doubles.
template <int N, bool NS, bool EX, bool BX = false>
__global__ __launch_bounds__(tile_nt<N>()) void k_st_feat(StArgs A, StFeat Q) {
  using ST = typename std::conditional<EX, double, float>::type;
  using RT = typename std::conditional<EX && NS, double, float>::type;
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  double* prow = reinterpret_cast<double*>(buf + lpn<double>(N));
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_ap + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  const int M = Q.bank.M;
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    st_frame_fft<N>(A, U, t, buf, tw, lane);
    const TimeTaps tp = time_taps(t, A.c.nt, U.Tend);
    auto mask_at = [&](int k) -> double {
      const double K = time_smooth((const RT*)A.R, A.c.FS, [&](int64_t q) { return U.mrow + q - U.r0; }, tp, t, A.c.nt, k);
      if constexpr (BX) return mask_box(A.c, K, tp.Et, k);
      return NS ? mask_nonstationary(A.c, K) : mask_stationary(A.c, K, tp.Et, k);
    };
    ST* seg_row = (ST*)A.seg + (U.srow + t - (U.ta0 + 1)) * (int64_t)A.c.n;
    const StFeatUnit S = Q.fu[tl.idx];
    const int64_t fr = t - (U.ta0 + 1);
    const int64_t mrow = S.mask_off + fr * (int64_t)A.c.F;
    auto emit = [&](int k, cx<double> Y, double m) {
      prow[k] = feat_power(Y, Q.scale, Q.power);
      if (Q.fmask) feat_store(Q.fmask, Q.dtype, mrow + k, m);
    };
    if constexpr (BX) mask_and_invert_pinned<N>(buf, tw, lane, mask_at, A.c.wfull, seg_row, emit);
    else mask_and_invert<N>(buf, tw, lane, mask_at, A.c.wfull, seg_row, emit);
    const int64_t frow = S.feat_off + fr * (int64_t)M;
    for (int m = fresh_lane(lane); m < M; m += NT) {
      const double lin = feat_filter_sum(Q.bank, A.c.F, m, [&](int k) { return prow[k]; }, prow[N]);
      feat_store(Q.feat, Q.dtype, frow + m, Q.take_log ? log(lin + Q.eps) : lin);
    }
    team_sync<SY>();
  }
}

// ---- overlap-add of the newly final samples, partial sums of the open ones, state update ----------------------------
// Sample p sums its frames in frame order, continuing the partial sum an earlier step left in the carry: the additions
// are the same whatever the block split.  out = sum seg / sum w^2; positions >= Lout are the zero tail.
// EX: float64 segments, and the float64 value goes to the caller's sample type without a detour through float32.
template <bool EX>
__global__ __launch_bounds__(256) void k_st_finish(StArgs A) {
  using ST = typename std::conditional<EX, double, float>::type;
  if ((int64_t)blockIdx.x >= A.n_fin) return;
  const Tile tl = A.tiles[A.t_fin + blockIdx.x];
  const StUnit U = A.units[tl.idx];
  const int W = A.c.W, H = A.c.H;
  if (tl.kind == ST_CLEAR) {
    for (int f = threadIdx.x; f < A.c.FS; f += blockDim.x) A.rmax[(int64_t)U.state * A.c.FS + f] = 0.0;
    if (A.nst)
      for (int f = threadIdx.x; f < 3 * A.c.FS; f += blockDim.x) A.nst[(int64_t)U.state * 3 * A.c.FS + f] = 0.0;
    return;
  }
  const int64_t p = tl.a + threadIdx.x;
  if (p >= tl.b) return;
  if (tl.kind == ST_APPEND) {
    A.ring[(int64_t)U.state * A.RC + p % A.RC] = load_sample(A.x, A.in_dtype, U.in_off + (p - U.n0));
    return;
  }
  const double* cold = A.carry + ((int64_t)U.state * 2 + U.par) * W;
  double* cnew = A.carry + ((int64_t)U.state * 2 + (U.par ^ 1)) * W;
  const int64_t e = p + A.c.padL;
  int64_t t_lo, t_hi;
  ola_span(e, W, H, U.Tend, &t_lo, &t_hi);
  double acc = p < U.cov0 ? cold[p % W] : 0.0;
  const int64_t ta = t_lo > U.ta0 + 1 ? t_lo : U.ta0 + 1, tb = t_hi < U.ta1 ? t_hi : U.ta1;
  for (int64_t t = ta; t <= tb; ++t)
    acc += (double)((const ST*)A.seg)[(U.srow + t - (U.ta0 + 1)) * (int64_t)A.c.n + (int)(e - t * H)];
  if (p >= U.E1) {
    cnew[p % W] = acc;
    return;
  }
  double val = 0.0;
  if (!U.flush || p < U.Lout) {
    const double norm = ola_envelope(A.c.wfull, e, H, t_lo, t_hi);
    val = norm > 1e-10 ? acc / norm : acc;
  }
  if constexpr (EX) store_sample(A.out, A.out_dtype, U.out_off + (p - U.E0), val);
  else store_sample(A.out, A.out_dtype, U.out_off + (p - U.E0), (float)val);
}

// ---- state transfer: a slot's live state <-> a canonical payload (sg_stream_export / sg_stream_import) ------------------
// Everything a stream keeps is 8-byte words (a float mask row is FS / 2 of them, FS being a multiple of 16), so both
// directions are one copy kernel over a table of fields.  A field is `rows` rows of rw words that live in a ring of R rows
// on the device, row first + i at position (first + i) % R, and lie in index order in the payload: the payload does not
// know RB or RF, which depend on max_block.  A tile is up to XW words of one field.  Export only reads state, import only
// writes it, and a slot appears once per call: no workgroup reads what another one of the launch writes.
struct StXField {
  unsigned long long* dev;   // row 0 of the ring on the device
  int64_t blob;              // word of the payload buffer holding word 0 of the field
  uint32_t first, R, rw, pad;   // first live row's ring position (< R), rows of the ring, words per row
};
struct StXArgs {
  unsigned long long* blob;
  const StXField* fields;
  const Tile* tiles;
  int64_t n_tiles;
};
constexpr int XW = 2048;   // words per tile: 8 per thread, all loads in flight before the first store

template <bool IMPORT>
__device__ __forceinline__ void st_copy_tile(const StXArgs& A) {
  if ((int64_t)blockIdx.x >= A.n_tiles) return;
  const Tile tl = A.tiles[blockIdx.x];
  const StXField f = A.fields[tl.idx];
  const uint32_t w0 = (uint32_t)tl.a + threadIdx.x, w1 = (uint32_t)tl.b;
  unsigned long long* blob = A.blob + f.blob;
  unsigned long long v[XW / 256];
  int64_t at[XW / 256];
#pragma unroll
  for (int q = 0; q < XW / 256; ++q) {
    const uint32_t w = w0 + 256u * q;
    v[q] = 0;
    at[q] = 0;
    if (w < w1) {
      const uint32_t i = w / f.rw, j = w - i * f.rw;
      uint32_t row = f.first + i;   // (i < R: a field never holds more rows than its ring)
      if (row >= f.R) row -= f.R;
      at[q] = (int64_t)row * f.rw + j;
      v[q] = IMPORT ? blob[w] : f.dev[at[q]];
    }
  }
#pragma unroll
  for (int q = 0; q < XW / 256; ++q) {
    const uint32_t w = w0 + 256u * q;
    if (w < w1) {
      if (IMPORT) f.dev[at[q]] = v[q];
      else blob[w] = v[q];
    }
  }
}
__global__ __launch_bounds__(256) void k_st_export(StXArgs A) { st_copy_tile<false>(A); }
__global__ __launch_bounds__(256) void k_st_import(StXArgs A) { st_copy_tile<true>(A); }

// ---- host side ---------------------------------------------------------------------------------------------------
struct StBank {
  RgCtx c{};
  int n_slots = 0, C = 0, RC = 0, RB = 0, wpr = 0;
  int ns = 0, L = 0, RF = 0;   // non-stationary bank, its lookahead in frames, depth of the A / fwd ring
  int ad = 0;                  // adaptive bank: the noise statistics are learnt from the stream (nst)
  int exact = 0;               // exact bank: float64 segments (and sigmoid rows), any sample type in and out
  int box = 0, K = 0, Lb = 0;  // box bank (ns too): frames of the moving mean, those of them behind the decided frame
  host::DevBuf wleft;          // box bank with win_length < n_fft: the window at the START of an n_fft frame (c.wfull64)
  double lam = 1.0;
  int64_t learn = -1;
  int64_t max_block = 0;
  // the buffers of stream_plan.hpp's StLayout (a kind of bank leaves those it does not have empty); tabs and ws grow
  host::DevBuf ring, carry, fst, fa, mk, rmax, bits, nst, thr, T2, stage, slot_list, tabs, ws;
  // the bank's own filterbank (st_set_filterbank): one allocation holding fb [F][M], fbT [M][F], khull [M] and mhull [F]
  host::DevBuf fbank;
  FeatBank fb{};   // pointers into fbank; M == 0: none set
  std::vector<StSlot> slots;
};

void st_destroy(StBank* b) { delete b; }

namespace {
StGeo st_geo(const RgCtx& c, int64_t channels, bool ns, int64_t lookahead, bool adaptive, bool exact, int64_t box_k = 0) {
  if (box_k) return st_make_geo_box(c.n, c.F, c.FS, c.W, c.H, c.nt, box_k, channels, exact);
  return st_make_geo(c.n, c.F, c.FS, c.W, c.H, c.nt, lookahead, channels,
                     adaptive ? SG_STREAM_ADAPTIVE : ns ? SG_STREAM_NONSTATIONARY : SG_STREAM_FIXED, exact);
}
StGeo st_geo(const StBank* b) { return st_geo(b->c, b->C, b->ns != 0, b->L, b->ad != 0, b->exact != 0, b->box ? b->K : 0); }
// what a box bank refuses
int box_refuses(const StBank* b, const char* who, const char* why, std::string* err) {
  if (!b->box) return SG_OK;
  *err = std::string(who) + ": not on a bank of TorchGate's gate (" + why + ")";
  return SG_E_INVALID;
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

namespace {
// k_st_feat of geometry N: launch_tile_kernel's LDS plus the row of N + 1 powers (16-byte granules).  At n_fft = 4096
// that is 32 KiB of twiddles, 36 KiB of padded frame and 16 KiB of powers, 86032 bytes: one workgroup per CU where the
// spectrum step's 69632 bytes allow two (160 KiB per CU); 43024 bytes (three per CU against four) at n_fft = 2048
template <int N>
hipError_t launch_feat_kernel(void (*kernel)(StArgs, StFeat), int64_t ntiles, hipStream_t st, const StArgs& A, const StFeat& Q) {
  const size_t lds = (size_t)(N + lpn<double>(N)) * sizeof(cx<double>) + ((size_t)(N + 1) * sizeof(double) + 15) / 16 * 16;
  return host::launch_lds_if(lds > 65536, kernel, tile_grid(ntiles), dim3(tile_nt<N>()), lds, st, A, Q);
}
}  // namespace

int64_t st_state_bytes(const RgCtx& c, bool ns, int64_t n_slots, int64_t channels, int64_t max_block, int64_t L, bool adaptive,
                       bool exact, int32_t box_k) {
  return st_layout(st_geo(c, channels, ns, L, adaptive, exact, box_k), n_slots, max_block).state_bytes();
}

int st_create(StBank** out, const RgCtx& c, int32_t n_slots, int32_t channels, int64_t max_block, bool ns, int32_t lookahead,
              const StAdaptive* ad, bool exact, std::string* err, int32_t box_k) {
  if (box_k && (!ns || ad || c.stationary || (c.W & 1) || box_k > SG_STREAM_MAX_LOOKAHEAD)) {
    *err = "sg_stream_create_ex: a bank of TorchGate's gate needs a non-stationary handle, an even win_length and 1 <= n_movemean <= 4096";
    return SG_E_INVALID;
  }
  if (ad && !c.stationary) { *err = "sg_stream_create_adaptive: the handle is not stationary"; return SG_E_INVALID; }
  if (ad && !(ad->forget > 0.0 && ad->forget <= 1.0)) {
    char m[120];
    snprintf(m, sizeof m, "sg_stream_create_adaptive: forget must lie in (0, 1], got %g", ad->forget);
    *err = m;
    return SG_E_INVALID;
  }
  if (ad && ad->learn_frames == 0) {
    *err = "sg_stream_create_adaptive: learn_frames must be at least 1 (or negative: unlimited), got 0";
    return SG_E_INVALID;
  }
  if (!tile_geom_ok(c.N)) { *err = "sg_stream_create: n_fft must be a power of two from 256 to 4096"; return SG_E_UNSUPPORTED; }
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
  b->exact = exact ? 1 : 0;
  if (box_k) {   // the lookahead is the part of the moving mean ahead of the frame: st_make_geo_box's
    b->box = 1;
    b->K = box_k;
    b->Lb = (box_k - 1) / 2;
    b->L = box_k - 1 - b->Lb;
    // the bank's frames are [t H - W / 2, t H - W / 2 + W) with the window at the start of the n_fft frame; the handle of
    // variant T centres the window and extends by n_fft / 2: the same samples, another phase
    b->c.padL = c.W / 2;
  }
  if (ad) {
    b->ad = 1;
    b->lam = ad->forget;
    b->learn = ad->learn_frames < 0 ? -1 : ad->learn_frames;
  }
  const StLayout y = st_layout(st_geo(b), n_slots, max_block);
  if (ns && (y.RC > INT32_MAX || y.RF > INT32_MAX || y.RB > INT32_MAX)) {
    char m[200];
    snprintf(m, sizeof m, "sg_stream_create_nonstationary: max_block = %lld with lookahead_frames = %d needs rings deeper than 2^31",
             (long long)max_block, b->L);
    *err = m;
    delete b;
    return SG_E_INVALID;
  }
  b->RC = (int)y.RC;
  b->RB = (int)y.RB_ring;
  b->RF = (int)y.RF;
  b->wpr = (c.F + 63) / 64;
  b->slots.assign(n_slots, StSlot());
  if (ns || ad)
    for (auto& sl : b->slots) sl.has_thr = true;   // a non-stationary or adaptive stream needs no noise profile
  // every buffer of the layout that this kind of bank has (the state that a fresh stream reads before writing it: zeroed)
  const struct { host::DevBuf& buf; int64_t bytes; bool zero; } bufs[] = {
      {b->ring, y.ring, false}, {b->carry, y.carry, false}, {b->fst, y.fst, true},     {b->fa, y.fa, false},
      {b->mk, y.mk, false},     {b->rmax, y.rmax, true},    {b->bits, y.bits_alloc, false}, {b->nst, y.nst, true},
      {b->thr, y.thr, true},    {b->T2, y.T2, true},        {b->stage, y.stage, true}, {b->slot_list, y.slot_list, true},
      {b->tabs, y.tabs, false}, {b->ws, y.ws, false}};
  bool ok = true;
  for (const auto& q : bufs) {
    if (!q.bytes) continue;
    if (hipMalloc(&q.buf.p, (size_t)q.bytes) != hipSuccess) { q.buf.p = nullptr; ok = false; break; }
    q.buf.bytes = (size_t)q.bytes;
    if (q.zero && hipMemset(q.buf.p, 0, (size_t)q.bytes) != hipSuccess) { ok = false; break; }
  }
  if (ok && b->box && c.W < c.n) {
    const size_t nb = (size_t)c.n * 8;
    ok = hipMalloc(&b->wleft.p, nb) == hipSuccess;
    if (ok) b->wleft.bytes = nb;
    else b->wleft.p = nullptr;
    ok = ok && hipMemset(b->wleft.p, 0, nb) == hipSuccess &&
         hipMemcpy(b->wleft.p, c.wfull64 + (c.n - c.W) / 2, (size_t)c.W * 8, hipMemcpyDeviceToDevice) == hipSuccess;
    if (ok) b->c.wfull64 = b->wleft.as<double>();
  }
  if (!ok) {
    char m[200];
    snprintf(m, sizeof m, "sg_stream_create: device allocation failed (the bank's state is %lld bytes)", (long long)y.state_bytes());
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
  if (b->ad) { *err = "sg_stream_set_threshold: an adaptive bank learns its threshold from the stream"; return SG_E_INVALID; }
  if (n > b->n_slots) { *err = "sg_stream_set_threshold: more slots listed than the bank has"; return SG_E_INVALID; }
  if (n == 0) return SG_OK;
  const double* src = thresh_dev;
  if (thresh_host) {
    if (hipMemcpyAsync(b->stage.p, thresh_host, (size_t)b->c.F * 8, hipMemcpyHostToDevice, st) != hipSuccess) {
      *err = "sg_stream_set_threshold: threshold upload failed";
      return SG_E_HIP;
    }
    src = b->stage.as<double>();
  }
  if (hipMemcpyAsync(b->slot_list.p, slots, (size_t)n * 4, hipMemcpyHostToDevice, st) != hipSuccess) {
    *err = "sg_stream_set_threshold: slot list upload failed";
    return SG_E_HIP;
  }
  hipLaunchKernelGGL(k_st_thresh, dim3(n), dim3(64), 0, st, src, b->slot_list.as<int32_t>(), b->thr.as<double>(), b->T2.as<double>(), b->c.F,
                     b->c.FS, b->c.mag_scale);
  if (hipGetLastError() != hipSuccess) { *err = "sg_stream_set_threshold: launch failed"; return SG_E_HIP; }
  for (int32_t i = 0; i < n; ++i) b->slots[slots[i]].has_thr = true;
  return SG_OK;
}

int st_set_filterbank(StBank* b, const float* fb_host, int32_t n_filters, std::string* err) {
  if (!fb_host || n_filters < 1 || n_filters > FEAT_MAX_FILTERS) {
    char m[120];
    snprintf(m, sizeof m, "sg_stream_set_filterbank: bad argument (1 <= n_filters <= %d)", FEAT_MAX_FILTERS);
    *err = m;
    return SG_E_INVALID;
  }
  const int F = b->c.F, M = n_filters;
  // one host image of the four tables, each part 256-byte aligned: fb, fbT, khull, mhull
  const size_t fbb = align256((size_t)F * M * 4), khb = align256((size_t)M * 8), mhb = align256((size_t)F * 8);
  std::vector<char> host(2 * fbb + khb + mhb, 0);
  memcpy(host.data(), fb_host, (size_t)F * M * 4);
  if (!feat_tables(fb_host, F, M, (float*)(host.data() + fbb), (int32_t*)(host.data() + 2 * fbb),
                   (int32_t*)(host.data() + 2 * fbb + khb))) {
    *err = "sg_stream_set_filterbank: the filterbank has a non-finite entry";
    return SG_E_INVALID;
  }
  host::DevBuf dev;   // (a refused filterbank: freed on return, the earlier one stays)
  if (hipMalloc(&dev.p, host.size()) != hipSuccess) { dev.p = nullptr; *err = "sg_stream_set_filterbank: device allocation failed"; return SG_E_NOMEM; }
  dev.bytes = host.size();
  if (hipMemcpy(dev.p, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
    *err = "sg_stream_set_filterbank: table upload failed";
    return SG_E_HIP;
  }
  // launches of an earlier step may still read the tables about to be freed
  if (b->fbank.p && hipDeviceSynchronize() != hipSuccess) {
    *err = "sg_stream_set_filterbank: hipDeviceSynchronize failed";
    return SG_E_HIP;
  }
  b->fbank.take(dev);
  char* d = b->fbank.as<char>();
  b->fb = FeatBank{(const float*)d, (const float*)(d + fbb), (const int2*)(d + 2 * fbb), (const int2*)(d + 2 * fbb + khb), M};
  return SG_OK;
}

int st_reset(StBank* b, const int32_t* slots, int32_t n, hipStream_t st, std::string* err) {
  int rc = check_slots(b, slots, n, "sg_stream_reset", err);
  if (rc) return rc;
  for (int32_t i = 0; i < n; ++i) {
    // (the ring, the bit rows and the carry need no clearing: a fresh stream reads none of them before it writes them)
    // (nor does the forward state of a non-stationary unit: frame 0 seeds it)
    if (!b->ns &&
        hipMemsetAsync(b->rmax.as<double>() + (size_t)slots[i] * b->C * b->c.FS, 0, (size_t)b->C * b->c.FS * 8, st) != hipSuccess) {
      *err = "sg_stream_reset: hipMemsetAsync failed";
      return SG_E_HIP;
    }
    if (b->ad &&
        hipMemsetAsync(b->nst.as<double>() + (size_t)slots[i] * b->C * 3 * b->c.FS, 0, (size_t)b->C * 3 * b->c.FS * 8, st) != hipSuccess) {
      *err = "sg_stream_reset: hipMemsetAsync failed";
      return SG_E_HIP;
    }
    const bool thr = b->slots[slots[i]].has_thr;
    b->slots[slots[i]] = StSlot();
    b->slots[slots[i]].has_thr = thr;
  }
  return SG_OK;
}

int st_noise_profile(StBank* b, int32_t slot, double* thresh_host, hipStream_t st, std::string* err) {
  if (!b->ad) { *err = "sg_stream_noise_profile: the bank is not adaptive (its profile is the one it was given)"; return SG_E_INVALID; }
  if (slot < 0 || slot >= b->n_slots) {
    char m[120];
    snprintf(m, sizeof m, "sg_stream_noise_profile: unknown slot %d (the bank has %d)", slot, b->n_slots);
    *err = m;
    return SG_E_INVALID;
  }
  const int FS = b->c.FS, F = b->c.F;
  std::vector<double> host((size_t)b->C * 3 * FS);
  if (hipMemcpyAsync(host.data(), b->nst.as<double>() + (size_t)slot * b->C * 3 * FS, host.size() * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    *err = "sg_stream_noise_profile: copy of the statistics failed";
    return SG_E_HIP;
  }
  // k_sa_decide's threshold after the unit's last decided frame; Wn = 0 (no frame yet): 0 / 0 = NaN
  for (int ch = 0; ch < b->C; ++ch) {
    const double* s = host.data() + (size_t)ch * 3 * FS;
    for (int f = 0; f < F; ++f) thresh_host[(size_t)ch * F + f] = s[FS + f] + b->c.n_std * std::sqrt(s[2 * FS + f] / s[f]);
  }
  return SG_OK;
}

int64_t st_bank_emitted(const StBank* b, int64_t n) { return st_counters_at(st_geo(b), n).E; }

int64_t st_bank_frames(const StBank* b, int64_t n) { return st_counters_at(st_geo(b), n).ta + 1; }

int st_counters(const StBank* b, int32_t slot, int64_t* n, int64_t* emitted, std::string* err) {
  if (slot < 0 || slot >= b->n_slots) { *err = "sg_stream_counters: unknown slot"; return SG_E_INVALID; }
  *n = b->slots[slot].n;
  *emitted = st_counters_at(st_geo(b), *n).E;
  return SG_OK;
}

// A step: check (st_check_step), plan (st_plan_step: both stream_plan.hpp's, host arithmetic on plain data), the tables to
// the device, four launches, then the slots' new state.
int st_push(StBank* b, const void* in_dev, int in_dtype, void* out_dev, int out_dtype, const sg_stream_rec* recs,
            int32_t n_recs, hipStream_t st, std::string* err, const StSpecOut* so, const StFeatOut* fo) {
  const RgCtx& c = b->c;
  const StGeo g = st_geo(b);
  const char* who = st_step_name(so, fo);
  int rc = so ? box_refuses(b, who, "the spectrum would need torch.stft's phase and scale", err) : SG_OK;
  if (rc) return rc;
  if ((rc = st_check_step(g, b->max_block, b->fb.M, b->slots, in_dtype, out_dtype, recs, n_recs, so, fo, err))) return rc;
  const StStep P = st_plan_step(g, b->slots, recs, n_recs, so, fo);
  // ---- tables and scratch
  const size_t ub = align256(P.units.size() * sizeof(StUnit)), tb = align256(P.tl.tiles.size() * sizeof(Tile));
  // (one optional third table: the spectrum step's or the feature step's)
  const void* third = fo ? (const void*)P.feats.data() : (const void*)P.specs.data();
  const size_t third_bytes = fo ? P.feats.size() * sizeof(StFeatUnit) : P.specs.size() * sizeof(StSpec);
  const size_t sb = align256(third_bytes);
  if ((rc = grow_device_buffer(b->tabs, ub + tb + sb, st, who, "table", err))) return rc;
  const bool ex = b->exact != 0, ns = b->ns != 0;
  const size_t Rb = align256((size_t)P.mrows * c.FS * (ex && ns ? 8 : 4)), Sb = align256((size_t)P.sframes * c.n * (ex ? 8 : 4));
  if ((rc = grow_device_buffer(b->ws, Rb + Sb, st, who, "workspace", err))) return rc;
  if (upload_tables(b->tabs.p, st, {{P.units.data(), P.units.size() * sizeof(StUnit), ub},
                                    {P.tl.tiles.data(), P.tl.tiles.size() * sizeof(Tile), tb},
                                    {third, third_bytes, sb}}) != hipSuccess) {
    *err = std::string(who) + ": table upload failed";
    return SG_E_HIP;
  }
  char* tabs = b->tabs.as<char>();
  StArgs A{};
  A.x = in_dev; A.in_dtype = in_dtype; A.out = out_dev; A.out_dtype = out_dtype;
  A.units = (const StUnit*)tabs;
  A.tiles = (const Tile*)(tabs + ub);
  A.t_dec = P.t_dec; A.n_dec = P.n_dec; A.t_fs = P.t_fs; A.n_fs = P.n_fs;
  A.t_ap = P.t_ap; A.n_ap = P.n_ap; A.t_fin = P.t_fin; A.n_fin = P.n_fin;
  A.ring = b->ring.as<double>(); A.bits = b->bits.as<unsigned long long>(); A.rmax = b->rmax.as<double>();
  A.carry = b->carry.as<double>(); A.thr = b->thr.as<double>(); A.T2 = b->T2.as<double>();
  A.R = b->ws.p; A.seg = b->ws.as<char>() + Rb;
  A.RC = b->RC; A.RB = b->RB;
  A.fst = b->fst.as<double>(); A.fa = b->fa.as<double>(); A.mk = b->mk.p; A.RF = b->RF; A.L = b->L;
  A.nst = b->nst.as<double>(); A.lam = b->lam; A.learn = b->learn;
  A.K = b->K; A.Lb = b->Lb;
  A.c = fill_consts(c);
  if (so) {
    A.spec = so->spec; A.smask = so->mask; A.spec_dtype = so->dtype;
    A.sp = (const StSpec*)(tabs + ub + tb);
  }
  StFeat Q{};
  if (fo) {
    Q.bank = b->fb;
    Q.feat = fo->feat; Q.fmask = fo->mask; Q.dtype = fo->dtype;
    Q.fu = (const StFeatUnit*)(tabs + ub + tb);
    Q.eps = fo->eps; Q.scale = fo->scale == 0.0 ? c.mag_scale : fo->scale;
    Q.power = fo->power; Q.take_log = fo->take_log ? 1 : 0;
  }
  // ---- the step: the same four launches whatever was pushed.  A kernel's flags (EX: exact bank, NS: non-stationary
  // bank) are template arguments, chosen by dispatch_flag(s); only the instantiations named here exist
  hipError_t e = hipSuccess;
  {
    Prof pr(c, SG_STAGE_RG_DECIDE, st);
    e = dispatch_N(c.N, [&](auto n) {
      constexpr int N = decltype(n)::value;
      if (b->ad) return launch_tile_kernel<N>(k_sa_decide<N>, A.n_dec, st, A);
      if (b->box) return dispatch_flag(ex, [&](auto EX) { return launch_tile_kernel<N>(k_sb_decide<N, decltype(EX)::value>, A.n_dec, st, A); });
      if (ns) return dispatch_flag(ex, [&](auto EX) { return launch_tile_kernel<N>(k_sn_decide<N, decltype(EX)::value>, A.n_dec, st, A); });
      return launch_tile_kernel<N>(k_st_decide<N>, A.n_dec, st, A);
    });
  }
  if (e == hipSuccess) {
    Prof pr(c, SG_STAGE_RG_FSMOOTH, st);
    e = ns ? dispatch_flag(ex, [&](auto EX) { return launch_flat_kernel(k_st_fsmooth<true, decltype(EX)::value>, A.n_fs, 256, st, A); })
           : launch_flat_kernel(k_st_fsmooth<false, false>, A.n_fs, 256, st, A);
  }
  if (e == hipSuccess) {
    Prof pr(c, SG_STAGE_RG_APPLY, st);
    e = dispatch_N(c.N, [&](auto n) {
      constexpr int N = decltype(n)::value;
      if (b->box) return dispatch_flag(ex, [&](auto EX) {   // (no spectrum step on a box bank: refused above)
        if (fo) return launch_feat_kernel<N>(k_st_feat<N, true, decltype(EX)::value, true>, A.n_ap, st, A, Q);
        return launch_tile_kernel<N>(k_st_apply<N, true, decltype(EX)::value, false, true>, A.n_ap, st, A);
      });
      if (fo) return dispatch_flags(ex, ns, [&](auto EX, auto NS) {
        return launch_feat_kernel<N>(k_st_feat<N, decltype(NS)::value, decltype(EX)::value>, A.n_ap, st, A, Q);
      });
      if (so) return dispatch_flags(ex, ns, [&](auto EX, auto NS) {
        return launch_tile_kernel<N>(k_st_apply<N, decltype(NS)::value, decltype(EX)::value, true>, A.n_ap, st, A);
      });
      return dispatch_flags(ex, ns, [&](auto EX, auto NS) {
        return launch_tile_kernel<N>(k_st_apply<N, decltype(NS)::value, decltype(EX)::value>, A.n_ap, st, A);
      });
    });
  }
  if (e == hipSuccess) {
    Prof pr(c, SG_STAGE_RG_OLA, st);
    e = dispatch_flag(ex, [&](auto EX) { return launch_flat_kernel(k_st_finish<decltype(EX)::value>, A.n_fin, 256, st, A); });
  }
  if (e != hipSuccess) {
    *err = std::string(who) + ": launch failed: " + hipGetErrorString(e);
    return SG_E_HIP;
  }
  for (int32_t i = 0; i < n_recs; ++i) b->slots[recs[i].slot] = P.after[i];
  return SG_OK;
}

// ---- state transfer ------------------------------------------------------------------------------------------------
namespace {
int64_t st_payload_words(const StBank* b, int64_t n) { return st_payload_words(st_geo(b), n); }

// the fields of one slot in payload order, word 0 of the payload at `blob`; the tiles of each
void st_fields(const StBank* b, int32_t slot, int64_t n, int par, int64_t blob, std::vector<StXField>* fields, TileList* tl) {
  const StGeo g = st_geo(b);
  const StLive v = st_live(g, n);
  const int64_t mkw = mk_words(g);
  const RgCtx& c = b->c;
  const int64_t FS = c.FS;
  auto field = [&](void* dev, int64_t first, int64_t R, int64_t rw, int64_t rows) {
    if (rows > 0) {
      fields->push_back(StXField{(unsigned long long*)dev, blob, (uint32_t)(first % R), (uint32_t)R, (uint32_t)rw, 0u});
      tl->push_ranges((int64_t)fields->size() - 1, 0, rows * rw, XW);
    }
    blob += rows * rw;
  };
  if (g.fixed) {
    field(b->thr.as<double>() + (int64_t)slot * FS, 0, 1, FS, 1);
    field(b->T2.as<double>() + (int64_t)slot * FS, 0, 1, FS, 1);
  }
  for (int ch = 0; ch < b->C; ++ch) {
    const int64_t u = (int64_t)slot * b->C + ch;
    field(b->ring.as<double>() + u * b->RC, v.ring_lo, b->RC, 1, v.ring_n);
    field(b->carry.as<double>() + (u * 2 + par) * c.W, v.E, c.W, 1, v.car_n);
    if (b->ns) {
      field(b->fst.as<double>() + u * FS, 0, 1, FS, 1);
      field(b->fa.as<double>() + u * b->RF * 2 * FS, v.ts + 1, b->RF, 2 * FS, v.fa_rows);
      field(b->mk.as<unsigned long long>() + u * b->RB * mkw, v.row_lo, b->RB, mkw, v.mk_rows);
    } else {
      field(b->rmax.as<double>() + u * FS, 0, 1, FS, 1);
      field(b->bits.as<unsigned long long>() + u * b->RB * b->wpr, v.row_lo, b->RB, b->wpr, v.bit_rows);
    }
    if (b->ad) field(b->nst.as<double>() + u * 3 * FS, 0, 1, 3 * FS, 1);
  }
}

void st_sign(const StBank* b, sg_stream_head* hd) {
  hd->magic = SG_STREAM_HEAD_MAGIC;
  hd->version = SG_STREAM_HEAD_VERSION;
  hd->channels = b->C;
  hd->kind = b->ad ? SG_STREAM_ADAPTIVE : b->ns ? SG_STREAM_NONSTATIONARY : SG_STREAM_FIXED;
  hd->lookahead_frames = b->L;
  hd->exact = b->exact;
  hd->noise_forget = b->lam;
  hd->noise_learn_frames = b->learn;
}

// the first signature field of `hd` that differs from the bank's (`own`), or null
const char* st_sig_diff(const sg_stream_head& hd, const sg_stream_head& own) {
#define SG_SIG(f) if (!(hd.f == own.f)) return #f;
  SG_SIG(n_fft) SG_SIG(win_length) SG_SIG(hop_length) SG_SIG(channels) SG_SIG(kind) SG_SIG(n_grad_freq) SG_SIG(n_grad_time)
  SG_SIG(smooth_mask) SG_SIG(lookahead_frames) SG_SIG(exact) SG_SIG(prop_decrease) SG_SIG(n_std_thresh) SG_SIG(top_db)
  SG_SIG(iir_b) SG_SIG(nonstat_thresh) SG_SIG(nonstat_slope) SG_SIG(noise_forget) SG_SIG(noise_learn_frames)
#undef SG_SIG
  return nullptr;
}

int st_check_transfer(const StBank* b, const int32_t* slots, int32_t n, const void* blob_dev, const int64_t* offsets,
                      const void* heads, const char* who, std::string* err) {
  int rc = check_slots(b, slots, n, who, err);
  if (rc) return rc;
  char m[200];
  if (n > 0 && (!blob_dev || !offsets || !heads || ((uintptr_t)blob_dev & 255))) {
    *err = std::string(who) + ": blob_dev (256-byte aligned), offsets and heads are needed";
    return SG_E_INVALID;
  }
  std::vector<char> seen(b->n_slots, 0);
  for (int32_t i = 0; i < n; ++i) {
    if (seen[slots[i]]) {
      snprintf(m, sizeof m, "%s: slot %d appears twice in one call", who, slots[i]);
      *err = m;
      return SG_E_INVALID;
    }
    seen[slots[i]] = 1;
    if (offsets[i] < 0 || (offsets[i] & 255)) {
      snprintf(m, sizeof m, "%s: slot %d: payload offset %lld is not a multiple of 256", who, slots[i], (long long)offsets[i]);
      *err = m;
      return SG_E_INVALID;
    }
  }
  return SG_OK;
}

// fields + tiles to the table buffer, then the one launch
template <class K>
int st_transfer(StBank* b, K kernel, int stage, void* blob_dev, const std::vector<StXField>& fields, const TileList& tl,
                hipStream_t st, const char* who, std::string* err) {
  const size_t fb = align256(fields.size() * sizeof(StXField)), tb = align256(tl.tiles.size() * sizeof(Tile));
  int rc = grow_device_buffer(b->tabs, fb + tb, st, who, "table", err);
  if (rc) return rc;
  if (upload_tables(b->tabs.p, st, {{fields.data(), fields.size() * sizeof(StXField), fb},
                                  {tl.tiles.data(), tl.tiles.size() * sizeof(Tile), tb}}) != hipSuccess) {
    *err = std::string(who) + ": table upload failed";
    return SG_E_HIP;
  }
  StXArgs A{};
  A.blob = (unsigned long long*)blob_dev;
  A.fields = b->tabs.as<const StXField>();
  A.tiles = (const Tile*)(b->tabs.as<char>() + fb);
  A.n_tiles = tl.size();
  hipError_t e;
  { Prof pr(b->c, stage, st); e = launch_flat_kernel(kernel, A.n_tiles, 256, st, A); }
  if (e != hipSuccess) {
    *err = std::string(who) + ": launch failed: " + hipGetErrorString(e);
    return SG_E_HIP;
  }
  return SG_OK;
}
}  // namespace

int st_head_bytes(const sg_stream_head& hd, int64_t* bytes) {
  const bool ns = hd.kind == SG_STREAM_NONSTATIONARY;
  if (hd.n < 0 || !tile_geom_ok(hd.n_fft / 2) || (hd.n_fft & 1) || hd.win_length < 2 || hd.win_length > hd.n_fft ||
      hd.hop_length < 1 || hd.channels < 1 || hd.n_grad_time < 0 ||
      (hd.kind != SG_STREAM_FIXED && !ns && hd.kind != SG_STREAM_ADAPTIVE) ||
      (ns && (hd.lookahead_frames < 0 || hd.lookahead_frames > SG_STREAM_MAX_LOOKAHEAD)))
    return SG_E_INVALID;
  *bytes = 8 * st_payload_words(st_geo(hd), hd.n);
  return SG_OK;
}

int st_export_bytes(const StBank* b, int32_t slot, int64_t* bytes, std::string* err) {
  const char* no_head = "a kind-1 header cannot tell the two non-stationary gates apart";
  if (int rc = box_refuses(b, "sg_stream_export_bytes", no_head, err)) return rc;
  if (slot < 0 || slot >= b->n_slots) { *err = "sg_stream_export_bytes: unknown slot"; return SG_E_INVALID; }
  *bytes = 8 * st_payload_words(b, b->slots[slot].n);
  return SG_OK;
}

int st_export(StBank* b, const int32_t* slots, int32_t n, void* blob_dev, const int64_t* offsets, const sg_stream_head& sig,
              sg_stream_head* heads, hipStream_t st, std::string* err) {
  const char* who = "sg_stream_export";
  int rc = box_refuses(b, who, "a kind-1 header cannot tell the two non-stationary gates apart", err);
  if (rc) return rc;
  rc = st_check_transfer(b, slots, n, blob_dev, offsets, heads, who, err);
  if (rc) return rc;
  if (n == 0) return SG_OK;
  // (payloads that overlap would make two workgroups write the same words)
  std::vector<std::pair<int64_t, int64_t>> spans;
  for (int32_t i = 0; i < n; ++i) spans.push_back({offsets[i], offsets[i] + 8 * st_payload_words(b, b->slots[slots[i]].n)});
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second) { *err = "sg_stream_export: payloads overlap"; return SG_E_INVALID; }
  std::vector<StXField> fields;
  TileList tl;
  for (int32_t i = 0; i < n; ++i) {
    const StSlot& S = b->slots[slots[i]];
    sg_stream_head hd = sig;
    st_sign(b, &hd);
    const StCounters k = st_counters_at(st_geo(b), S.n);
    hd.n = S.n; hd.td = k.td; hd.ts = k.ts; hd.ta = k.ta; hd.E = k.E;
    hd.par = S.par;
    hd.has_thr = S.has_thr ? 1 : 0;
    hd.payload_bytes = 8 * st_payload_words(b, S.n);
    hd.client0 = hd.client1 = hd.client2 = hd.client3 = 0;
    heads[i] = hd;
    st_fields(b, slots[i], S.n, S.par, offsets[i] / 8, &fields, &tl);
  }
  return st_transfer(b, k_st_export, SG_STAGE_ST_EXPORT, blob_dev, fields, tl, st, who, err);
}

int st_import(StBank* b, const int32_t* slots, int32_t n, const void* blob_dev, const int64_t* offsets, const sg_stream_head& sig,
              const sg_stream_head* heads, hipStream_t st, std::string* err) {
  const char* who = "sg_stream_import";
  int rc = box_refuses(b, who, "a kind-1 header cannot tell the two non-stationary gates apart", err);
  if (rc) return rc;
  rc = st_check_transfer(b, slots, n, blob_dev, offsets, heads, who, err);
  if (rc) return rc;
  if (n == 0) return SG_OK;
  char m[200];
  sg_stream_head own = sig;
  st_sign(b, &own);
  for (int32_t i = 0; i < n; ++i) {
    const sg_stream_head& hd = heads[i];
    if (hd.magic != SG_STREAM_HEAD_MAGIC || hd.version != SG_STREAM_HEAD_VERSION) {
      snprintf(m, sizeof m, "sg_stream_import: slot %d: not a stream state of this version (magic %#x, version %d)", slots[i],
               (unsigned)hd.magic, hd.version);
      *err = m;
      return SG_E_INVALID;
    }
    if (const char* f = st_sig_diff(hd, own)) {
      snprintf(m, sizeof m, "sg_stream_import: slot %d: the state comes from a different kind of bank: %s differs", slots[i], f);
      *err = m;
      return SG_E_INVALID;
    }
    // (the sizes of every write below follow from n alone; the other counters have to be the ones n gives)
    const StCounters v = hd.n >= 0 ? st_counters_at(st_geo(b), hd.n) : StCounters{};
    if (hd.n < 0 || hd.td != v.td || hd.ts != v.ts || hd.ta != v.ta || hd.E != v.E || (hd.par != 0 && hd.par != 1) ||
        hd.payload_bytes != 8 * st_payload_words(b, hd.n)) {
      snprintf(m, sizeof m, "sg_stream_import: slot %d: the state's counters or payload size do not fit together", slots[i]);
      *err = m;
      return SG_E_INVALID;
    }
  }
  std::vector<StXField> fields;
  TileList tl;
  for (int32_t i = 0; i < n; ++i) st_fields(b, slots[i], heads[i].n, heads[i].par, offsets[i] / 8, &fields, &tl);
  rc = st_transfer(b, k_st_import, SG_STAGE_ST_IMPORT, const_cast<void*>(blob_dev), fields, tl, st, who, err);
  if (rc) return rc;
  for (int32_t i = 0; i < n; ++i) {
    const sg_stream_head& hd = heads[i];
    StSlot& S = b->slots[slots[i]];
    S.n = hd.n;   // (td, ts, ta, E: checked above to be the ones n gives)
    S.par = hd.par;
    S.has_thr = b->thr.p ? hd.has_thr != 0 : true;
  }
  return SG_OK;
}
}  // namespace sg
