// Ragged batches of recordings (sg_process_clips): tables, kernels and the host side of the batched path.  See
// ragged.hpp and DESIGN section 11.
//
// Every kernel reads a tile table: tile i = {index (unit or noise source), first, end} -- frames for the transform
// kernels, rows for the frequency smoothing, bands for the recurrence, output samples for the overlap-add.  What a frame
// goes through is tile_core.hpp's, shared with rows.hip and stream.hip; this file holds what only the clips have: units
// (one channel of one chunk of one clip) with their own window and frame ranges, the channel mean of a noise source, the
// forward-backward recurrence.  Nothing waits on another workgroup, and every cross-frame reduction is either exact
// (maxima as integer atomics on the bit patterns of non-negative doubles) or serial within one unit / one noise source.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tile_core.hpp"
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

struct RgArgs {
  const void* x; int in_dtype;
  const void* xn; int noise_dtype;
  void* out; int out_dtype;
  const RgUnit* units;
  const RgNoise* noises;
  const Tile* tiles;             // all tile lists, back to back
  int64_t t_np, n_np;            // noise power tiles (first, count)
  int64_t t_nf, n_nf;            // noise final tiles (noise, band block)
  int64_t t_dec, n_dec;          // data-frame tiles
  int64_t t_iir, n_iir;          // recurrence tiles (unit, band block)
  int64_t t_fs, n_fs;            // frequency smoothing tiles (unit, rows)
  int64_t t_ap, n_ap;            // live-frame tiles
  int64_t t_ola, n_ola;          // output tiles (unit, positions)
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
  TileConsts c;
};

// window * frame t of the unit (unit samples [t H - padL, t H - padL + n)), forward transform in place.  Samples outside
// the window or outside the clip read as 0 (SpectralGate._read_chunk).
template <int N>
__device__ __forceinline__ void rg_unit_fft(const RgArgs& A, const RgUnit& U, int64_t t, cx<double>* buf,
                                            const cx<double>* tw, int lane) {
  const int64_t s0 = t * A.c.H - A.c.padL;
  frame_fft<N>(buf, tw, lane, [&](int jj) -> double {
    const int64_t s = s0 + jj;
    const int64_t g = U.win0 + s;
    const double v = (s >= 0 && s < U.Lp && g >= 0 && g < U.n) ? load_sample(A.x, A.in_dtype, U.x_off + g) : 0.0;
    return v * A.c.wfull[jj];
  });
}

// ---- stationary: noise statistics ----------------------------------------------------------------------------------
// power of every frame of every noise source: channel mean (sequential float64 sum / C, k_channel_mean), window, transform
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_rg_noise_power(RgArgs A) {
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_np) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_np + blockIdx.x];
  const RgNoise S = A.noises[tl.idx];
  const void* src = S.in_x ? A.x : A.xn;
  const int dt = S.in_x ? A.in_dtype : A.noise_dtype;
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    const int64_t s0 = t * A.c.H - A.c.padL;
    frame_fft<N>(buf, tw, lane, [&](int jj) -> double {
      const int64_t s = s0 + jj;
      double acc = 0.0;
      if (s >= 0 && s < S.n) {
        for (int c = 0; c < S.C; ++c) acc += load_sample(src, dt, S.off + c * S.stride + s);
        acc = acc / (double)S.C;
      }
      return acc * A.c.wfull[jj];
    });
    double* row = A.Pn + (S.prow + t) * A.c.FS;
    for (int k = lane; k <= N; k += NT) row[k] = bin_power<N>(buf, tw, k);
    team_sync<SY>();
  }
}

// one thread per (noise source, band): the threshold, and the compare constant of the threshold alone (k_t2_rows without
// the floor: the floor is a per-(unit, band) override, k_rg_fsmooth)
__global__ __launch_bounds__(64) void k_rg_noise_final(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_nf) return;
  const Tile tl = A.tiles[A.t_nf + blockIdx.x];
  const int f = (int)tl.a + (int)threadIdx.x;
  if (f >= A.c.F) return;
  const RgNoise S = A.noises[tl.idx];
  const double th = noise_band_threshold(A.c, A.Pn + S.prow * A.c.FS + f, S.T);
  A.T2n[(int64_t)tl.idx * A.c.FS + f] = thresh_to_t2(th, A.c.mag_scale);
  A.thr_all[S.gidx * A.c.FS + f] = th;
}

// ---- per data frame: decision bits + band maxima (stationary) or magnitudes (non-stationary) ------------------------
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_rg_decide(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_dec) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_dec + blockIdx.x];
  const RgUnit U = A.units[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  double vmax[tile_bins<N>()];
#pragma unroll
  for (int m = 0; m < tile_bins<N>(); ++m) vmax[m] = 0.0;
  const double* T2 = A.T2n + (int64_t)U.noise * A.c.FS;
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rg_unit_fft<N>(A, U, t, buf, tw, lane);
    const int64_t row = U.drow + (t - U.d0);
    decide_frame<N>(A.c, buf, tw, lane, T2, A.bits + row * A.c.wpr, A.mag + row * A.c.FS, vmax);
    team_sync<tile_sy<N>()>();
  }
  if (A.c.stationary) merge_band_maxima<N>(A.pmax + (int64_t)tl.idx * A.c.FS, lane, vmax);
}

// ---- non-stationary: filtfilt(padtype=None) one-pole over the unit's frames + sigmoid (k_iir_sigmoid) -------------
// one thread per (unit, band); frames outside [d0, d1) have magnitude 0 and are stepped through all the same
__global__ __launch_bounds__(64) void k_rg_iir(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_iir) return;
  const Tile tl = A.tiles[A.t_iir + blockIdx.x];
  const int f = (int)tl.a + (int)threadIdx.x;
  if (f >= A.c.F) return;
  const int FS = A.c.FS;
  const RgUnit U = A.units[tl.idx];
  auto mag_at = [&](int64_t t) -> double {
    return (t >= U.d0 && t < U.d1) ? (double)A.mag[(U.drow + t - U.d0) * FS + f] : 0.0;
  };
  const double b = A.c.iir_b, c = 1.0 - A.c.iir_b;
  double s = mag_at(0);
  for (int64_t t = 0; t < U.T; ++t) {
    s = b * mag_at(t) + c * s;
    if (t >= U.d0) A.fw[(U.frow + t - U.d0) * FS + f] = (float)s;
    // (before d0 every magnitude is 0 and so is s: the forward value is 0 there)
  }
  const double fprev = s;
  for (int64_t t = U.T - 1; t >= 0; --t) {
    double fwv = t >= U.d0 ? (double)A.fw[(U.frow + t - U.d0) * FS + f] : 0.0;
    if (t == U.T - 1) fwv = fprev;
    s = b * fwv + c * s;
    if (t >= U.r0 && t < U.r1) A.sig[(U.mrow + t - U.r0) * FS + f] = sigmoid_ratio(mag_at(t), s, (float)A.c.nthresh, (float)A.c.slope);
  }
}

// ---- mask smoothing along frequency (fsmooth_row) -------------------------------------------------------------------
// Stationary raw mask: the decision bit, with the -top_db floor applied per (unit, band) from the unit's band maximum
// (band_mode).  Rows outside the data frames transform to exactly 0: their bit is 0 unless the band passes everywhere.
__global__ __launch_bounds__(256) void k_rg_fsmooth(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_fs) return;
  __shared__ unsigned char mode[2112];   // band_mode per band (F <= 2049)
  const Tile tl = A.tiles[A.t_fs + blockIdx.x];
  const RgUnit U = A.units[tl.idx];
  const int FS = A.c.FS;
  if (A.c.stationary) {
    const int64_t gi = A.noises[U.noise].gidx;
    for (int f = threadIdx.x; f < A.c.F; f += blockDim.x) {
      const double pm = __longlong_as_double((long long)A.pmax[(int64_t)tl.idx * FS + f]);
      mode[f] = band_mode(pm, A.thr_all[gi * FS + f], A.T2n[(int64_t)U.noise * FS + f], A.c.mag_scale, A.c.top_db);
    }
  }
  __syncthreads();
  for (int64_t r = tl.a; r < tl.b; ++r) {
    const bool data = r >= U.d0 && r < U.d1;
    const unsigned long long* brow = A.bits + (U.drow + r - U.d0) * A.c.wpr;
    const float* srow = A.sig + (U.mrow + r - U.r0) * FS;
    fsmooth_row(A.R + (U.mrow + r - U.r0) * FS, A.c.F, A.c.nf, [&](int g) -> float {
      if (!A.c.stationary) return srow[g];
      const unsigned char md = mode[g];
      return md == 1 ? 1.f : (md == 2 ? 0.f : (data ? bit_at(brow, g) : 0.f));
    });
  }
}

// ---- live frames: time smoothing, masked multiply, inverse transform ---------------------------------------------------
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_rg_apply(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_ap + blockIdx.x];
  const RgUnit U = A.units[tl.idx];
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    rg_unit_fft<N>(A, U, t, buf, tw, lane);
    const TimeTaps tp = time_taps(t, A.c.nt, U.T);
    auto mask_at = [&](int k) -> double {
      const double K = time_smooth(A.R, A.c.FS, [&](int64_t q) { return U.mrow + q - U.r0; }, tp, t, A.c.nt, k);
      return A.c.stationary ? mask_stationary(A.c, K, tp.Et, k) : mask_nonstationary(A.c, K);
    };
    mask_and_invert<N>(buf, tw, lane, mask_at, A.c.wfull, A.seg + (U.srow + t - U.l0) * (int64_t)A.c.n);
  }
}

// ---- overlap-add of the kept samples (k_ola): out = sum seg / sum w^2; positions >= Lout are the zero tail -----------
__global__ __launch_bounds__(256) void k_rg_ola(RgArgs A) {
  if ((int64_t)blockIdx.x >= A.n_ola) return;
  const Tile tl = A.tiles[A.t_ola + blockIdx.x];
  const RgUnit U = A.units[tl.idx];
  const int64_t p = tl.a + threadIdx.x;
  if (p >= tl.b) return;
  double val = 0.0;
  if (p < U.Lout) {
    double acc, norm;
    ola_sum(A.c, A.seg, [&](int64_t t) { return U.srow + t - U.l0; }, p + A.c.padL, U.T, &acc, &norm);
    val = norm > 1e-10 ? acc / norm : acc;
  }
  store_sample(A.out, A.out_dtype, U.out_off + (p - U.k0), (float)val);
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct RgState {
  host::DevBuf ws, thr;
  int64_t last_noise = 0, last_batches = 0;
  int FS = 0;
};

void rg_free(RgState* s) { delete s; }

int64_t rg_last_batches(const RgState* s) { return s ? s->last_batches : 0; }

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
  const int64_t nch = chunked ? tile_cdiv(n, cs) : 1;
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
      U.d0 = std::max<int64_t>(0, tile_fdiv(a + c.padL - c.W, c.H) + 1);
      U.d1 = std::min<int64_t>(U.T, tile_cdiv(b + c.padL, c.H));
      if (U.d0 > U.T) U.d0 = U.T;
      if (U.d1 < U.d0) U.d1 = U.d0;
      const int64_t ke = std::min(U.k1, U.Lout);
      if (ke > U.k0) {
        int64_t lo = tile_cdiv(U.k0 + c.padL - c.n + 1, c.H);
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

struct Layout {
  size_t tabs, Pn, T2n, pmax, bits, mag, fw, sig, R, seg, total;
};
Layout layout(const RgCtx& c, int64_t n_units, int64_t n_noise, int64_t noise_rows, int64_t drows, int64_t frows,
              int64_t mrows, int64_t sframes, int64_t n_tiles) {
  Layout L{};
  const int wpr = (c.F + 63) / 64;
  size_t o = 0;
  auto take = [&](size_t b) { size_t r = o; o += align256(b); return r; };
  L.tabs = take((size_t)n_units * sizeof(RgUnit) + (size_t)n_noise * sizeof(RgNoise) + (size_t)n_tiles * sizeof(Tile));
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
    ntiles += tile_cdiv(T, FPT) + tile_cdiv(c.F, 64);
  }
  void add_clip(const RgCtx& c, const sg_clip& cl) {
    Plan P;
    plan_clip(c, c.cs, c.pad, cl, 0, P);
    for (const RgUnit& U : P.units) {
      ++nu;
      ntiles += tile_cdiv(U.d1 - U.d0, FPT) + tile_cdiv(U.r1 - U.r0, RPT) + tile_cdiv(U.l1 - U.l0, FPT) + tile_cdiv(U.k1 - U.k0, 256);
      if (!c.stationary && U.r1 > U.r0) ntiles += tile_cdiv(c.F, 64);
    }
    drows += P.drows; frows += P.frows; mrows += P.mrows; sframes += P.sframes;
  }
  Layout layout_of(const RgCtx& c) const { return layout(c, nu, nn, noise_rows, drows, frows, mrows, sframes, ntiles); }
};
}  // namespace

static bool geom_ok(const RgCtx& c, std::string* err) {
  if (!tile_geom_ok(c.N)) {
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
  if (!s || !s->thr.p || n_noise != s->last_noise) {
    *err = "sg_debug_clip_thresholds: n_noise does not match the last sg_process_clips call";
    return SG_E_STATE;
  }
  if (hipStreamSynchronize(st) != hipSuccess) { *err = "hipStreamSynchronize failed"; return SG_E_HIP; }
  std::vector<double> tmp((size_t)n_noise * s->FS);
  if (!tmp.empty() && hipMemcpy(tmp.data(), s->thr.p, tmp.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) {
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
    if (S->thr.bytes < tb) {
      if (S->thr.p) { (void)hipStreamSynchronize(st); S->thr.release(); }
      if (hipMalloc(&S->thr.p, tb) != hipSuccess) { S->thr.p = nullptr; *err = "threshold buffer allocation failed"; return SG_E_NOMEM; }
      S->thr.bytes = tb;
    }
  }
  if (max_ws <= 0) max_ws = (int64_t)4 << 30;
  // sub-batches: clips in order, greedily, under the budget (a clip that alone exceeds it is a sub-batch of its own)
  std::vector<int64_t> nrows_of(n_noise > 0 ? n_noise : 1, 0);
  for (int32_t i = 0; i < n_noise && c.stationary; ++i) nrows_of[i] = noise_frames(c, noise[i].n);
  int64_t i0 = 0;
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
    TileList tl;
    RgArgs A{};
    const int64_t nu = (int64_t)P.units.size(), nn = (int64_t)noises.size();
    A.t_np = tl.begin_stage();
    for (int64_t k = 0; k < nn; ++k) tl.push_ranges(k, 0, noises[k].T, FPT);
    A.n_np = tl.count_since(A.t_np);
    A.t_nf = tl.begin_stage();
    for (int64_t k = 0; k < nn; ++k) tl.push_ranges(k, 0, c.F, 64, false);
    A.n_nf = tl.count_since(A.t_nf);
    A.t_dec = tl.begin_stage();
    for (int64_t u = 0; u < nu; ++u) tl.push_ranges(u, P.units[u].d0, P.units[u].d1, FPT);
    A.n_dec = tl.count_since(A.t_dec);
    A.t_iir = tl.begin_stage();
    for (int64_t u = 0; u < nu && !c.stationary; ++u)
      if (P.units[u].r1 > P.units[u].r0) tl.push_ranges(u, 0, c.F, 64, false);
    A.n_iir = tl.count_since(A.t_iir);
    A.t_fs = tl.begin_stage();
    for (int64_t u = 0; u < nu; ++u) tl.push_ranges(u, P.units[u].r0, P.units[u].r1, RPT);
    A.n_fs = tl.count_since(A.t_fs);
    A.t_ap = tl.begin_stage();
    for (int64_t u = 0; u < nu; ++u) tl.push_ranges(u, P.units[u].l0, P.units[u].l1, FPT);
    A.n_ap = tl.count_since(A.t_ap);
    A.t_ola = tl.begin_stage();
    for (int64_t u = 0; u < nu; ++u) tl.push_ranges(u, P.units[u].k0, P.units[u].k1, 256);
    A.n_ola = tl.count_since(A.t_ola);
    const int64_t ntl = tl.size();
    if (nu != z.nu || nn != z.nn || noise_rows != z.noise_rows || ntl != z.ntiles || P.drows != z.drows ||
        P.frows != z.frows || P.mrows != z.mrows || P.sframes != z.sframes) {
      *err = "sg_process_clips: internal error: sub-batch tables disagree with their size estimate";
      return SG_E_STATE;
    }
    Layout L = layout(c, nu, nn, noise_rows, P.drows, P.frows, P.mrows, P.sframes, ntl);
    if ((rc = grow_device_buffer(S->ws, L.total, st, "sg_process_clips", "workspace", err))) return rc;
    char* w = S->ws.as<char>();
    const size_t ub = nu * sizeof(RgUnit), nb = nn * sizeof(RgNoise), tb = ntl * sizeof(Tile);
    if (upload_tables(w + L.tabs, st, {{P.units.data(), ub, ub}, {noises.data(), nb, nb}, {tl.tiles.data(), tb, tb}}) != hipSuccess) {
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
    A.noises = (const RgNoise*)(w + L.tabs + ub);
    A.tiles = (const Tile*)(w + L.tabs + ub + nb);
    A.Pn = (double*)(w + L.Pn); A.T2n = (double*)(w + L.T2n); A.thr_all = S->thr.as<double>();
    A.pmax = (unsigned long long*)(w + L.pmax); A.bits = (unsigned long long*)(w + L.bits);
    A.mag = (float*)(w + L.mag); A.fw = (float*)(w + L.fw); A.sig = (float*)(w + L.sig); A.R = (float*)(w + L.R);
    A.seg = (float*)(w + L.seg);
    A.c = fill_consts(c);

    hipError_t e = hipSuccess;
    if (c.stationary) {
      { Prof pr(c, SG_STAGE_RG_NOISE_POWER, st); e = dispatch_N(c.N, [&](auto n) { return launch_tile_kernel<n()>(k_rg_noise_power<n()>, A.n_np, st, A); }); }
      if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_NOISE_FINAL, st); e = launch_flat_kernel(k_rg_noise_final, A.n_nf, 64, st, A); }
    }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_DECIDE, st); e = dispatch_N(c.N, [&](auto n) { return launch_tile_kernel<n()>(k_rg_decide<n()>, A.n_dec, st, A); }); }
    if (e == hipSuccess && !c.stationary) { Prof pr(c, SG_STAGE_RG_IIR, st); e = launch_flat_kernel(k_rg_iir, A.n_iir, 64, st, A); }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_FSMOOTH, st); e = launch_flat_kernel(k_rg_fsmooth, A.n_fs, 256, st, A); }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_APPLY, st); e = dispatch_N(c.N, [&](auto n) { return launch_tile_kernel<n()>(k_rg_apply<n()>, A.n_ap, st, A); }); }
    if (e == hipSuccess) { Prof pr(c, SG_STAGE_RG_OLA, st); e = launch_flat_kernel(k_rg_ola, A.n_ola, 256, st, A); }
    if (e != hipSuccess) {
      *err = std::string("sg_process_clips: launch failed: ") + hipGetErrorString(e);
      return SG_E_HIP;
    }
    ++S->last_batches;
    i0 = i1;
  }
  return SG_OK;
}
}  // namespace sg
