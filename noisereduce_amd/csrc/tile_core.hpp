// The tile core shared by the three table-driven paths: ragged.hip (sg_process_clips), rows.hip (sg_process_rows) and
// stream.hip (sg_stream_push).  DESIGN sections 11-13.
//
// Every kernel of those paths reads a tile table (tile = {index of a unit / row / noise source, first, end}) and works
// on frames of one geometry: one wavefront per frame up to N = 512, a 256-thread team from N = 1024 on.  What a frame
// goes through -- window + forward transform, power of a bin, threshold -> compare constant, band mode of the -top_db
// floor, frequency and time smoothing of the mask, the masked inverse transform, the overlap-add span -- is written here
// ONCE, as __device__ __forceinline__ functions that take what differs per path (where a sample comes from, where a mask
// row lies) as a functor.  The host half holds the tile list, the workspace / upload / launch helpers and TileConsts.
// This header holds no __global__ kernel, so any translation unit may include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "fft_wave.hpp"
#include "geom.hpp"
#include "thresh.hpp"
#include "ragged.hpp"
#include "launch.hpp"
#include "devbuf.hpp"
#include "tile_tables.hpp"   // Tile, TileList, tile_fdiv / tile_cdiv, align256

namespace sg {

// ---- what every kernel of the three paths needs of the handle (fill_consts) -------------------------------------------
struct TileConsts {
  int n, W, H, F, FS, padL, wpr;   // n_fft, win_length, hop, bins, padded bins, zero extension, 64-bit words per bit row
  double mag_scale, top_db, n_std, prop, nthresh, slope, iir_b;
  int ddof, nf, nt, stationary;
  double ktot;                     // (nf + 1)^2 (nt + 1)^2: weight of the whole smoothing triangle
  const cx<double>* tw;            // cx<double>[N]: w_2N^k
  const double* wfull;             // window embedded in an n_fft frame
};

// ---- device side -------------------------------------------------------------------------------------------------
// threads per frame: one wavefront up to N = 512 (wave-private buffer, SY = 1: no barrier between passes); the whole
// 256-thread workgroup from N = 1024 on, where a wavefront's share of a float64 transform would not fit its registers
template <int N>
constexpr int tile_nt() { return N <= 512 ? 64 : 256; }
template <int N>
constexpr int tile_sy() { return tile_nt<N>() <= 64 ? 1 : tile_nt<N>(); }
// bins per thread of a frame's N + 1 bins
template <int N>
constexpr int tile_bins() { return N / tile_nt<N>() + 1; }

__device__ __forceinline__ double nan_if_nonfinite(double P) { return (P <= 1.79769313486231570e308) ? P : (double)NAN; }

// the workgroup's twiddles into LDS, visible to every thread on return
template <int N>
__device__ __forceinline__ void stage_tile_twiddles(cx<double>* tw, const cx<double>* src) {
  stage_twiddles<tile_nt<N>(), N>(tw, src, (int)threadIdx.x);
  __syncthreads();
}

// window * frame into the team's padded buffer, forward transform in place.  windowed_sample(jj) is element jj
// (0 .. 2N - 1) of the windowed frame: every path supplies its own loader.
template <int N, class WindowedSample>
__device__ __forceinline__ void frame_fft(cx<double>* buf, const cx<double>* tw, int lane, WindowedSample&& windowed_sample) {
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  for (int j = lane; j < N; j += NT) {
    const double v0 = windowed_sample(2 * j);
    const double v1 = windowed_sample(2 * j + 1);
    buf[lp<double>(j)] = {v0, v1};
  }
  team_sync<SY>();
  wave_fft<double, N, false, NT, SY>(buf, tw, lane);
}

// bin k (0..N) of the real transform held packed in buf, and its power (NaN when not finite)
template <int N>
__device__ __forceinline__ cx<double> packed_bin(const cx<double>* buf, const cx<double>* tw, int k) {
  cx<double> a = buf[lp<double>(k == N ? 0 : k)];
  cx<double> b = buf[lp<double>((k == 0 || k == N) ? 0 : N - k)];
  return rfft_bin(a, b, tw[k == N ? 0 : k], k, N);
}
template <int N>
__device__ __forceinline__ double bin_power(const cx<double>* buf, const cx<double>* tw, int k) {
  const cx<double> X = packed_bin<N>(buf, tw, k);
  return nan_if_nonfinite(X.x * X.x + X.y * X.y);
}

// the wavefront's decisions on bands k (one per lane) as one word of a bit row
__device__ __forceinline__ void store_ballot(unsigned long long* row, int wpr, int lane, int k, bool pass) {
  const unsigned long long word = __ballot(pass);
  if ((lane & 63) == 0 && (k >> 6) < wpr) row[k >> 6] = word;
}

// one transformed frame of the offline paths: decision bits against the threshold's compare constant and the running
// band maxima (stationary), or the magnitudes (non-stationary)
template <int N>
__device__ __forceinline__ void decide_frame(const TileConsts& C, const cx<double>* buf, const cx<double>* tw, int lane,
                                             const double* T2, unsigned long long* bits_row, float* mag_row,
                                             double (&vmax)[tile_bins<N>()]) {
  constexpr int NT = tile_nt<N>();
#pragma unroll
  for (int m = 0; m < tile_bins<N>(); ++m) {
    const int k = lane + NT * m;
    const double P = k <= N ? bin_power<N>(buf, tw, k) : 0.0;
    if (C.stationary) {
      vmax[m] = nanmax(vmax[m], P);
      store_ballot(bits_row, C.wpr, lane, k, k <= N && P > T2[k <= N ? k : 0]);
    } else if (k <= N) {
      mag_row[k] = (float)sqrt(P);
    }
  }
}
// exact whatever the order: the bit patterns of non-negative doubles order as the doubles do (NaN above all)
template <int N>
__device__ __forceinline__ void merge_band_maxima(unsigned long long* pmax_row, int lane, const double (&vmax)[tile_bins<N>()]) {
#pragma unroll
  for (int m = 0; m < tile_bins<N>(); ++m) {
    const int k = lane + tile_nt<N>() * m;
    if (k <= N) atomicMax(&pmax_row[k], (unsigned long long)__double_as_longlong(vmax[m]));
  }
}

// dB threshold -> compare constant on the raw power: T2_NEVER for a NaN threshold, -1 ("every cell passes") for one
// below 20 log10(eps), else ((10^(th / 20) - eps) / mag_scale)^2
__device__ __forceinline__ double thresh_to_t2(double th, double mag_scale) {
  const double eps = 2.220446049250313e-16;
  if (th != th) return T2_NEVER;
  if (20.0 * log10(eps) > th) return -1.0;
  const double tm = (exp10(th / 20.0) - eps) / mag_scale;
  return tm > 0.0 ? tm * tm : 0.0;
}

// threshold (dB) of one band of a noise source from its T power values col[t * FS]: maximum, moments of the floored dB
// relative to it (k_row_decide's summation structure: d = max(dB - max_dB, -top_db), s1 = sum d, s2 = sum d^2, serial
// over the frames), mean + n_std * std
__device__ __forceinline__ double noise_band_threshold(const TileConsts& C, const double* col, int64_t T) {
  double m = 0.0;
  for (int64_t t = 0; t < T; ++t) m = nanmax(m, col[t * C.FS]);
  const double mdb = cell_db(m, C.mag_scale);
  double s1 = 0.0, s2 = 0.0;
  for (int64_t t = 0; t < T; ++t) {
    double d = cell_db(col[t * C.FS], C.mag_scale) - mdb;
    d = (d != d) ? d : fmax(d, -C.top_db);
    s1 += d;
    s2 += d * d;
  }
  const double Tn = (double)T;
  const double mean_d = s1 / Tn;
  double var = (s2 - s1 * s1 / Tn) / (Tn - (double)C.ddof);
  if (var < 0.0) var = 0.0;
  return (mdb + mean_d) + sqrt(var) * C.n_std;
}

// what the band maximum makes of a band: 0 = the cell's own compare decides, 1 = every cell passes (the floor
// max - top_db lies above the threshold, or the threshold below 20 log10(eps): t2 < 0), 2 = none passes (NaN maximum
// or threshold)
__device__ __forceinline__ int band_mode(double pmax, double th, double t2, double mag_scale, double top_db) {
  if (th != th) return 2;
  const double fl = cell_db(pmax, mag_scale) - top_db;
  if (fl != fl) return 2;
  return (fl > th || t2 < 0.0) ? 1 : 0;
}

__device__ __forceinline__ float bit_at(const unsigned long long* row, int g) { return (float)((row[g >> 6] >> (g & 63)) & 1ull); }

// mask smoothing along frequency, one row by the whole workgroup: out[f] = sum_df (nf + 1 - |df|) raw(f + df), in the
// row's element type RT (float32; float64 for the sigmoid rows of an exact stream bank), df ascending, bands outside
// [0, F) skipped
template <class RT = float, class Raw>
__device__ __forceinline__ void fsmooth_row(RT* out, int F, int nf, Raw&& raw) {
  for (int f = threadIdx.x; f < F; f += blockDim.x) {
    RT acc = (RT)0;
    for (int df = -nf; df <= nf; ++df) {
      const int g = f + df;
      if (g < 0 || g >= F) continue;
      acc += (RT)(nf + 1 - (df < 0 ? -df : df)) * raw(g);
    }
    out[f] = acc;
  }
}

// mask smoothing along time at band k of frame t: K = sum_q (nt + 1 - |q - t|) R[row_of(q)][k] over the frames
// [t - nt, t + nt] that exist, and Et, the triangle's weight over those frames
struct TimeTaps {
  int64_t ta, tb;
  double Et;
};
__device__ __forceinline__ TimeTaps time_taps(int64_t t, int nt, int64_t T) {
  return {t - nt < 0 ? 0 : t - nt, t + nt >= T ? T - 1 : t + nt, (double)tri_valid(nt, t, T)};
}
template <class RT = float, class RowOf>
__device__ __forceinline__ double time_smooth(const RT* R, int FS, RowOf&& row_of, const TimeTaps& tp, int64_t t, int nt, int k) {
  double K = 0.0;
  for (int64_t q = tp.ta; q <= tp.tb; ++q) {
    const int64_t d = q - t;
    K += (double)(nt + 1 - (d < 0 ? -d : d)) * (double)R[row_of(q) * FS + k];
  }
  return K;
}
// stationary: prop_decrease first, then the zero-padded smoothing (the value outside the field is 0, not 1 - p)
__device__ __forceinline__ double mask_stationary(const TileConsts& C, double K, double Et, int k) {
  return (C.prop * K + (1.0 - C.prop) * Et * (double)tri_valid(C.nf, k, C.F)) / C.ktot;
}
// non-stationary: smoothed first, prop_decrease after
__device__ __forceinline__ double mask_nonstationary(const TileConsts& C, double K) {
  return (K / C.ktot) * C.prop + (1.0 - C.prop);
}

// ---- the merge half of a masked inverse: the Hermitian half Y[0 .. N] of a length-2N real frame's spectrum back into
// the packed half-size spectrum in buf, inverse transform, synthesis window.  Shared by mask_and_invert (Y = X * mask)
// and the adjoint of the gated spectrogram (Y = grad * mask, rows.hip's k_rw_spec_bwd).
// bins 0 and N, both real, into packed element 0
__device__ __forceinline__ void merge_dc_nyquist(cx<double>* buf, double y0, double yN) {
  buf[lp<double>(0)] = {0.5 * (y0 + yN), 0.5 * (y0 - yN)};
}
// bins k and N - k (0 < k <= N / 2; w = w_2N^k) into packed elements k and N - k
__device__ __forceinline__ void merge_bin_pair(cx<double>* buf, int k, int N, cx<double> Yk, cx<double> Yn, cx<double> w) {
  cx<double> Ep = {(Yk.x + Yn.x) * 0.5, (Yk.y - Yn.y) * 0.5};
  cx<double> D = {(Yk.x - Yn.x) * 0.5, (Yk.y + Yn.y) * 0.5};
  cx<double> wc = {w.x, -w.y};
  cx<double> Op = cmul(D, wc);
  buf[lp<double>(k)] = {Ep.x - Op.y, Ep.y + Op.x};
  if (k != N - k) buf[lp<double>(N - k)] = {Ep.x + Op.y, -Ep.y + Op.x};
}
// the merged spectrum in buf (every lane has written its elements) -> un-normalised inverse transform -> window * scale,
// the frame's n samples to seg_row in its element type ST (float32 rounds them once; float64 -- an exact stream bank --
// keeps them: same lane-to-sample mapping, double2 stores)
template <int N, class ST = float>
__device__ __forceinline__ void invert_and_window(cx<double>* buf, const cx<double>* tw, int lane, const double* wfull,
                                                  const double inv, ST* seg_row) {
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  team_sync<SY>();
  wave_fft<double, N, true, NT, SY>(buf, tw, lane);
  for (int j = lane; j < N; j += NT) {
    const cx<double> z = buf[lp<double>(j)];
    if constexpr (std::is_same<ST, double>::value)
      reinterpret_cast<double2*>(seg_row)[j] = make_double2(z.x * wfull[2 * j] * inv, z.y * wfull[2 * j + 1] * inv);
    else
      reinterpret_cast<float2*>(seg_row)[j] = make_float2((float)(z.x * wfull[2 * j] * inv), (float)(z.y * wfull[2 * j + 1] * inv));
  }
  team_sync<SY>();
}

// the packed transform of a real frame in buf times mask_at(k), k = 0 .. N (split / mask / merge; mask_at is called
// once per band), inverse transform (1 / N), synthesis window, the frame's n samples to seg_row.  emit(k, Y, m) sees
// every band's product Y[k] = X[k] * m -- the value that is merged and inverted, X unscaled -- and its mask value m
// once: a lane's bands are k = lane + NT i ascending and N - k descending, so lanes hold consecutive bins either way
// (the stream bank's spectrum store).  Bins 0 and N are real: their Y.y is +0.0.
struct NoEmit {
  __device__ __forceinline__ void operator()(int, cx<double>, double) const {}
};
template <int N, class ST = float, class MaskAt, class Emit = NoEmit>
__device__ __forceinline__ void mask_and_invert(cx<double>* buf, const cx<double>* tw, int lane, MaskAt&& mask_at,
                                                const double* wfull, ST* seg_row, Emit&& emit = Emit()) {
  constexpr int NT = tile_nt<N>();
  for (int k = lane; k <= N / 2; k += NT) {
    if (k == 0) {
      cx<double> a = buf[lp<double>(0)];
      const double s0 = a.x + a.y;
      const double m0 = mask_at(0);
      const double y0 = s0 * m0;
      const double sN = a.x - a.y;
      const double mN = mask_at(N);
      const double yN = sN * mN;
      emit(0, cx<double>{y0, 0.0}, m0);
      emit(N, cx<double>{yN, 0.0}, mN);
      merge_dc_nyquist(buf, y0, yN);
    } else {
      cx<double> a = buf[lp<double>(k)], b = buf[lp<double>(N - k)];
      cx<double> w = tw[k];
      cx<double> E = {(a.x + b.x) * 0.5, (a.y - b.y) * 0.5};
      cx<double> O = {(a.y + b.y) * 0.5, (b.x - a.x) * 0.5};
      cx<double> wO = cmul(w, O);
      const double mk = mask_at(k), mn = (k != N - k) ? mask_at(N - k) : mk;
      cx<double> Yk = {(E.x + wO.x) * mk, (E.y + wO.y) * mk};
      cx<double> Yn = {(E.x - wO.x) * mn, (-E.y + wO.y) * mn};
      emit(k, Yk, mk);
      if (k != N - k) emit(N - k, Yn, mn);
      merge_bin_pair(buf, k, N, Yk, Yn, w);
    }
  }
  invert_and_window<N, ST>(buf, tw, lane, wfull, 1.0 / (double)N, seg_row);
}

// the adjoint frame of Y = mask .* rfft(window * frame) with the mask fixed: Y[k] = m[k] g[k] for
// 0 < k < N, Y[0] = 2 m[0] Re g[0], Y[N] = 2 m[N] Re g[N] read as a Hermitian half, merged, inverted WITHOUT the 1 / N
// and windowed: seg_row[j] = window[j] Re sum_{k=0}^{N} m[k] g[k] e^{+2 pi i k j / 2N}, every bin with weight 1.
// grad_at(k) -> cx<double>, mask_at(k) -> double; each is called once per band.  No envelope division.
template <int N, class ST = float, class GradAt, class MaskAt>
__device__ __forceinline__ void mask_and_adjoint(cx<double>* buf, const cx<double>* tw, int lane, GradAt&& grad_at,
                                                 MaskAt&& mask_at, const double* wfull, ST* seg_row) {
  constexpr int NT = tile_nt<N>();
  for (int k = lane; k <= N / 2; k += NT) {
    if (k == 0) {
      merge_dc_nyquist(buf, 2.0 * grad_at(0).x * mask_at(0), 2.0 * grad_at(N).x * mask_at(N));
    } else {
      const cx<double> gk = grad_at(k), gn = (k != N - k) ? grad_at(N - k) : gk;
      const double mk = mask_at(k), mn = (k != N - k) ? mask_at(N - k) : mk;
      merge_bin_pair(buf, k, N, {gk.x * mk, gk.y * mk}, {gn.x * mn, gn.y * mn}, tw[k]);
    }
  }
  invert_and_window<N, ST>(buf, tw, lane, wfull, 1.0, seg_row);
}

// frames [t_lo, t_hi] of a T-frame signal whose `span` samples cover extended position e (= output position + padL)
__device__ __forceinline__ void ola_span(int64_t e, int span, int H, int64_t T, int64_t* t_lo, int64_t* t_hi) {
  *t_hi = e / H;
  if (*t_hi > T - 1) *t_hi = T - 1;
  *t_lo = (e - span + 1 <= 0) ? 0 : (e - span + H) / H;
}
// sum of w^2 over those frames (the overlap-add envelope at e)
__device__ __forceinline__ double ola_envelope(const double* wfull, int64_t e, int H, int64_t t_lo, int64_t t_hi) {
  double norm = 0.0;
  for (int64_t t = t_lo; t <= t_hi; ++t) {
    const double w = wfull[(int)(e - t * H)];
    norm += w * w;
  }
  return norm;
}
// overlap-add of the offline paths at extended position e: sum of the frames' segments (frame t's at seg_row_of(t) * n)
// and the envelope, in one walk over the frames
template <class ST = float, class SegRowOf>
__device__ __forceinline__ void ola_sum(const TileConsts& C, const ST* seg, SegRowOf&& seg_row_of, int64_t e, int64_t T,
                                        double* acc, double* norm) {
  int64_t t_lo, t_hi;
  ola_span(e, C.n, C.H, T, &t_lo, &t_hi);
  *acc = 0.0;
  *norm = 0.0;
  for (int64_t t = t_lo; t <= t_hi; ++t) {
    const int m = (int)(e - t * C.H);
    *acc += (double)seg[seg_row_of(t) * (int64_t)C.n + m];
    *norm += C.wfull[m] * C.wfull[m];
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
inline bool tile_geom_ok(int N) { return N == 128 || N == 256 || N == 512 || N == 1024 || N == 2048; }

inline TileConsts fill_consts(const RgCtx& c) {
  TileConsts C{};
  C.n = c.n; C.W = c.W; C.H = c.H; C.F = c.F; C.FS = c.FS; C.padL = c.padL; C.wpr = (c.F + 63) / 64;
  C.mag_scale = c.mag_scale; C.top_db = c.top_db; C.n_std = c.n_std; C.prop = c.prop; C.nthresh = c.nthresh;
  C.slope = c.slope; C.iir_b = c.iir_b; C.ddof = c.ddof; C.nf = c.nf; C.nt = c.nt; C.stationary = c.stationary;
  C.ktot = (double)((int64_t)(c.nf + 1) * (c.nf + 1) * (int64_t)(c.nt + 1) * (c.nt + 1));
  C.tw = (const cx<double>*)c.tw64; C.wfull = c.wfull64;
  return C;
}

// profiler scope of one stage (api.hip's hooks, RgCtx)
struct Prof {
  const RgCtx& c;
  void* tok;
  Prof(const RgCtx& c_, int stage, hipStream_t st) : c(c_), tok(c_.prof_begin ? c_.prof_begin(c_.hook_ctx, stage, st) : nullptr) {}
  ~Prof() { if (c.prof_end) c.prof_end(tok); }
};

// a device buffer of at least `need` bytes; growing it synchronises the stream once and drops the old contents
inline int grow_device_buffer(host::DevBuf& buf, size_t need, hipStream_t st, const char* who, const char* what, std::string* err) {
  if (buf.bytes >= need) return SG_OK;
  if (buf.p) { (void)hipStreamSynchronize(st); buf.release(); }
  if (hipMalloc(&buf.p, need) != hipSuccess) {
    buf.p = nullptr;
    char b[160];
    snprintf(b, sizeof b, "%s: %s allocation of %zu bytes failed", who, what, need);
    *err = b;
    return SG_E_NOMEM;
  }
  buf.bytes = need;
  return SG_OK;
}

// several host tables into consecutive device memory with one copy: part i takes `room` bytes (>= bytes) at dst.  The
// staging buffer is pageable host memory: hipMemcpyAsync has staged it before returning, so it may go at once.
struct TablePart {
  const void* p;
  size_t bytes, room;
};
inline hipError_t upload_tables(void* dst, hipStream_t st, std::initializer_list<TablePart> parts) {
  size_t total = 0;
  for (const TablePart& t : parts) total += t.room;
  if (total == 0) return hipSuccess;
  std::vector<char> host(total);
  size_t o = 0;
  for (const TablePart& t : parts) {
    if (t.bytes) memcpy(host.data() + o, t.p, t.bytes);
    o += t.room;
  }
  return hipMemcpyAsync(dst, host.data(), host.size(), hipMemcpyHostToDevice, st);
}

// f(std::integral_constant<int, N>{}) for the half transform length N of the handle
template <class F>
hipError_t dispatch_N(int N, F&& f) {
  switch (N) {
    case 128: return f(std::integral_constant<int, 128>{});
    case 256: return f(std::integral_constant<int, 256>{});
    case 512: return f(std::integral_constant<int, 512>{});
    case 1024: return f(std::integral_constant<int, 1024>{});
    case 2048: return f(std::integral_constant<int, 2048>{});
  }
  return hipErrorInvalidValue;
}

// f(std::true_type{}) or f(std::false_type{}): a run-time switch as a template argument of what f launches.  The true
// branch is named first; dispatch_flags(a, b, f) calls f(A, B) and names (1, 1), (1, 0), (0, 1), (0, 0) in that order
template <class F>
auto dispatch_flag(bool on, F&& f) {
  return on ? f(std::true_type{}) : f(std::false_type{});
}
template <class F>
auto dispatch_flags(bool a, bool b, F&& f) {
  return dispatch_flag(a, [&](auto A) { return dispatch_flag(b, [&](auto B) { return f(A, B); }); });
}

inline dim3 tile_grid(int64_t ntiles) { return dim3((unsigned)std::max<int64_t>(1, ntiles)); }

// a transform kernel of geometry N, one workgroup per tile: twiddles + padded frame buffer in dynamic LDS
template <int N, class Args>
hipError_t launch_tile_kernel(void (*kernel)(Args), int64_t ntiles, hipStream_t st, const Args& A) {
  const size_t lds = (size_t)(N + lpn<double>(N)) * sizeof(cx<double>);
  return host::launch_lds_if(lds > 65536, kernel, tile_grid(ntiles), dim3(tile_nt<N>()), lds, st, A);
}
// a kernel without dynamic LDS, one workgroup of `block` threads per tile
template <class Args>
hipError_t launch_flat_kernel(void (*kernel)(Args), int64_t ntiles, int block, hipStream_t st, const Args& A) {
  hipLaunchKernelGGL(kernel, tile_grid(ntiles), dim3(block), 0, st, A);
  return hipGetLastError();
}

}  // namespace sg
