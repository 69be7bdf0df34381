// libmi355gate.so -- the gate engine behind the C ABI of include/mi355gate.h: the FFT-size dispatchers, the workspace,
// every stage and pipeline (statistics, decide, smooth, apply, the one-pass and row gates) and the entry points that run
// them, enqueued on the caller's HIP stream.  gfx950 only.  The one unit that includes the gate's kernel headers.
// The rest of the host side: create.hip (handle, tables, buffers), debug.hip (options, profiler, taps), shims.hip
// (clips / rows / stream entry points); handle.hpp is what the four share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mi355gate_debug.h"
// Floating-point contraction only INSIDE a source expression (the language rule), never across statements: with the
// compiler's default (fast) the back end fuses a product into whichever neighbouring add it meets first, and that
// choice changes with unrelated edits -- two kernels that share a formula then round differently in the cells where
// both products of a sum are inexact.  The one-pass gate and the three-kernel path are bit-identical by
// construction only under this rule; where a fused multiply-add is wanted across statements the code says fmaf().
#pragma clang fp contract(on)
#include "kernels.hpp"
#include "fused.hpp"
#include "czt.hpp"
#include "mixed.hpp"
#include "onepass.hpp"
#include "rowgate.hpp"
#include "rowbwd.hpp"
#include "fast512.hpp"
#include "onepass512.hpp"
#include "fast256.hpp"
#include "onepass256.hpp"
#include "fast2048.hpp"
#include "onepass2048.hpp"
#include "nonstat.hpp"
#include "fast64.hpp"
#include "big.hpp"
#include "exact.hpp"
#include "apply64.hpp"
#include "ragged.hpp"
#include "rows.hpp"
#include "stream.hpp"
#include "spec.hpp"
#include "feat.hpp"
#include "feat_tables.hpp"
#include "handle.hpp"
#include "launch.hpp"

// complex transform length from which a whole 256-thread workgroup (instead of one wavefront) works on ONE frame in
// the general LDS kernels: at N = 2048 (n_fft = 4096) a wavefront holds 4 radix-8 butterflies = 64 complex values per
// lane -- 256 VGPRs and scratch, one wave per SIMD
#ifndef SG_TEAM_N
#define SG_TEAM_N 2048
#endif
// (round 5) threads that share one frame in the LDS-Stockham kernels (fft_wave.hpp): the whole workgroup from N = SG_TEAM_N
// on, one wavefront for 512 <= N < SG_TEAM_N, and SUB-wavefront teams for short frames -- a radix-8 pass over N complex
// points has N / 8 butterflies, so a 64-lane team on N = 128 (n_fft = 256) idles 48 lanes in two of its three passes.
// SG_SHORT_TEAMS=0 at build time restores one wavefront per frame (A/B).
#ifndef SG_SHORT_TEAMS
#define SG_SHORT_TEAMS 1
#endif
template <int N>
constexpr int team_threads() {
  return N >= SG_TEAM_N ? 256 : (!SG_SHORT_TEAMS ? 64 : (N <= 128 ? 16 : (N == 256 ? 32 : 64)));
}
// teams per workgroup: 256 threads unless the transform buffers (`elem` bytes per complex point) would not fit
template <int N>
constexpr int team_count(size_t elem) {
  return N >= SG_TEAM_N ? 1 : (team_threads<N>() < 64 ? 256 / team_threads<N>() : ((N * elem > 16384) ? 2 : 4));
}
#ifndef SG_APPLY_WAVES
#define SG_APPLY_WAVES 4  // wavefronts per workgroup of k_apply_fast: tile = 4*W frames -> 4*W-3 hops
#endif

using namespace sg;
using namespace sg::host;

// Register geometries: n_fft = win = 512 / 256 / 2048, hop = n_fft / 4 (fast512.hpp, fast256.hpp, fast2048.hpp and the
// one-pass gates of onepass512.hpp, onepass256.hpp, onepass2048.hpp).  One descriptor per geometry holds its constants and
// its kernels; sg_create stores the handle's (sg_handle::reg) and every stage of these geometries reads it.

// The hops (hop-sample blocks of the extended signal, ext = unit sample + padL) that hold the output samples [om.p0, om.p1)
struct HopRange {
  int64_t h_begin, h_end;
  int64_t count() const { return h_end - h_begin; }
};
static HopRange hop_range(const OutMap& om, const Geom& g, int hop) {
  return {(om.p0 + g.padL) / hop, (om.p1 - 1 + g.padL) / hop + 1};
}
// abutting tiles of `frames` frames over nh hops: the last tile must reach 3 hops past the range (its leading partials)
static int64_t abutting_tiles(int64_t nh, int frames) { return (nh + 3 + frames - 1) / frames; }

constexpr size_t FAST5_LDS = (size_t)(fast::FN + 4 * fast::WAVE_CX_H) * sizeof(fast::cf) + (512 + 264) * sizeof(float);
constexpr size_t FAST25_LDS = (size_t)(fast::FN + 4 * fast::WAVE_CX_H) * sizeof(fast::cf) + (256 + fast::F25_T2) * sizeof(float);
constexpr size_t FAST20_LDS = (size_t)(1024 + 4 * fast::WAVE_CX_H) * sizeof(fast::cf) + 1028 * sizeof(float);

// n_fft = 512: the 512-point complex transform of the default geometry carries two real frames
const RegGeom sg::host::REG512{
    512, 128, 32, 29, FAST5_LDS, &sg_handle::tw512,
    {128, fast::O5_NF, fast::O5_NH, fast::O5_TILE_WORDS, fast::O5_XW, fast::O5_MAX_NF, fast::O5_MAX_NT, 257, FAST5_LDS + 16 + 2048},
    {128, fast::O5_NF, fast::O5_NF, fast::O5_TILE_WORDS, fast::O5_XW, fast::O5_MAX_NF, fast::O5_MAX_NT, 257, FAST5_LDS + 16 + 2048, 3},
    false, 2,
    {fast::k_decide_fast512<4, false>, fast::k_decide_fast512<4, true>}, fast::k_mag_fast512<4>,
    {fast::k_apply_fast512<4, false>, fast::k_apply_fast512<4, true>},
    {fast::k_gate_onepass512<4, false>, fast::k_gate_onepass512<4, true>}, fast::k_ola_seam<128, 32>};
// n_fft = 256 (round 5): the same transform carries four real frames
const RegGeom sg::host::REG256{
    256, 64, 64, 61, FAST25_LDS, &sg_handle::tw512,
    {64, fast::O25_NF, fast::O25_NH, fast::O25_TILE_WORDS, fast::O25_XW, fast::O25_MAX_NF, fast::O25_MAX_NT, 129, FAST25_LDS + 16 + 2048},
    {64, fast::O25_NF, fast::O25_NF, fast::O25_TILE_WORDS, fast::O25_XW, fast::O25_MAX_NF, fast::O25_MAX_NT, 129, FAST25_LDS + 16 + 2048, 3},
    false, 3,
    {fast::k_decide_fast256<4, false>, fast::k_decide_fast256<4, true>}, fast::k_mag_fast256<4>,
    {fast::k_apply_fast256<4, false>, fast::k_apply_fast256<4, true>},
    {fast::k_gate_onepass256<4, false>, fast::k_gate_onepass256<4, true>}, fast::k_ola_seam<64, 64>};
// n_fft = 2048: one real frame per 32 lanes (1024-point transform); the one-pass gate's tiles always abut
const RegGeom sg::host::REG2048{
    2048, 512, 8, 5, FAST20_LDS, &sg_handle::tw32,
    {512, fast::O20_NF, fast::O20_NF, fast::O20_TILE_WORDS, fast::O20_XW, fast::O20_MAX_NF, fast::O20_MAX_NT, 1025, FAST20_LDS + 16 + 2048, 3},
    {512, fast::O20_NF, fast::O20_NF, fast::O20_TILE_WORDS, fast::O20_XW, fast::O20_MAX_NF, fast::O20_MAX_NT, 1025, FAST20_LDS + 16 + 2048, 3},
    true, 1,
    {fast::k_decide_fast2048<4, false>, fast::k_decide_fast2048<4, true>}, fast::k_mag_fast2048<4>,
    {fast::k_apply_fast2048<4, false>, fast::k_apply_fast2048<4, true>},
    {fast::k_gate_onepass2048<4, false>, fast::k_gate_onepass2048<4, true>}, fast::k_ola_seam<512, 8>};

// n_fft = 1024, hop 256 (onepass.hpp): abutting tiles of 16 frames.  The PROP instantiations keep 528 bytes more.
constexpr size_t OP_PROP_LDS = 528;
static const OnePassGeom OP1024{
    256, 16, 16, fast::OP_TILE_WORDS, fast::OP_XW, 8, fast::OP_MAX_NT, 513,
    (size_t)(fast::FN + 4 * fast::WAVE_CX_H) * sizeof(fast::cf) + (1024 + T2_FLOATS) * sizeof(float) + 256 * 8 + 514 * 8 + 192 * 8 + 32,
    3};

// the handle's register geometry, or nullptr (another geometry, or SG_OPT_FORCE_NOFAST)
static const RegGeom* reg_geom(const sg_handle* h) { return h->force_nofast ? nullptr : h->reg; }

// Routing (route.hpp): what plan_S / plan_T read of the handle, copied once per call.  The one place where a capability flag
// or a force_* option is read for the choice of a route; the stages take the plan.
static_assert(route::NS_TT == NS_TT && route::NS_MAX_NF == NS_MAX_NF && route::NS_IIR_MAX_NT == NS_IIR_MAX_NT &&
              route::NS_BOX_MAX_NT == NS_BOX_MAX_NT && route::NS_BOX_KB == NS_BOX_KB && route::XIIR_TT == exact::XIIR_TT &&
              route::RG_FRAMES == fast::RG_FRAMES && route::RG_NFMAX == fast::RG_NFMAX && route::RG_NTMAX == fast::RG_NTMAX &&
              route::ns_iir_nt_ok(25) == ns_iir_nt_ok(25) && route::ns_iir_nt_ok(21) == ns_iir_nt_ok(21),
              "route.hpp states the limits of the kernel headers");
static int64_t ws_budget(const sg_handle* h) {
  return h->p.max_workspace_bytes > 0 ? h->p.max_workspace_bytes : (int64_t)8 << 30;
}
static route::RouteCaps route_caps(const sg_handle* h) {
  route::RouteCaps c;
  c.variant = h->p.variant; c.stationary = h->p.stationary != 0; c.smooth_mask = h->p.smooth_mask != 0;
  c.prop_decrease = h->p.prop_decrease; c.iir_b = h->p.iir_b;
  c.nf = h->p.n_grad_freq; c.nt = h->p.n_grad_time; c.n_movemean = h->p.n_movemean;
  c.ktot = h->ktot; c.fused_ok = h->fused_ok; c.t_sm2_ok = h->t_sm2_ok;
  using route::GeomClass;
  c.geom = h->big_M ? GeomClass::LONG : h->mr_ok ? GeomClass::MIXED : h->czt_M ? GeomClass::CZT :
           h->fast_ok ? GeomClass::DEFAULT : h->reg ? GeomClass::REG : GeomClass::POW2;
  if (c.geom == GeomClass::DEFAULT) c.op = c.op_seam = &OP1024;
  if (c.geom == GeomClass::REG) { c.op = &h->reg->op; c.op_seam = &h->reg->op_seam; c.reg_abut = h->reg->abut; c.reg_frames = h->reg->frames; }
  c.ftab3 = h->ftab3.p != nullptr; c.optab = h->optab.p != nullptr; c.regtab = h->regtab.p != nullptr; c.norm64 = h->norm64.p != nullptr;
  c.force_unfused = h->force_unfused; c.force_nofast = h->force_nofast; c.force_f64_decide = h->force_f64_decide;
  c.force_noseam = h->force_noseam; c.force_nolean = h->force_nolean; c.force_split = h->force_split;
  c.fast_integer = h->fast_integer; c.force_exact = h->force_exact; c.exact_materialised = h->exact_materialised;
  c.rowgate_mode = h->rowgate_mode; c.tile_order = h->tile_order;
  c.ws_budget = ws_budget(h);
  return c;
}
// ... and of the call: the geometry of its units and the hops of the handle's tile geometry under the output map
static route::RouteShape route_shape(const route::RouteCaps& c, const Geom& g, int64_t p0, int64_t p1, int in_dtype, int out_dtype,
                                     int64_t units) {
  route::RouteShape s;
  s.F = g.F; s.FS = g.FS; s.n = g.n; s.T = g.T;
  if (c.op) s.nh = (p1 - 1 + g.padL) / c.op->hop + 1 - (p0 + g.padL) / c.op->hop;   // hop_range(om, g, hop).count()
  s.in_dtype = in_dtype; s.out_dtype = out_dtype; s.units = units;
  return s;
}
// (host bookkeeping behind sg_debug_fetch / sg_debug_dims / sg_debug_range: what a batch left in the workspace.  A route
// that keeps no fields reports 0 units; one that decides no bits leaves the range of the last one that did.)
static void note_batch(sg_handle* h, const route::BatchFacts& f, int64_t nb, const Geom& g, const Decided& d = Decided{}) {
  LastBatch& b = h->last;
  if (!f.keeps) { b.units = 0; return; }
  b.units = nb; b.T = g.T; b.g = g;
  b.has_P = f.has_P; b.has_raw = f.has_raw; b.fused = f.fused; b.fast = f.fast; b.k16_only = f.k16_only; b.rg = f.rg;
  b.xbits = f.range == route::Range::TILES;
  if (b.xbits) b.tiles = d.tiles;
  if (f.range == route::Range::ALL) { b.db = 0; b.de = g.T; }
  else if (f.range != route::Range::KEEP) { b.db = d.db; b.de = d.de; }
}
// host bookkeeping behind sg_debug_counter 17 (no kernel reads or writes it)
static void note_smooth(sg_handle* h, int id, int cell_bytes, int tile_frames) {
  h->smooth_route = (int64_t)id | ((int64_t)cell_bytes << 8) | ((int64_t)tile_frames << 16);
}

// ------------------------------------------------------------------------------------------
// kernel dispatch on the FFT size
// ------------------------------------------------------------------------------------------
// f(std::integral_constant<int, N>{}) for the half transform length n = N, a power of two in [32, MAX]  (tile_core.hpp: dispatch_N)
template <int MAX, int N = 32, class F>
static hipError_t dispatch_pow2(int n, F&& f) {
  if (n == N) return f(std::integral_constant<int, N>{});
  if constexpr (N < MAX) return dispatch_pow2<MAX, 2 * N>(n, f);
  else return hipErrorInvalidValue;
}

template <typename TC, int N>
static hipError_t launch_stft_n(const View& v, const Geom& g, int64_t units, const void* tw, const void* wfull,
                                double* P, float* mag, double* z, double zscale, hipStream_t st,
                                unsigned long long* pmax_bits) {
  // n_fft = 8192 (N = 4096): the whole workgroup cooperates on one frame
  constexpr int NT = team_threads<N>();
  constexpr int WAVES = team_count<N>(sizeof(cx<TC>));
  size_t lds = (size_t)(N + WAVES * lpn<TC>(N)) * sizeof(cx<TC>);
  // few units (the noise clip): one frame per wave so that the grid still covers the chip
  const bool small = units * ((g.T + WAVES * 4 - 1) / (WAVES * 4)) < 1024;
  auto launch = [&](auto kern, int fpw) -> hipError_t {
    dim3 grid((unsigned)((g.T + WAVES * fpw - 1) / (WAVES * fpw)), (unsigned)units);
    return launch_lds_if(lds > 65536, kern, grid, dim3(WAVES * NT), lds, st, v, g, (const cx<TC>*)tw, (const TC*)wfull, P, mag,
                         z, zscale, pmax_bits);
  };
  if constexpr (sizeof(TC) == 8 && N >= 1024 && N < SG_TEAM_N) {
    // (round 5) the noise clip in float64 at n_fft = 2048: 293 workgroups of four one-frame wavefronts are one
    // latency-bound round of 32 us.  The whole workgroup on one frame (the N >= SG_TEAM_N shape): four times the
    // workgroups, each transform split over 256 threads: 16.5 us.  (n_fft = 1024 measured too: 14.0 -> 15.9 us, so not there.)
    if (small && units * g.T <= 16384) {
      const size_t lds1 = (size_t)(N + lpn<TC>(N)) * sizeof(cx<TC>);
      return launch_lds_if(lds1 > 65536, k_stft<TC, N, 1, 1, 256>, dim3((unsigned)g.T, (unsigned)units), dim3(256), lds1, st, v, g,
                           (const cx<TC>*)tw, (const TC*)wfull, P, mag, z, zscale, pmax_bits);
    }
  }
  if (small) return launch(k_stft<TC, N, WAVES, 1, NT>, 1);
  return launch(k_stft<TC, N, WAVES, 4, NT>, 4);
}

template <typename TC>
static hipError_t launch_stft(int N, const View& v, const Geom& g, int64_t units, const void* tw,
                              const void* wfull, double* P, float* mag, double* z, double zscale,
                              hipStream_t st, unsigned long long* pmax_bits = nullptr) {
  return dispatch_pow2<4096>(N, [&](auto n) { return launch_stft_n<TC, decltype(n)::value>(v, g, units, tw, wfull, P, mag, z, zscale, st, pmax_bits); });
}

template <int N, int MODE>
static hipError_t launch_bits_n(const View& v, const Geom& g, int64_t units, const void* tw, const void* wfull,
                                const ThreshConsts& tc, double mag_scale, double top_db,
                                unsigned long long* pmax_bits, unsigned long long* bits, int wpr,
                                hipStream_t st) {
  // from N = 2048 (n_fft = 4096) on the 256 threads of a workgroup share one frame (k_stft does the same): a single wave's
  // 2048-point float64 pass held 512 registers and 476 B of scratch
  constexpr int NT = N >= SG_TEAM_N ? 256 : 64;
  constexpr int WAVES = N >= SG_TEAM_N ? 1 : ((N * sizeof(cx<double>) > 16384) ? 2 : 4);
  constexpr int FPW = 4;
  size_t lds = (size_t)(N + WAVES * lpn<double>(N)) * sizeof(cx<double>) + (size_t)(N + 1) * sizeof(double);
  auto kern = k_stft_bits<N, WAVES, FPW, MODE, NT>;
  dim3 grid((unsigned)((g.T + WAVES * FPW - 1) / (WAVES * FPW)), (unsigned)units);
  return launch_lds_if(lds > 65536, kern, grid, dim3(WAVES * NT), lds, st, v, g, (const cx<double>*)tw, (const double*)wfull, tc,
                       mag_scale, top_db, pmax_bits, bits, wpr);
}

template <int MODE>
static hipError_t launch_bits(int N, const View& v, const Geom& g, int64_t units, const void* tw,
                              const void* wfull, const ThreshConsts& tc, double mag_scale, double top_db,
                              unsigned long long* pmax_bits, unsigned long long* bits, int wpr, hipStream_t st) {
  return dispatch_pow2<2048>(N, [&](auto n) { return launch_bits_n<decltype(n)::value, MODE>(v, g, units, tw, wfull, tc, mag_scale, top_db, pmax_bits, bits, wpr, st); });
}

template <int N>
static hipError_t launch_decide_lds_n(const sg_handle* h, const View& v, const Geom& g, int64_t units,
                                      const ThreshConsts& tc, unsigned long long* bits, int wpr, hipStream_t st) {
  constexpr int NT = team_threads<N>() > 64 ? 64 : team_threads<N>();   // (a frame never spans wavefronts here)
  constexpr int WAVES = NT < 64 ? 256 / NT : ((N * sizeof(cx<float>) > 8192) ? 2 : 4);
  constexpr int FPW = 4;
  const size_t lds = (size_t)(N + WAVES * N) * sizeof(cx<float>) + (size_t)(N + 1) * sizeof(float);
  auto kern = k_decide_lds<N, WAVES, FPW, NT>;
  dim3 grid((unsigned)((g.T + WAVES * FPW - 1) / (WAVES * FPW)), (unsigned)units);
  return launch_lds_if(lds > 65536, kern, grid, dim3(WAVES * NT), lds, st, v, g, (const cx<float>*)h->tw32.p,
                       (const float*)h->wa32.p, (const cx<double>*)h->tw64.p, (const double*)h->wfull64.p, tc,
                       h->mag_scale, h->p.top_db, bits, wpr);
}

// (mixed-radix frame lengths, mixed.hpp: see the section below)
static hipError_t launch_decide_mr(const sg_handle* h, const View& v, const Geom& g, int64_t units, const ThreshConsts& tc,
                                   unsigned long long* bits, int wpr, hipStream_t st) {
  return mr_launch_decide(h->mr, v, g, units, (const cx<float>*)h->tw32.p, (const cx<float>*)h->mr_pt32.p, (const float*)h->wa32.p, (const cx<double>*)h->tw64.p,
                          (const double*)h->wfull64.p, tc, h->mag_scale, h->p.top_db, bits, wpr, st);
}
static hipError_t launch_decide_lds(const sg_handle* h, const View& v, const Geom& g, int64_t units,
                                    const ThreshConsts& tc, unsigned long long* bits, int wpr, hipStream_t st) {
  if (h->mr_ok) return launch_decide_mr(h, v, g, units, tc, bits, wpr, st);
  return dispatch_pow2<2048>(h->N, [&](auto n) { return launch_decide_lds_n<decltype(n)::value>(h, v, g, units, tc, bits, wpr, st); });
}

template <int N>
static hipError_t launch_apply_n(const View& v, const Geom& g, int64_t units, const void* tw, const float* wa,
                                 const float* ws, const float* M, float* seg, hipStream_t st,
                                 const unsigned short* K16, float kscale) {
  constexpr int NT = team_threads<N>();
  constexpr int WAVES = team_count<N>(sizeof(cx<float>));
  constexpr int FPW = 4;
  size_t lds = (size_t)(N + WAVES * lpn<float>(N)) * sizeof(cx<float>);
  auto kern = k_apply_istft<N, WAVES, FPW, NT>;
  dim3 grid((unsigned)((g.T + WAVES * FPW - 1) / (WAVES * FPW)), (unsigned)units);
  return launch_lds_if(lds > 65536, kern, grid, dim3(WAVES * NT), lds, st, v, g, (const cx<float>*)tw, wa, ws, M, seg, K16, kscale);
}

static hipError_t launch_apply(int N, const View& v, const Geom& g, int64_t units, const void* tw,
                               const float* wa, const float* ws, const float* M, float* seg, hipStream_t st,
                               const unsigned short* K16 = nullptr, float kscale = 0.f) {
  return dispatch_pow2<4096>(N, [&](auto n) { return launch_apply_n<decltype(n)::value>(v, g, units, tw, wa, ws, M, seg, st, K16, kscale); });
}

// ------------------------------------------------------------------------------------------
// mixed-radix kernels (mixed.hpp): frame lengths 2 N with N = 2^a 3^b 5^c 7^d 11^e 13^f <= 2048 that are not powers of two
// ------------------------------------------------------------------------------------------
template <typename TC>
static hipError_t launch_stft_mr(const sg_handle* h, const View& v, const Geom& g, int64_t units, const void* wfull, double* P,
                                 float* mag, double* z, double zscale, hipStream_t st, unsigned long long* pmax_bits) {
  if constexpr (sizeof(TC) == 8)
    return mr_launch_stft64(h->mr, v, g, units, (const cx<double>*)h->tw64.p, (const cx<double>*)h->mr_pt64.p, (const double*)wfull, P, mag, z, zscale,
                            pmax_bits, st);
  else
    return mr_launch_stft32(h->mr, v, g, units, (const cx<float>*)h->tw32.p, (const cx<float>*)h->mr_pt32.p, (const float*)wfull, P, mag, z, zscale,
                            pmax_bits, st);
}
template <int MODE>
static hipError_t launch_bits_mr(const sg_handle* h, const View& v, const Geom& g, int64_t units, const ThreshConsts& tc,
                                 unsigned long long* pmax_bits, unsigned long long* bits, int wpr, hipStream_t st) {
  return mr_launch_bits(MODE, h->mr, v, g, units, (const cx<double>*)h->tw64.p, (const cx<double>*)h->mr_pt64.p, (const double*)h->wfull64.p, tc, h->mag_scale,
                        h->p.top_db, pmax_bits, bits, wpr, st);
}
static hipError_t launch_apply_mr(const sg_handle* h, const View& v, const Geom& g, int64_t units, const float* wa, const float* ws,
                                  const float* M, float* seg, hipStream_t st, const unsigned short* K16, float kscale) {
  return mr_launch_apply(h->mr, v, g, units, (const cx<float>*)h->tw32.p, (const cx<float>*)h->mr_pt32.p, wa, ws, M, seg, K16, kscale, st);
}
// (the decision kernels of the fused path, whatever transform the frame length runs on)
template <int MODE>
static hipError_t launch_bits_any(const sg_handle* h, const View& v, const Geom& g, int64_t units, const ThreshConsts& tc,
                                  unsigned long long* pmax_bits, unsigned long long* bits, int wpr, hipStream_t st) {
  if (h->mr_ok) return launch_bits_mr<MODE>(h, v, g, units, tc, pmax_bits, bits, wpr, st);
  return launch_bits<MODE>(h->N, v, g, units, h->tw64.p, h->wfull64.p, tc, h->mag_scale, h->p.top_db, pmax_bits, bits, wpr, st);
}

// ------------------------------------------------------------------------------------------
// chirp-z kernels (n_fft not a power of two): dispatch on the convolution size M
// ------------------------------------------------------------------------------------------
template <int M>
struct CztShape {
  static constexpr int NT = M >= 2048 ? 256 : 64;  // threads per frame
  static constexpr int FR = M >= 2048 ? 1 : 4;     // frames in flight per workgroup
};

template <typename TC, int M>
static hipError_t launch_stft_czt_m(const View& v, const Geom& g, int64_t units, const CztTabs<TC>& tb,
                                    const void* wfull, double* P, float* mag, double* z, double zscale,
                                    hipStream_t st, unsigned long long* pmax_bits) {
  constexpr int NT = CztShape<M>::NT, FR = CztShape<M>::FR;
  const size_t lds = (size_t)FR * lpn<TC>(M) * sizeof(cx<TC>);
  auto kern = k_stft_czt<TC, M, NT, FR>;
  const int fpb = units * ((g.T + FR * 4 - 1) / (FR * 4)) < 1024 ? 1 : 4;
  dim3 grid((unsigned)((g.T + FR * fpb - 1) / (FR * fpb)), (unsigned)units);
  return launch_lds_if(lds > 65536, kern, grid, dim3(NT * FR), lds, st, v, g, tb, (const TC*)wfull, P, mag, z, zscale, pmax_bits,
                       fpb);
}

template <int M>
static hipError_t launch_apply_czt_m(const View& v, const Geom& g, int64_t units, const CztTabs<float>& tb,
                                     const float* wa, const float* ws, const float* Mk, float* seg,
                                     hipStream_t st) {
  constexpr int NT = CztShape<M>::NT, FR = CztShape<M>::FR;
  const size_t lds = (size_t)FR * lpn<float>(M) * sizeof(cx<float>);
  auto kern = k_apply_istft_czt<M, NT, FR>;
  const int fpb = 4;
  dim3 grid((unsigned)((g.T + FR * fpb - 1) / (FR * fpb)), (unsigned)units);
  return launch_lds_if(lds > 65536, kern, grid, dim3(NT * FR), lds, st, v, g, tb, wa, ws, Mk, seg, fpb);
}

#define SG_CZT_SWITCH(M_, CALL)            \
  switch (M_) {                            \
    case 64: return CALL(64);              \
    case 128: return CALL(128);            \
    case 256: return CALL(256);            \
    case 512: return CALL(512);            \
    case 1024: return CALL(1024);          \
    case 2048: return CALL(2048);          \
    case 4096: return CALL(4096);          \
    case 8192: return CALL(8192);          \
  }                                        \
  return hipErrorInvalidValue

template <typename TC>
static CztTabs<TC> czt_tabs(const sg_handle* h) {
  if (sizeof(TC) == 8)
    return {(const cx<TC>*)h->czt_tw64.p, (const cx<TC>*)h->czt_ch64.p, (const cx<TC>*)h->czt_bh64.p};
  return {(const cx<TC>*)h->czt_tw32.p, (const cx<TC>*)h->czt_ch32.p, (const cx<TC>*)h->czt_bh32.p};
}

// ------------------------------------------------------------------------------------------
// long frames (big.hpp): four-step transform through HBM, frames in batches of <= 256 MB of work buffer
// ------------------------------------------------------------------------------------------
static big::BigTabs big_tabs(const sg_handle* h) {
  return big::BigTabs{(const big::cd*)h->big_twM.p, (const big::cd*)h->big_tw2.p, (const big::cd*)h->big_ch.p,
                      (const big::cd*)h->big_bh.p, h->big_M, h->big_M / 16, h->big_czt};
}

template <int M2>
static hipError_t big_rows_m2(big::cd* W, const big::BigTabs& tb, int64_t nf, int mode, hipStream_t st) {
  const size_t lds = (size_t)lpn<double>(M2) * sizeof(big::cd);
  auto go = [&](auto kern) -> hipError_t {
    return launch_lds_if(lds > 65536, kern, dim3((unsigned)(nf * 16)), dim3(256), lds, st, W, tb, nf);
  };
  if (mode == 0) return go(big::k_big_rows<M2, false, false>);
  if (mode == 1) return go(big::k_big_rows<M2, true, false>);
  return go(big::k_big_rows<M2, false, true>);
}

// mode 0: forward rows, 1: inverse rows, 2: forward rows x B then inverse rows (chirp-z)
static hipError_t big_rows(big::cd* W, const big::BigTabs& tb, int64_t nf, int mode, hipStream_t st) {
  switch (tb.M2) {
    case 1024: return big_rows_m2<1024>(W, tb, nf, mode, st);
    case 2048: return big_rows_m2<2048>(W, tb, nf, mode, st);
    case 4096: return big_rows_m2<4096>(W, tb, nf, mode, st);
  }
  return hipErrorInvalidValue;
}

// the length-n DFT of the staged frames: natural order in; out = permuted bins (power of two) or the chirp-z
// convolution in natural order
static hipError_t big_dft(big::cd* W, const big::BigTabs& tb, int64_t nf, hipStream_t st) {
  const dim3 gc((unsigned)((tb.M2 + 255) / 256), (unsigned)nf);
  hipLaunchKernelGGL(big::k_big_cols<false>, gc, dim3(256), 0, st, W, tb, nf);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = big_rows(W, tb, nf, tb.czt ? 2 : 0, st)) != hipSuccess) return e;
  if (tb.czt) {
    hipLaunchKernelGGL(big::k_big_cols<true>, gc, dim3(256), 0, st, W, tb, nf);
    e = hipGetLastError();
  }
  return e;
}

static int64_t big_batch(const sg_handle* h, int64_t total) {
  const int64_t per = (int64_t)h->big_M * (int64_t)sizeof(big::cd);
  return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(total, 32768), ((int64_t)256 << 20) / per));
}

static int big_stft(sg_handle* h, const View& v, const Geom& g, int64_t units, double* P, float* mag, double* z,
                    double zscale, hipStream_t st, unsigned long long* pmax_bits) {
  const big::BigTabs tb = big_tabs(h);
  const int64_t total = units * g.T, nb = big_batch(h, total);
  int rc = ensure(h, h->big_W, (size_t)nb * tb.M * sizeof(big::cd));
  if (rc) return rc;
  big::cd* W = (big::cd*)h->big_W.p;
  for (int64_t f0 = 0; f0 < total; f0 += nb) {
    const int64_t nf = std::min(nb, total - f0);
    hipLaunchKernelGGL(big::k_big_frames, dim3(64, (unsigned)nf), dim3(256), 0, st, v, g, tb, (const double*)h->wfull64.p,
                       W, f0, nf);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, big_dft(W, tb, nf, st));
    hipLaunchKernelGGL(big::k_big_out, dim3((unsigned)std::min<int64_t>(32, (g.F + 255) / 256), (unsigned)nf), dim3(256), 0,
                       st, (const big::cd*)W, g, tb, f0, nf, P, mag, z, zscale, pmax_bits);
    HIPCHK(h, hipGetLastError());
  }
  return SG_OK;
}

template <typename TM, typename TS>
static int big_apply(sg_handle* h, const View& v, const Geom& g, int64_t units, const TM* Mk, TS* seg,
                     hipStream_t st) {
  const big::BigTabs tb = big_tabs(h);
  const int64_t total = units * g.T, nb = big_batch(h, total);
  int rc = ensure(h, h->big_W, (size_t)nb * tb.M * sizeof(big::cd));
  if (!rc) rc = ensure(h, h->big_W2, (size_t)nb * tb.M * sizeof(big::cd));
  if (rc) return rc;
  big::cd *W = (big::cd*)h->big_W.p, *W2 = (big::cd*)h->big_W2.p;
  for (int64_t f0 = 0; f0 < total; f0 += nb) {
    const int64_t nf = std::min(nb, total - f0);
    hipLaunchKernelGGL(big::k_big_frames, dim3(64, (unsigned)nf), dim3(256), 0, st, v, g, tb, (const double*)h->wfull64.p,
                       W, f0, nf);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, big_dft(W, tb, nf, st));
    hipLaunchKernelGGL(big::k_big_mask<TM>, dim3(64, (unsigned)nf), dim3(256), 0, st, (const big::cd*)W, W2, g, tb, f0, nf, Mk);
    HIPCHK(h, hipGetLastError());
    if (tb.czt) {
      HIPCHK(h, big_dft(W2, tb, nf, st));   // inverse DFT = forward chirp-z of conj(Y), conjugated
    } else {
      HIPCHK(h, big_rows(W2, tb, nf, 1, st));
      hipLaunchKernelGGL(big::k_big_cols<true>, dim3((unsigned)((tb.M2 + 255) / 256), (unsigned)nf), dim3(256), 0, st, W2,
                         tb, nf);
      HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(big::k_big_seg<TS>, dim3(64, (unsigned)nf), dim3(256), 0, st, (const big::cd*)W2, g, tb, f0, nf,
                       (const double*)h->wfull64.p, seg);
    HIPCHK(h, hipGetLastError());
  }
  return SG_OK;
}

// forward STFT of `units` units on the kernels that fit the handle's frame length
template <typename TC>
static hipError_t stft_any(const sg_handle* h, const View& v, const Geom& g, int64_t units, double* P, float* mag,
                           double* z, double zscale, hipStream_t st, unsigned long long* pmax_bits = nullptr) {
  if (h->big_M) {
    const int rc = big_stft(const_cast<sg_handle*>(h), v, g, units, P, mag, z, zscale, st, pmax_bits);
    return rc == SG_OK ? hipSuccess : (rc == SG_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown);
  }
  const void* wfull = sizeof(TC) == 8 ? h->wfull64.p : h->wa32.p;
  if (sizeof(TC) == 8 && h->fast_ok && !h->force_nofast && P && !mag && !z && units * ((g.T + 15) / 16) >= 512) {
    // default geometry, float64 powers only, enough 16-frame blocks for two per CU: register FFT
    // core (fast64.hpp).  (A single noise clip is faster on k_stft's one-frame-per-wave grid: 13.7 vs 18 us.)
    // Samples staged as float32 where that is exact (float32 / int16 recordings), as float64 otherwise.
    constexpr int WAVES = 4;
    fast::Pow64Args A{v, g, (const double*)h->wfull64.p, (const fast::cd*)h->tw64.p, P, pmax_bits};
    const size_t lds = (size_t)(fast::FN + WAVES * 4 * fast::FSLOTS_D + 32) * sizeof(fast::cd);
    dim3 grid((unsigned)((g.T + WAVES * 4 - 1) / (WAVES * 4)), (unsigned)units);
    auto go = [&](auto kern) -> hipError_t {
      return launch_lds(kern, grid, dim3(WAVES * 64), lds, st, A);
    };
    if (v.dtype == SG_F32 || v.dtype == SG_I16)
      return pmax_bits ? go(fast::k_power_fast64<WAVES, true>) : go(fast::k_power_fast64<WAVES, false>);
    return pmax_bits ? go(fast::k_power_fast64<WAVES, true, double>) : go(fast::k_power_fast64<WAVES, false, double>);
  }
  if (!h->czt_M) {
    const void* tw = sizeof(TC) == 8 ? h->tw64.p : h->tw32.p;
    return launch_stft<TC>(h->N, v, g, units, tw, wfull, P, mag, z, zscale, st, pmax_bits);
  }
  if (h->mr_ok) return launch_stft_mr<TC>(h, v, g, units, wfull, P, mag, z, zscale, st, pmax_bits);
  const CztTabs<TC> tb = czt_tabs<TC>(h);
#define SG_CALL(M) launch_stft_czt_m<TC, M>(v, g, units, tb, wfull, P, mag, z, zscale, st, pmax_bits)
  SG_CZT_SWITCH(h->czt_M, SG_CALL);
#undef SG_CALL
}

static hipError_t apply_any(const sg_handle* h, const View& v, const Geom& g, int64_t units, const float* Mk,
                            float* seg, hipStream_t st, const unsigned short* K16 = nullptr, float kscale = 0.f) {
  if (h->big_M) {
    const int rc = big_apply(const_cast<sg_handle*>(h), v, g, units, Mk, seg, st);
    return rc == SG_OK ? hipSuccess : (rc == SG_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown);
  }
  const float* wa = (const float*)h->wa32.p;
  const float* ws = (const float*)h->ws32.p;
  if (!h->czt_M) return launch_apply(h->N, v, g, units, h->tw32.p, wa, ws, Mk, seg, st, K16, kscale);
  if (h->mr_ok) return launch_apply_mr(h, v, g, units, wa, ws, Mk, seg, st, K16, kscale);
  const CztTabs<float> tb = czt_tabs<float>(h);
#define SG_CALL(M) launch_apply_czt_m<M>(v, g, units, tb, wa, ws, Mk, seg, st)
  SG_CZT_SWITCH(h->czt_M, SG_CALL);
#undef SG_CALL
}

static DbFast db_fast_consts(const sg_handle* h) {
  const double eps = 2.220446049250313e-16;
  const double ymin = eps * 134217728.0 / h->mag_scale;   // eps 2^27 / mag_scale
  return DbFast{(const double*)h->logtab.p, 20.0 * std::log10(h->mag_scale), ymin * ymin, eps / h->mag_scale};
}

static unsigned grid_1d(int64_t work, int block) {
  int64_t b = (work + block - 1) / block;
  return (unsigned)std::min<int64_t>(std::max<int64_t>(b, 1), 256 * 32);
}

// ------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------
// Workspace per unit, for the callers that plan no route (variant T, the backward passes).  lean: the fused stationary path with
// the fused apply kernel only keeps the bit mask (T*wpr*8 B) and the uint16 weight sums (T*FS*2 B).  route.hpp's unit_bytes, which
// sizes run_S's batches and sg_workspace_bytes, states the same bytes for a RouteShape: asserted below.
static constexpr size_t unit_bytes(const sg_handle* h, const Geom& g, bool lean) {
  size_t cells = (size_t)g.T * g.FS;
  if (lean) return (size_t)g.T * ((g.F + 63) / 64) * 8 + cells * 2 + (size_t)g.FS * 16 + 64 +
           (size_t)(g.T / 16 + 2) * 6 * 256 * 4;
  return cells * (8 + 4 + 4 + 2) + (size_t)g.T * g.n * 4 + (size_t)g.FS * 16 +
         (size_t)(g.T / NS_TT + 1) * 2 * g.FS * 8 * 2 +  // + partials and carries of the two-pass non-stationary mask
         (size_t)(g.T / 8 + 1) * 2 * g.FS * 8;           // + the magnitude kernels' per-tile partials (tiles of 8 frames at n_fft = 2048)
}
constexpr bool unit_bytes_agree(int n, int64_t T) {
  Geom g{};
  g.n = n; g.F = n / 2 + 1; g.FS = (g.F + 15) / 16 * 16; g.T = T;
  route::RouteShape s;
  s.n = g.n; s.F = g.F; s.FS = g.FS; s.T = g.T;
  return unit_bytes(nullptr, g, false) == route::unit_bytes(s, false) && unit_bytes(nullptr, g, true) == route::unit_bytes(s, true);
}
static_assert(unit_bytes_agree(1024, 2579) && unit_bytes_agree(256, 7) && unit_bytes_agree(2048, 65) && unit_bytes_agree(1000, 128),
              "route.hpp and api.hip state the same bytes per unit");

static int64_t units_per_batch(const sg_handle* h, const Geom& g, int64_t total, bool lean = false) {
  int64_t ub = ws_budget(h) / (int64_t)unit_bytes(h, g, lean);
  ub = std::max<int64_t>(1, std::min<int64_t>(ub, 32768));
  return std::min(ub, total);
}

static int ensure_ws(sg_handle* h, const Geom& g, int64_t ub, bool lean = false) {
  size_t cells = (size_t)ub * g.T * g.FS;
  int rc;
  if (!lean) {
    if ((rc = ensure(h, h->P, cells * 8))) return rc;  // power (f64) or magnitude (f32)
    if ((rc = ensure(h, h->raw, cells * 4))) return rc;
    if ((rc = ensure(h, h->M, cells * 4))) return rc;
    if ((rc = ensure(h, h->seg, std::max((size_t)ub * g.T * g.n * 4, cells * 4)))) return rc;
  }
  if ((rc = ensure(h, h->pmax, (size_t)ub * g.FS * 8))) return rc;
  if ((rc = ensure(h, h->thr_rows, (size_t)ub * g.FS * 8))) return rc;
  return SG_OK;
}

// ------------------------------------------------------------------------------------------
// pipeline pieces (all enqueue on `st`)
// ------------------------------------------------------------------------------------------
// time slices for the column statistics: enough blocks to fill 256 CUs even for one unit
#ifndef SG_STAT_SLICES_MAX
#define SG_STAT_SLICES_MAX 64
#endif
#ifndef SG_STAT_FRAMES_PER_SLICE
#define SG_STAT_FRAMES_PER_SLICE 36   // k_colstats1 (stage_stats)
#endif
static int stat_slices(const Geom& g, int64_t ub) {
  int64_t blocks = (int64_t)((g.F + 63) / 64) * ub;
  int64_t nts = (2048 + blocks - 1) / blocks;
  nts = std::max<int64_t>(1, std::min<int64_t>(nts, std::min<int64_t>(SG_STAT_SLICES_MAX, std::max<int64_t>(1, g.T / 16))));
  return (int)nts;
}

// power field + column max of a batch of units
static int stage_power(sg_handle* h, const View& v, const Geom& g, int64_t ub, hipStream_t st) {
  if (ub >= 16) {
    // power field; the per-(unit, band) maximum is folded into the STFT kernel (atomic max: one
    // address per (unit, band), little contention when there are many units)
    HIPCHK(h, hipMemsetAsync(h->pmax.p, 0, (size_t)ub * g.FS * 8, st));
    ProfScope ps(h, SG_STAGE_STFT_POWER, st);
    HIPCHK(h, stft_any<double>(h, v, g, ub, (double*)h->P.p, nullptr, nullptr, 1.0, st,
                               (unsigned long long*)h->pmax.p));
    return SG_OK;
  }
  // few units (the noise clip): thousands of frames would hammer the same 513 addresses; reduce
  // the maximum with the two-stage column kernels instead
  {
    ProfScope ps(h, SG_STAGE_STFT_POWER, st);
    HIPCHK(h, stft_any<double>(h, v, g, ub, (double*)h->P.p, nullptr, nullptr, 1.0, st));
  }
  ProfScope ps(h, SG_STAGE_COLMAX, st);
  const int nts = stat_slices(g, ub);
  int rc = ensure(h, h->part, (size_t)ub * nts * 2 * g.FS * 8);
  if (rc) return rc;
  dim3 grid((g.F + 63) / 64, (unsigned)ub, nts);
  hipLaunchKernelGGL(k_colmax, grid, dim3(64 * STAT_TG), 0, st, (const double*)h->P.p, g, (double*)h->part.p);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_colmax_final, dim3(grid_1d(ub * g.FS, 256)), dim3(256), 0, st, (const double*)h->part.p, g,
                     nts, (double*)h->pmax.p, ub);
  HIPCHK(h, hipGetLastError());
  return SG_OK;
}

static int stage_colstats(sg_handle* h, const Geom& g, int64_t ub, double* thresh_out, hipStream_t st) {
  ProfScope ps(h, SG_STAGE_COLSTATS, st);
  const int nts = stat_slices(g, ub);
  int rc = ensure(h, h->part, (size_t)ub * nts * 2 * g.FS * 8);
  if (rc) return rc;
  dim3 grid((g.F + 63) / 64, (unsigned)ub, nts);
  hipLaunchKernelGGL(k_colstats, grid, dim3(64 * STAT_TG), 0, st, (const double*)h->P.p, g,
                     (const double*)h->pmax.p, h->mag_scale, h->p.top_db, (double*)h->part.p);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_colstats_final, dim3(grid_1d(ub * g.FS, 256)), dim3(256), 0, st,
                     (const double*)h->part.p, g, nts, (const double*)h->pmax.p, h->mag_scale,
                     h->p.n_std_thresh, h->p.ddof, thresh_out, ub);
  HIPCHK(h, hipGetLastError());
  return SG_OK;
}

// Noise statistics in two launches (k_noise_moments + k_colstats1_final on 16-band workgroups): one noise clip of a register
// geometry.  A slice is the TEAMS - 1 frames of one k_noise_moments workgroup, and the final stage holds at most
// NM_TG * (64 / NM_BW) * NM_MAXS = 256 slices in registers; clips beyond that keep the three launches (n_fft = 2048, whose 256-thread
// teams leave 3 frames per slice: beyond 768 frames).  Below 512 frames the three-launch route stays too: its slicing
// is what the short statistics clips of the tests were built against, and one round of workgroups has nothing to gain there.
constexpr int NM_TG = 4;       // wavefronts of the final stage's workgroup
constexpr int NM_BW = 16;      // bands of the final stage's workgroup: 4 slice groups per wavefront
constexpr int NM_MAXS = 16;    // slices per thread
constexpr int NM_MIN_FRAMES = 512;
template <int N>
constexpr int nm_team_threads() { return N >= 1024 ? 256 : team_threads<N>(); }   // (n_fft = 2048: the whole-workgroup shape of launch_stft_n)
template <int N>
constexpr int nm_frames_per_slice() { return 1024 / nm_team_threads<N>() - 1; }
static int nm_fps(int N) {
  switch (N) {
    case 128: return nm_frames_per_slice<128>();
    case 256: return nm_frames_per_slice<256>();
    case 512: return nm_frames_per_slice<512>();
    case 1024: return nm_frames_per_slice<1024>();
  }
  return 0;
}
static bool stats_two_launch(const sg_handle* h, const Geom& g, int64_t ub) {
  if (h->stats_three || ub != 1 || h->p.variant != SG_VARIANT_S || !(h->fast_ok || h->reg) || h->big_M || h->czt_M) return false;
  const int fps = nm_fps(h->N);
  return fps > 0 && g.T >= NM_MIN_FRAMES && (g.T + fps - 1) / fps <= NM_TG * (64 / NM_BW) * NM_MAXS;
}
template <int N>
static hipError_t launch_noise_moments_n(const sg_handle* h, const View& v, const Geom& g, int nts, hipStream_t st,
                                         unsigned* alim_b, int n_alim) {
  constexpr int NT = nm_team_threads<N>(), TEAMS = 1024 / NT;
  const size_t lds = (size_t)(N + TEAMS * lpn<double>(N)) * sizeof(cx<double>);
  auto kern = k_noise_moments<N, NT, TEAMS>;
  return launch_lds(kern, dim3((unsigned)nts, 1), dim3(TEAMS * NT), lds, st, v, g, (const cx<double>*)h->tw64.p,
                    (const double*)h->wfull64.p, (double*)h->P.p, h->mag_scale, (double*)h->part.p, db_fast_consts(h),
                    alim_b, n_alim);
}
static hipError_t launch_noise_moments(const sg_handle* h, const View& v, const Geom& g, int nts, hipStream_t st,
                                       unsigned* alim_b, int n_alim) {
  switch (h->N) {
    case 128: return launch_noise_moments_n<128>(h, v, g, nts, st, alim_b, n_alim);
    case 256: return launch_noise_moments_n<256>(h, v, g, nts, st, alim_b, n_alim);
    case 512: return launch_noise_moments_n<512>(h, v, g, nts, st, alim_b, n_alim);
    case 1024: return launch_noise_moments_n<1024>(h, v, g, nts, st, alim_b, n_alim);
  }
  return hipErrorInvalidValue;
}

// power field + band statistics -> threshold
static int stage_stats(sg_handle* h, const View& v, const Geom& g, int64_t ub, double* thresh_out, hipStream_t st,
                       bool gate_consts = false) {
  if (ub < 16 && stats_two_launch(h, g, ub)) {
    // one noise clip of a register geometry: transform + slice partials -> final (2 launches instead of 3)
    const int fps = nm_fps(h->N);
    const int nts = (int)((g.T + fps - 1) / fps);
    int rc = ensure(h, h->part, (size_t)nts * STAT1_NP * g.FS * 8);
    if (rc) return rc;
    GateConsts gc{};
    if (gate_consts && (g.FS + 63) / 64 <= 62) {
      if ((rc = ensure(h, h->T2, (size_t)g.FS * 8))) return rc;
      if ((rc = ensure_zeroed(h, h->alim, 256, st))) return rc;
      gc.T2 = (double*)h->T2.p; gc.alim_b = (unsigned*)h->alim.p + 2; gc.sum_abs_w = h->sum_abs_w;
    }
    {
      ProfScope ps(h, SG_STAGE_STFT_POWER, st);
      HIPCHK(h, launch_noise_moments(h, v, g, nts, st, gc.alim_b, (g.FS + 63) / 64));
    }
    ProfScope ps(h, SG_STAGE_COLSTATS, st);
    hipLaunchKernelGGL((k_colstats1_final<NM_TG, true, NM_BW, NM_MAXS>), dim3((unsigned)((g.FS + NM_BW - 1) / NM_BW), 1), dim3(64 * NM_TG), 0, st,
                       (const double*)h->part.p, (const double*)h->P.p, g, nts, h->mag_scale, h->p.top_db,
                       h->p.n_std_thresh, h->p.ddof, (double*)h->pmax.p, thresh_out, gc, fps);
    HIPCHK(h, hipGetLastError());
    if (gc.T2 != nullptr) h->t2_ready = true;
    h->stats_route = SG_STATS_TWO_LAUNCH;
    return SG_OK;
  }
  if (ub < 16) {
    // few units (the noise clip): STFT -> one pass over the power field -> final (3 launches instead of 5)
    h->stats_route = SG_STATS_THREE_LAUNCH;
    {
      ProfScope ps(h, SG_STAGE_STFT_POWER, st);
      HIPCHK(h, stft_any<double>(h, v, g, ub, (double*)h->P.p, nullptr, nullptr, 1.0, st));
    }
    ProfScope ps(h, SG_STAGE_COLSTATS, st);
    // (round 6) at least SG_STAT_FRAMES_PER_SLICE frames per slice, at most 64 slices.  Measured (k_colstats1 + k_colstats1_final, us):
    // n_fft = 1024 (T = 2345): 64 slices 8.0 + 8.3, 32 slices 9.9 + 8.8; n_fft = 2048 (T = 1172): 32 slices 8.1 + 7.3, 16 slices 10.5 + 7.3,
    // 64 slices 9.6 + 7.3.  (Before k_colstats1_final loaded its partials unconditionally it paid 0.08 us per slice: 13.2 us at 64.)
    const int nts = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(stat_slices(g, ub), STAT_TG * STAT1_MAXS), g.T / SG_STAT_FRAMES_PER_SLICE));
    int rc = ensure(h, h->part, (size_t)ub * nts * STAT1_NP * g.FS * 8);
    if (rc) return rc;
    dim3 grid((g.F + 63) / 64, (unsigned)ub, nts);
    hipLaunchKernelGGL(k_colstats1, grid, dim3(64 * STAT_TG), 0, st, (const double*)h->P.p, g, h->mag_scale,
                       (double*)h->part.p, db_fast_consts(h));
    HIPCHK(h, hipGetLastError());
    // (for the stationary gate's noise statistics the final kernel also derives the gate's compare constants: no
    // k_prep_thresh_lazy launch in the calls that follow)
    // (round 6: the final stage INSIDE k_colstats1 -- run by the last workgroup of a band block to finish its slice -- measured:
    // with __threadfence() around the arrival counter + 43 us per call, a device-scope release writes back the L2; fence-free
    // (partials as sc1 stores, s_waitcnt vmcnt(0), counter, sc1 loads) + 2 / - 1 / + 0.5 / + 4 us at n_fft = 1024 / 256 / 512 /
    // 2048: what the launch boundary costs the last arriver pays in memory round trips.  DESIGN 8, profiles/r06_stats_fused_ab.txt)
    GateConsts gc{};
    if (gate_consts && ub == 1 && grid.x <= 62) {   // (one bound per 64-band block: 9 at n_fft = 1024, 33 at 4096)
      if ((rc = ensure(h, h->T2, (size_t)g.FS * 8))) return rc;
      if ((rc = ensure_zeroed(h, h->alim, 256, st))) return rc;
      gc.T2 = (double*)h->T2.p; gc.alim_b = (unsigned*)h->alim.p + 2; gc.sum_abs_w = h->sum_abs_w;
    }
    hipLaunchKernelGGL((k_colstats1_final<STAT_TG, false>), dim3((unsigned)((g.FS + 63) / 64), (unsigned)ub), dim3(64 * STAT_TG), 0, st,
                       (const double*)h->part.p, (const double*)h->P.p, g, nts, h->mag_scale, h->p.top_db,
                       h->p.n_std_thresh, h->p.ddof, (double*)h->pmax.p, thresh_out, gc, 0);
    HIPCHK(h, hipGetLastError());
    if (gc.T2 != nullptr) h->t2_ready = true;
    return SG_OK;
  }
  int rc = stage_power(h, v, g, ub, st);
  if (rc) return rc;
  return stage_colstats(h, g, ub, thresh_out, st);
}

static int stage_decide(sg_handle* h, const Geom& g, int64_t ub, const double* thresh, int64_t ustride,
                        hipStream_t st) {
  ProfScope ps(h, SG_STAGE_DECIDE, st);
  int64_t cells = ub * g.T * g.FS;
  hipLaunchKernelGGL(k_decide, dim3(grid_1d(cells, 256)), dim3(256), 0, st, (const double*)h->P.p, g,
                     (const double*)h->pmax.p, thresh, ustride, h->mag_scale, h->p.top_db, (float*)h->raw.p, ub);
  HIPCHK(h, hipGetLastError());
  return SG_OK;
}

// Hand-offs between workgroups of one launch (tagged granules, bounded polls): the host-mapped error word, the
// verdict on earlier launches, a fresh epoch.  Granule buffers are zero when (re)allocated and the epoch only grows:
// a fresh granule never carries it.
// A new tag for the granules of the next hand-off launch (a call that launches twice takes two).
static int handoff_next_epoch(sg_handle* h, hipStream_t st) {
  if (++h->epoch == 0) {  // wrapped: tags of 2^32 launches ago could alias
    if (h->xbits.p) HIPCHK(h, hipMemsetAsync(h->xbits.p, 0, h->xbits.bytes, st));
    if (h->xpart.p) HIPCHK(h, hipMemsetAsync(h->xpart.p, 0, h->xpart.bytes, st));
    if (h->farrive.p) HIPCHK(h, hipMemsetAsync(h->farrive.p, 0, h->farrive.bytes, st));
    h->epoch = 1;
    if (h->err_host) h->err_host[1] = 0u;   // the floor-test stamp is an epoch too
  }
  return SG_OK;
}

static int handoff_prepare(sg_handle* h, hipStream_t st) {
  {
    // The work counter is never reset: every launch takes exactly its grid size in tickets, the kernels subtract
    // the running base.
    bool fresh = false;
    int rc = ensure_zeroed(h, h->xticket, 64, st, &fresh);
    if (rc) return rc;
    if (fresh) h->ticket_base = 0;
  }
  if (!h->err_host) {
    HIPCHK(h, hipHostMalloc((void**)&h->err_host, 64, hipHostMallocMapped));
    *h->err_host = 0u;
    h->err_host[1] = 0u;   // floor-test stamp (onepass_run)
    HIPCHK(h, hipHostGetDevicePointer((void**)&h->err_dev, h->err_host, 0));
  }
  if (*h->err_host != 0u) {
    // only reached by callers that never synchronise through the library (sg_check_errors and every synchronising
    // entry point report a lost hand-off for the call that suffered it)
    const unsigned e = *h->err_host;
    *h->err_host = 0u;
    FAIL(h, SG_E_HANDOFF, "a tile hand-off of an EARLIER call on this handle timed out (code %u): that call's output "
                          "is invalid (call sg_check_errors after a call to learn about it in time)", e);
  }
  h->lose_now = 0;
  if (h->inject_fault) {  // test hook: this launch "loses" a hand-off
    *h->err_host = h->inject_fault & 7u;          // bits 0..2: reported only (the output is fine)
    h->lose_now = (h->inject_fault >> 3) & 15u;   // bits 3..6: lost INSIDE the kernel (the output is poisoned)
    h->inject_fault = 0;
  }
  return handoff_next_epoch(h, st);
}

// After the stream has been synchronised: did a hand-off of the work just completed time out?
int sg::host::handoff_verdict(sg_handle* h) {
  if (h->err_host && *h->err_host != 0u) {
    const unsigned e = *h->err_host;
    *h->err_host = 0u;
    FAIL(h, SG_E_HANDOFF, "a tile hand-off timed out (code %u: %s%s%s): the output of the call(s) enqueued since the "
                          "last check is invalid; re-run them (SG_OPT_FORCE_SPLIT + SG_OPT_FORCE_NOLEAN select the "
                          "kernels without in-launch hand-offs)",
         e, (e & 1u) ? "mask bits " : "", (e & 2u) ? "partial hops (one-pass gate) " : "",
         (e & 4u) ? "partial hops (fused apply)" : ((e & 8u) ? "band maxima (floor fix-up)" : ""));
  }
  return SG_OK;
}

extern "C" int sg_check_errors(sg_handle* h, void* stream) {
  if (!h) return SG_E_INVALID;
  HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
  return handoff_verdict(h);
}

// (defined next to the decision kernels' other stages, below)
static int stage_prep_floor(sg_handle* h, const View& v, const Geom& g, int64_t ub, ThreshConsts* tc_out, hipStream_t st,
                            const View* v_exact, unsigned* live_host, unsigned stamp);

// ------------------------------------------------------------------------------------------
// stages of the register geometries (n_fft = 512 / 256 / 2048): each reads the handle's RegGeom
// ------------------------------------------------------------------------------------------
static fast::RegArgs reg_args(const sg_handle* h, const RegGeom* r, const View& v, const Geom& g) {
  fast::RegArgs A{};
  A.view = v; A.g = g;
  A.win = (const float*)h->wa32.p;
  A.win64 = (const double*)h->wfull64.p;
  A.tw = (const fast::cf*)(h->*r->tw).p;
  A.tw64 = (const cx<double>*)h->tw64.p;
  A.mag_scale = h->mag_scale; A.top_db = h->p.top_db;
  A.wsq = (const float*)h->wsq32.p;
  A.invn = (const float*)h->invn.p;
  return A;
}

static int stage_decide_reg(sg_handle* h, const RegGeom* r, const View& v, const Geom& g, int64_t ub, const ThreshConsts& tc,
                            unsigned long long* bits, hipStream_t st, const FloorLazy& fl = FloorLazy{}, bool redo = false) {
  ProfScope ps(h, redo ? SG_STAGE_STFT_MAX : SG_STAGE_DECIDE_FAST, st);   // (the early-exit second launch is booked with the pre-pass)
  fast::RegArgs A = reg_args(h, r, v, g);
  A.tc = tc;
  A.bits = bits;
  A.fl = fl;
  HIPCHK(h, launch_lds(r->decide[redo], dim3((unsigned)((g.T + r->frames - 1) / r->frames), (unsigned)ub), dim3(256), r->lds, st, A));
  return SG_OK;
}

static int stage_mag_reg(sg_handle* h, const RegGeom* r, const View& v, const Geom& g, int64_t ub, float* mag, hipStream_t st,
                         double iir_b, double* sub /* per-tile recurrence partials (mag_sub_partials) */) {
  ProfScope ps(h, SG_STAGE_STFT_MAG, st);
  fast::RegArgs A = reg_args(h, r, v, g);
  A.mag = mag;
  A.iir_b = iir_b;
  A.sub = sub;
  HIPCHK(h, launch_lds(r->mag, dim3((unsigned)((g.T + r->frames - 1) / r->frames), (unsigned)ub), dim3(256), r->lds, st, A));
  return SG_OK;
}

// seam hops of abutting apply / one-pass tiles (fastpath.hpp: k_ola_seam)
static int launch_seam(sg_handle* h, const RegGeom* r, const fast::RegArgs& A, int64_t ub, hipStream_t st) {
  if (A.n_tiles < 2) return SG_OK;
  fast::SeamArgs S{};
  S.view = A.view; S.g = A.g; S.om = A.om; S.h_begin = A.h_begin; S.h_end = A.h_end; S.normalize = A.normalize;
  S.invn = A.invn; S.wsq = A.wsq; S.part = A.part; S.n_tiles = A.n_tiles;
  hipLaunchKernelGGL(r->seam, dim3((unsigned)(A.n_tiles - 1), (unsigned)ub), dim3(r->hop), 0, st, S);
  HIPCHK(h, hipGetLastError());
  return SG_OK;
}

// abutting tiles over nh hops + their seam partials in h->seam
static int reg_seam_tiles(sg_handle* h, const RegGeom* r, int64_t nh, int64_t ub, fast::RegArgs* A) {
  const int64_t tiles = abutting_tiles(nh, r->frames);
  int rc = ensure(h, h->seam, (size_t)ub * tiles * 6 * r->hop * sizeof(float));
  if (rc) return rc;
  A->part = (float*)h->seam.p;
  A->n_tiles = (int)tiles;
  return SG_OK;
}

static int stage_apply_reg(sg_handle* h, const RegGeom* r, const View& v, const Geom& g, int64_t ub, const OutMap& om,
                           const float* mask_f /* nullptr: uint16 weight sums in h->K16 (natural bin order) */,
                           int normalize, hipStream_t st) {
  ProfScope ps(h, SG_STAGE_APPLY_FAST, st);
  fast::RegArgs A = reg_args(h, r, v, g);
  A.Mf = mask_f;
  A.K = (const unsigned short*)h->K16.p;
  A.inv_ktot = (float)(1.0 / (double)h->ktot);
  A.om = om;
  A.normalize = normalize;
  const HopRange hr = hop_range(om, g, r->hop);
  A.h_begin = hr.h_begin;
  A.h_end = hr.h_end;
  const int64_t nh = hr.count();
  if (nh <= 0) return SG_OK;
  // (round 6) abutting tiles; the 3 hops that straddle two tiles as partial sums + k_ola_seam (fastpath.hpp)
  const int64_t tiles = abutting_tiles(nh, r->frames);
  const bool seam = tiles >= 2 && !h->force_noseam;
  A.n_tiles = (int)tiles;
  int rc;
  if (seam && (rc = reg_seam_tiles(h, r, nh, ub, &A))) return rc;
  const dim3 grid((unsigned)(seam ? tiles : (nh + r->hops - 1) / r->hops), (unsigned)ub);
  HIPCHK(h, launch_lds(r->apply[mask_f == nullptr], grid, dim3(256), r->lds, st, A));
  if (seam) return launch_seam(h, r, A, ub, st);
  return SG_OK;
}

// Floor test of a gate call (is some band's -top_db floor possibly live?): a priori -- k_unit_absmax reads the recording once
// more (stage_prep_floor: 26 us of a 345 us call at 10 minutes of 48 kHz) -- or in the gate / decision kernels on the samples
// they stage (onepass.hpp "floor test"), which costs nothing unless a unit reports; then that unit is gated twice.  Both are
// exact; the choice is a prediction from the host-mapped stamp "a unit of launch <epoch> reported / had its flag set", read
// WITHOUT synchronising (it may lag by the calls still queued): recent -> a priori.  Opens the call's hand-off epoch first
// (the floor test stamps err_host[1] with it).  lazy: tc / fl hold the in-kernel test's constants (k_prep_thresh_lazy writes
// `nb` bounds when the threshold did not come from sg_noise_stats); otherwise the caller runs stage_prep_floor.
struct FloorSetup {
  bool lazy = false;
  ThreshConsts tc{};
  FloorLazy fl{};
};
static int floor_setup(sg_handle* h, const Geom& g, int64_t ub, int nb, hipStream_t st, FloorSetup* out) {
  int rc;
  if ((rc = handoff_prepare(h, st))) return rc;
  const unsigned live_stamp = h->err_host[1];
  // the flags the tiles raise are tagged with this launch's epoch (30 bits; 0 = untagged): nothing to clear per call
  const unsigned need_tag = h->epoch & 0x3fffffffu;
  // Once per 2^30 launches the tag wraps: flags of the previous era carry LARGER tags, which atomicMax would keep.  Not
  // every epoch reaches this function (a lazy call takes two, stage_apply_fast takes its own), so the crossing is
  // detected by the era (epoch >> 30) changing between two calls here, not by need_tag == 0.
  const unsigned era = h->epoch >> 30;
  if (era != h->need_era || need_tag == 0u) {
    if (h->need.p) HIPCHK(h, hipMemsetAsync(h->need.p, 0, h->need.bytes, st));
    if (h->alim.p) HIPCHK(h, hipMemsetAsync((char*)h->alim.p + 4, 0, 4, st));
    h->need_era = era;
  }
  FloorSetup f;
  f.lazy = need_tag != 0u &&
           (h->floor_test == 2 || (h->floor_test == 0 && !(live_stamp != 0u && h->epoch - live_stamp <= 16u)));
  if (f.lazy) {
    const int wpr = (g.F + 63) / 64;
    if ((rc = ensure(h, h->bits, (size_t)ub * g.T * wpr * 8))) return rc;
    if ((rc = ensure_zeroed(h, h->need, (size_t)ub * 4, st))) return rc;
    if ((rc = ensure(h, h->T2, (size_t)g.FS * 8))) return rc;
    if ((rc = ensure_zeroed(h, h->alim, 256, st))) return rc;
    if (!h->t2_ready) {
      // the threshold did not come from sg_noise_stats (whose last kernel derives T2 / alim itself): one small launch
      ProfScope ps(h, SG_STAGE_PREP, st);
      hipLaunchKernelGGL(k_prep_thresh_lazy, dim3(1), dim3(256), 0, st, (const double*)h->thresh.p, g.F, h->mag_scale,
                         h->sum_abs_w, h->p.top_db, (double*)h->T2.p, (unsigned*)h->alim.p, nb);
      HIPCHK(h, hipGetLastError());
      h->t2_ready = true;
    }
    f.tc = ThreshConsts{(const double*)h->T2.p, (const double*)h->thresh.p, (const double*)h->pmax.p, (const int*)h->need.p,
                        need_tag};
    f.fl = FloorLazy{(unsigned*)h->alim.p, nb, h->err_dev + 1, h->epoch};
  }
  *out = f;
  return SG_OK;
}

// One-pass gate (all four geometries): decide + smooth + apply in one kernel, tiles exchange their bits.  onepass_run owns the
// launch protocol -- floor test, tiles, exchange buffer, tickets, epochs, the REDO launch of a lazy call -- and the two
// geometries' stages (stage_onepass_reg, stage_onepass) supply what is particular to them.
//
// What onepass_run has worked out when it hands the arguments to the geometry's `first` hook:
struct OnePassCall {
  FloorSetup fs;      // fs.lazy: the floor test runs in the first launch and a REDO launch follows
  int64_t n_tiles;    // tiles per unit (the exchange buffer holds two halo tiles more)
  unsigned total;     // units * (n_tiles + 2): the workgroups, and the tickets, of a launch with one tile per workgroup
  unsigned grid;      // workgroups of the first launch (the hook may change it) ...
  unsigned tickets;   // ... and the tickets it draws from the running counter
};
// ARGS: the kernel's argument struct (fast::OnePassArgs / fast::OnePassRegArgs) with the geometry's tables filled in.
// first(P, C) completes it before the first launch (compare constants, what only that kernel has) and returns SG_OK or an
// error; launch(P, redo, grid) enqueues the kernel.  nb: bounds of the in-kernel floor test (floor_setup).
// fix(P, plan, lose): the geometry's one-launch floor fix-up (n_fft = 1024: k_floor_fix), or nullptr -- the register geometries'
// REDO bodies take their own argument struct and keep the two launches.
template <typename ARGS, typename FIRST, typename LAUNCH, typename FIX>
static int onepass_run(sg_handle* h, const View& v, const View& vx, const Geom& g, int64_t ub, const OutMap& om, hipStream_t st,
                       const OnePassGeom& S, int nb, ARGS P, FIRST first, LAUNCH launch, FIX fix, Decided* dec) {
  int rc;
  OnePassCall C;
  if ((rc = floor_setup(h, g, ub, nb, st, &C.fs))) return rc;
  const bool lazy = C.fs.lazy;
  ++(lazy ? h->n_floor_lazy : h->n_floor_apriori);
  if (!lazy && (rc = stage_prep_floor(h, v, g, ub, &C.fs.tc, st, &vx, h->err_dev + 1, h->epoch))) return rc;
  const HopRange hr = hop_range(om, g, S.hop);
  P.A.om = om;
  P.A.normalize = 1;
  P.A.h_begin = hr.h_begin;
  P.A.h_end = hr.h_end;
  const int64_t n_tiles = S.tiles(hr.count()), ntt = n_tiles + 2;
  // granule buffers are zero when (re)allocated and the epoch only grows: a fresh granule never carries it
  if ((rc = ensure_zeroed(h, h->xbits, (size_t)ub * ntt * S.tile_words * 8, st))) return rc;
  P.xbits = (unsigned long long*)h->xbits.p;
  P.ticket = (unsigned*)h->xticket.p;
  P.ticket_base = h->ticket_base;
  P.epoch = h->epoch;
  P.err = h->err_dev;
  P.nf = h->p.n_grad_freq; P.nt = h->p.n_grad_time;
  P.prop = (float)h->p.prop_decrease;
  {
    // the part of a unit's window outside its tiles' spans, dealt evenly to the unit's tiles ("floor test" in the kernels)
    const int64_t SPAN = (int64_t)(S.NF - 1 + 4) * S.hop;
    const int64_t sp0 = (hr.h_begin - 3 - S.NH) * S.hop - g.padL, sp1 = (hr.h_begin - 3 + n_tiles * S.NH) * S.hop - g.padL + SPAN;
    const int64_t inside = std::max<int64_t>(0, std::min<int64_t>(v.Lp, sp1) - std::max<int64_t>(0, sp0));
    const int64_t q = (v.Lp - inside + ntt - 1) / ntt;
    if (q > 0x7fffffff) FAIL(h, SG_E_UNSUPPORTED, "one-pass gate: window of %lld samples", (long long)v.Lp);
    P.scan_q = (int)q;
  }
  C.n_tiles = n_tiles;
  C.total = C.grid = C.tickets = (unsigned)(ub * ntt);
  if ((rc = first(P, C))) return rc;
  h->ticket_base += C.tickets;
  {
    ProfScope ps(h, SG_STAGE_ONEPASS, st);
    HIPCHK(h, launch(P, false, dim3(C.grid)));
  }
  h->floor_route = 0;
  if (lazy) {
    // the units whose floor test fired: float64 band maxima, then the gate again with them.  Every launch here returns at
    // once when no unit reported (the common case)
    ProfScope ps(h, SG_STAGE_STFT_MAX, st);
    fast::FloorFixPlan fp{};
    if constexpr (!std::is_same<FIX, std::nullptr_t>::value) {
      if (!h->floor_two && !h->mr_ok) fp = fast::floor_fix_plan(ub, g.T, C.total);
    }
    if (!fp.ok) {
      HIPCHK(h, launch_bits_any<0>(h, vx, g, ub, C.fs.tc, (unsigned long long*)h->pmax.p, (unsigned long long*)h->bits.p,
                                   (g.F + 63) / 64, st));
    } else if ((rc = ensure_zeroed(h, h->farrive, (size_t)ub * 8, st))) {
      return rc;
    }
    if ((rc = handoff_next_epoch(h, st))) return rc;
    P.epoch = h->epoch;
    P.ticket = (unsigned*)h->xticket.p + 8;   // its own counter (zeroed by the first launch's ticket-0 workgroup): it takes tickets only if a unit reported
    P.ticket_base = 0;
    if constexpr (!std::is_same<FIX, std::nullptr_t>::value) {
      // (SG_OPT_INJECT_HANDOFF_FAULT bits 3..4 lose every poll of the one-pass gate, bit 6 the wait for the maxima alone)
      if (fp.ok) HIPCHK(h, fix(P, fp, (h->lose_now & (3u | 8u)) != 0u));
    }
    if (!fp.ok) HIPCHK(h, launch(P, true, dim3(C.total)));
    h->floor_route = fp.ok ? SG_FLOOR_ONE_LAUNCH : SG_FLOOR_TWO_LAUNCH;
  }
  dec->tiles = TileLayout{S.NF, S.NH, S.tile_words, S.xw, (int)ntt, hr.h_begin - 3};
  dec->db = std::max<int64_t>(0, hr.h_begin - 3 - S.NH);
  dec->de = std::min<int64_t>(g.T, hr.h_begin - 3 + (int64_t)S.NH * (n_tiles + 1) + (S.NF - S.NH));
  return SG_OK;
}

// (round 6) one-pass gate of a register geometry (seam: abutting tiles + k_ola_seam, the default; SG_OPT_FORCE_NOSEAM keeps
// overlapping tiles where the geometry has them)
static int stage_onepass_reg(sg_handle* h, const RegGeom* r, const View& v, const View& vx, const Geom& g, int64_t ub,
                             const OutMap& om, bool seam, hipStream_t st, Decided* dec) {
  fast::OnePassRegArgs P{};
  P.A = reg_args(h, r, v, g);
  P.A.inv_ktot = (float)(1.0 / (double)h->ktot);
  P.tab = (const unsigned long long*)h->regtab.p;
  int rc;
  if (seam && (rc = reg_seam_tiles(h, r, hop_range(om, g, r->hop).count(), ub, &P.A))) return rc;
  const OnePassGeom& S = seam ? r->op_seam : r->op;
  auto first = [&](fast::OnePassRegArgs& Q, const OnePassCall& C) -> int {
    Q.A.tc = C.fs.tc;
    Q.A.fl = C.fs.fl;
    Q.n_tiles = (int)C.n_tiles;
    return SG_OK;
  };
  fast::RegArgs last{};
  auto launch = [&](fast::OnePassRegArgs& Q, bool redo, dim3 grid) {
    const bool lose = !redo && (h->lose_now & 3u);   // test hook: every poll of the first launch gives up at once (the timeout path itself)
    Q.poll_epoch = lose ? ~Q.epoch : Q.epoch;
    Q.spin_max = lose ? 0 : fast::OP_SPIN_MAX;
    last = Q.A;
    return launch_lds(r->gate[redo], grid, dim3(256), S.lds, st, Q);
  };
  if ((rc = onepass_run(h, v, vx, g, ub, om, st, S, (g.FS + 63) / 64, P, first, launch, nullptr, dec))) return rc;
  note_smooth(h, SG_SMOOTH_ONEPASS_REG, 1, S.NF);
  if (!seam) return SG_OK;
  if (r->abut && P.A.n_tiles < 2) return SG_OK;   // (2048 books no seam stage for a single tile)
  ProfScope ps(h, SG_STAGE_APPLY_FAST, st);   // (after the second launch, if any: a redone unit rewrote its partials)
  return launch_seam(h, r, last, ub, st);
}

static int stage_mag(sg_handle* h, const View& v, const Geom& g, int64_t ub, hipStream_t st, double iir_b = 0.0,
                     double* sub = nullptr /* register geometries: recurrence partials per magnitude tile (16 / 32 / 64 / 8 frames) */) {
  float* mag = (float*)h->P.p;
  if (const RegGeom* r = reg_geom(h)) return stage_mag_reg(h, r, v, g, ub, mag, st, iir_b, sub);
  if (h->fast_ok && !h->force_nofast) {
    ProfScope ps(h, SG_STAGE_STFT_MAG, st);
    constexpr int WAVES = 4;
    fast::MagArgs M;
    M.view = v; M.g = g;
    M.win = (const float*)h->wa32.p;
    M.tw512 = (const fast::cf*)h->tw512.p;
    M.tw1024 = (const fast::cf*)h->tw32.p;
    M.mag = mag;
    M.iir_b = iir_b; M.sub = sub;
    size_t lds = (size_t)(fast::FN + WAVES * fast::WAVE_CX_H) * sizeof(fast::cf) + 1024 * sizeof(float);
    auto kern = fast::k_mag_fast<WAVES>;
    dim3 grid((unsigned)((g.T + 4 * WAVES - 1) / (4 * WAVES)), (unsigned)ub);
    HIPCHK(h, launch_lds(kern, grid, dim3(WAVES * 64), lds, st, M));
  } else {
    ProfScope ps(h, SG_STAGE_STFT_MAG, st);
    HIPCHK(h, stft_any<float>(h, v, g, ub, nullptr, mag, nullptr, 1.0, st));
  }
  return SG_OK;
}

// Variant-S non-stationary mask in two passes over |X| (nonstat.hpp): partials -> chain -> IIR + sigmoid (+ smoothing).
// (route.hpp: NsMask::SMOOTHED -- k_iir_mask also smooths, the mask in one kernel; NsMask::CHAIN -- other smoothing widths
// take k_iir_mask<0> for the raw sigmoid field and the general smoothing kernels after it.)

// smooth: IIR + sigmoid + smoothing + prop_decrease -> M;  !smooth: the raw sigmoid field -> raw (smoothing follows),
// or, without a smoothing filter, p * sigmoid + (1 - p) -> M
// pp: c^len and 1 - c^(2 len) of the chain's pieces, worked out in the call's first batch and kept for the others
struct PiecePows {
  int plen = 0;
  int64_t np = 0;
  double o[4];
};
static int stage_nonstat_mask2(sg_handle* h, const View& v, const Geom& g, int64_t ub, bool smooth, hipStream_t st, PiecePows* pp) {
  // register geometries: the magnitude kernel also leaves the recurrence partials of its tiles -- 16 frames at n_fft = 1024,
  // (round 6) 32 / 64 / 8 at 512 / 256 / 2048 -- no second pass over |X| (k_iir_part); PER pieces per 64-frame tile of the chain
  const RegGeom* r = reg_geom(h);
  const int plen = r ? r->frames : 16, per = NS_TT / plen;
  const int64_t nsub = (g.T + plen - 1) / plen;
  const bool sub_ok = r ? !h->force_split && ub <= 65535 &&
                              nsp_ok((g.T + NS_TT - 1) / NS_TT, per)   // (the serial chain kernels know 16-frame pieces only)
                        : h->fast_ok && !h->force_nofast;
  int rc;
  if (sub_ok && (rc = ensure(h, h->nss, (size_t)ub * nsub * 2 * g.FS * sizeof(double)))) return rc;
  rc = stage_mag(h, v, g, ub, st, h->p.iir_b, sub_ok ? (double*)h->nss.p : nullptr);
  if (rc) return rc;
  const float* mag = (const float*)h->P.p;
  const int nf = smooth ? h->p.n_grad_freq : 0, nt = smooth ? h->p.n_grad_time : 0;
  NsTiling tl{g.T, nt};
  const int64_t nk = tl.n_tiles();
  const size_t bytes = (size_t)ub * nk * 2 * g.FS * sizeof(double);
  if ((rc = ensure(h, h->nsp, bytes))) return rc;
  if ((rc = ensure(h, h->nsc, bytes))) return rc;
  {
    ProfScope ps(h, SG_STAGE_IIR_CHAIN, st);
    // (round 5) k_iir_chain_par: the chain in 16 runs per band, straight from the 16-frame sub-tile partials where
    // k_mag_fast left them (no k_iir_comb); SG_OPT_FORCE_SPLIT keeps the serial kernels (A/B)
    const bool par = !h->force_split && ub <= 65535;
    const dim3 pgrid((unsigned)((g.F + 63) / 64), (unsigned)ub);
    // c^len and 1 - c^(2 len) of a full piece and of the unit's last one (uniform: computed here, not per thread)
    auto piece_pows = [&](int plen, int64_t np, double* o) {
      if (pp->plen != plen || pp->np != np) {
        const double c = 1.0 - h->p.iir_b, len_last = (double)(g.T - (np - 1) * plen);
        pp->o[0] = std::pow(c, (double)plen); pp->o[1] = 1.0 - std::pow(c, 2.0 * plen);
        pp->o[2] = std::pow(c, len_last); pp->o[3] = 1.0 - std::pow(c, 2.0 * len_last);
        pp->plen = plen; pp->np = np;
      }
      std::copy(pp->o, pp->o + 4, o);
    };
    double pw[4];
    if (sub_ok && par && nsp_ok(nk, per)) {
      piece_pows(plen, nsub, pw);
      auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, pgrid, dim3(64 * NSP_WAVES), 0, st, mag, (const double*)h->nss.p, g, tl, h->p.iir_b,
                           (double*)h->nsc.p, (int)nsub, pw[0], pw[1], pw[2], pw[3]);
      };
      if (per == 4) go(k_iir_chain_par<4>);
      else if (per == 2) go(k_iir_chain_par<2>);
      else if (per == 1) go(k_iir_chain_par<1>);
      else go(k_iir_chain_par<8>);
      HIPCHK(h, hipGetLastError());
    } else {
      if (sub_ok)
        hipLaunchKernelGGL(k_iir_comb, dim3((unsigned)((nk * g.FS + 255) / 256), (unsigned)ub), dim3(256), 0, st,
                           (const double*)h->nss.p, g, tl, h->p.iir_b, (double*)h->nsp.p, (int)nsub);
      else
        hipLaunchKernelGGL(k_iir_part, dim3((unsigned)((nk * (g.FS / 4) + 255) / 256), (unsigned)ub), dim3(256), 0,
                           st, mag, g, tl, h->p.iir_b, (double*)h->nsp.p);
      HIPCHK(h, hipGetLastError());
      // (tile partials: n_fft = 256 / 512 / 2048 -- 162 / 81 / 21 tiles per unit -- measured 12 / 6 / 1.4 % of the call)
      if (par && nk >= 8 && nsp_ok(nk, 1)) {
        piece_pows(NS_TT, nk, pw);
        hipLaunchKernelGGL(k_iir_chain_par<1>, pgrid, dim3(64 * NSP_WAVES), 0, st, mag, (const double*)h->nsp.p, g, tl,
                           h->p.iir_b, (double*)h->nsc.p, (int)nk, pw[0], pw[1], pw[2], pw[3]);
      } else {
        hipLaunchKernelGGL((k_iir_chain<float, false>), dim3((unsigned)((ub * g.FS + 63) / 64)), dim3(64), 0, st, mag,
                           (const double*)h->nsp.p, g, tl, h->p.iir_b, (double*)h->nsc.p, ub);
      }
      HIPCHK(h, hipGetLastError());
    }
  }
  {
    ProfScope ps(h, SG_STAGE_IIR_MASK, st);
    const int BW = 64 - 2 * nf;
    const unsigned gx = (unsigned)(((g.F + BW - 1) / BW + 3) / 4);
    const bool to_raw = !smooth && h->p.smooth_mask;
    for (int64_t k0 = 0; k0 < nk; k0 += 65535) {   // grid.y <= 65535 tiles per launch (a 6-hour window has more)
      tl.k0 = k0;
      HIPCHK(h, launch_iir_mask(nt, dim3(gx, (unsigned)std::min<int64_t>(65535, nk - k0), (unsigned)ub), st, mag,
                                (const double*)h->nsc.p, g, tl, h->p.iir_b, h->p.nonstat_thresh, h->p.nonstat_slope, nf,
                                to_raw ? 1.0f : (float)h->p.prop_decrease, to_raw ? (float*)h->raw.p : (float*)h->M.p));
    }
    note_smooth(h, smooth ? SG_SMOOTH_IIR_MASK : SG_SMOOTH_OFF, 4, smooth ? NS_TT : 0);   // (k_iir_mask<0>: the general smoothing follows, if any)
  }
  return SG_OK;
}

// Variant-T non-stationary mask in one kernel (nonstat.hpp: k_box_mask): the default moving-mean length and the
// smoothing widths k_iir_mask also covers; other settings keep k_boxcar_sigmoid + the general smoothing kernels
// (route.hpp: NsMask::BOX).

static int stage_box_mask(sg_handle* h, const View& v, const Geom& g, int64_t ub, hipStream_t st) {
  int rc = stage_mag(h, v, g, ub, st);
  if (rc) return rc;
  ProfScope ps(h, SG_STAGE_NONSTAT_MASK, st);
  const int nf = h->p.smooth_mask ? h->p.n_grad_freq : 0, nt = h->p.smooth_mask ? h->p.n_grad_time : 0;
  const int BW = 64 - 2 * nf;
  const unsigned gx = (unsigned)(((g.F + BW - 1) / BW + 3) / 4);
  const unsigned nk = (unsigned)((g.T + NS_TT - 1) / NS_TT);
  for (int64_t k0 = 0; k0 < (int64_t)nk; k0 += 65535)   // grid.y <= 65535 tiles per launch
    HIPCHK(h, launch_box_mask(nt, h->p.n_movemean, dim3(gx, (unsigned)std::min<int64_t>(65535, (int64_t)nk - k0), (unsigned)ub), st,
                              (const float*)h->P.p, g, h->p.nonstat_thresh, h->p.nonstat_slope, nf, (float)h->p.prop_decrease,
                              (float*)h->M.p, k0));
  note_smooth(h, SG_SMOOTH_BOX_MASK, 4, NS_TT);
  return SG_OK;
}

static int stage_nonstat_raw(sg_handle* h, const View& v, const Geom& g, int64_t ub, hipStream_t st) {
  int rc0 = stage_mag(h, v, g, ub, st);
  if (rc0) return rc0;
  float* mag = (float*)h->P.p;
  ProfScope ps(h, SG_STAGE_NONSTAT_MASK, st);
  dim3 grid((g.F + 63) / 64, (unsigned)ub);
  if (h->p.variant == SG_VARIANT_S) {
    // |Z| scale (1/sum_w) cancels in (A-S)/S: work on the unscaled magnitude.
    if (g.T >= 4 * IIR_NSEG)
      hipLaunchKernelGGL(k_iir_sigmoid_seg, grid, dim3(64 * IIR_NSEG), 0, st, (const float*)mag, g, h->p.iir_b,
                         h->p.nonstat_thresh, h->p.nonstat_slope, (float*)h->raw.p);
    else
      hipLaunchKernelGGL(k_iir_sigmoid, grid, dim3(64), 0, st, (const float*)mag, g, h->p.iir_b,
                         h->p.nonstat_thresh, h->p.nonstat_slope, (float*)h->raw.p);
  } else {
    dim3 bgrid((unsigned)((g.F + 63) / 64), (unsigned)((g.T + 4 * BOX_TSEG - 1) / (4 * BOX_TSEG)), (unsigned)ub);
    hipLaunchKernelGGL(k_boxcar_sigmoid, bgrid, dim3(256), 0, st, (const float*)mag, g, h->p.n_movemean,
                       h->p.nonstat_thresh, h->p.nonstat_slope, (float*)h->raw.p);
  }
  HIPCHK(h, hipGetLastError());
  return SG_OK;
}

// M_out: where the mask goes (nullptr: the workspace field h->M)
static int stage_smooth(sg_handle* h, const Geom& g, int64_t ub, hipStream_t st, float* M_out = nullptr) {
  float* const Mdst = M_out ? M_out : (float*)h->M.p;
  ProfScope ps(h, SG_STAGE_SMOOTH, st);
  int64_t cells = ub * g.T * g.FS;
  float p = (float)h->p.prop_decrease;
  if (!h->p.smooth_mask) {
    hipLaunchKernelGGL(k_prop_only, dim3(grid_1d(cells, 256)), dim3(256), 0, st, (const float*)h->raw.p, g, p,
                       Mdst, ub);
    HIPCHK(h, hipGetLastError());
    note_smooth(h, SG_SMOOTH_OFF, 4, 0);
    return SG_OK;
  }
  // prop_decrease is applied before smoothing by stationary.py:108-114 and torchgate.py:241-249,
  // after smoothing by nonstationary.py:78-84.
  const int prop_before0 = (h->p.variant == SG_VARIANT_T || h->p.stationary) ? 1 : 0;
  {
    const int nf = h->p.n_grad_freq, nt = h->p.n_grad_time;
    const int rows = SMF_TT + 2 * nt, cols = SMF_FB + 2 * nf;
    // +3: the sliding windows read up to 3 entries past the last tap
    size_t lds = ((size_t)(rows + 3) * (cols | 1) + (size_t)(rows + 3) * (SMF_FB + 1) + 8 + 64 + SMF_KT + SMF_FB + SMF_TT) * sizeof(float);
    // (time half-widths up to 94: short frames have long smoothing windows in frames -- n_fft = 256 at 48 kHz: nt = 37 --
    // and used to fall through to the two direct global-memory convolutions below: 0.73 ms of a 1.09 ms call)
    if (lds <= 150 * 1024 && ub <= 65535 && nf <= 30 && 2 * nt + 4 <= SMF_KT && SMF_FB + 2 * nf <= 192) {
      auto kern = k_smooth_tiled;
      dim3 grid((g.F + SMF_FB - 1) / SMF_FB, (unsigned)((g.T + SMF_TT - 1) / SMF_TT), (unsigned)ub);
      HIPCHK(h, launch_lds_if(lds > 65536, kern, grid, dim3(256), lds, st, (const float*)h->raw.p, g, (const float*)h->kf.p, nf,
                              (const float*)h->kt.p, nt, p, prop_before0, Mdst));
      note_smooth(h, SG_SMOOTH_TILED, 4, SMF_TT);
      return SG_OK;
    }
  }
  float* tmp = (float*)h->seg.p;  // seg is not live yet
  hipLaunchKernelGGL(k_smooth_f, dim3(grid_1d(cells, 256)), dim3(256), 0, st, (const float*)h->raw.p, g,
                     (const float*)h->kf.p, h->p.n_grad_freq, tmp, ub);
  HIPCHK(h, hipGetLastError());
  // prop_decrease is applied before smoothing by stationary.py:108-114 and torchgate.py:241-249,
  // after smoothing by nonstationary.py:78-84.
  int prop_before = (h->p.variant == SG_VARIANT_T || h->p.stationary) ? 1 : 0;
  hipLaunchKernelGGL(k_smooth_t, dim3(grid_1d(cells, 256)), dim3(256), 0, st, (const float*)tmp, g,
                     (const float*)h->kt.p, h->p.n_grad_time, (const float*)h->kf.p, h->p.n_grad_freq, p,
                     prop_before, Mdst, ub);
  HIPCHK(h, hipGetLastError());
  note_smooth(h, SG_SMOOTH_SEPARATE, 4, 0);
  return SG_OK;
}

static int stage_apply_ola(sg_handle* h, const View& v, const Geom& g, int64_t ub, const float* M,
                           const OutMap& om, int normalize, hipStream_t st, const unsigned short* K16 = nullptr,
                           float kscale = 0.f) {
  {
    ProfScope ps(h, SG_STAGE_APPLY_ISTFT, st);
    HIPCHK(h, apply_any(h, v, g, ub, M, (float*)h->seg.p, st, K16, kscale));
  }
  int64_t np = om.p1 - om.p0;
  if (np > 0) {
    ProfScope ps(h, SG_STAGE_OLA, st);
    dim3 grid((unsigned)((np + 255) / 256), (unsigned)ub);
    hipLaunchKernelGGL(k_ola, grid, dim3(256), 0, st, v, g, om, (const float*)h->seg.p, (const float*)h->wsq32.p,
                       normalize);
    HIPCHK(h, hipGetLastError());
  }
  return SG_OK;
}

// bits -> K (uint16 weight sums), natural or lane order
static int stage_smooth_bits(sg_handle* h, const Geom& g, int64_t ub, bool fast, int64_t tb, int64_t te,
                             hipStream_t st) {
  const int wpr = (g.F + 63) / 64;
  ProfScope ps(h, SG_STAGE_SMOOTH, st);
  const int nf = h->p.n_grad_freq, nt = h->p.n_grad_time;
  int64_t cells = ub * g.T * g.FS;
  if (h->p.smooth_mask && nf <= 30) {
    const int tt = h->sm2_tt;
    const int rows = tt + 2 * nt;
    const bool small = (nf + 1) * (nf + 1) <= 255;
    const unsigned long long* ftab = (small && h->ftab.p) ? (const unsigned long long*)h->ftab.p : nullptr;
    size_t lds = smooth2_cf_bytes(rows + 2, g.F, small ? 1 : 2) + (size_t)rows * (wpr + 2) * 8 + (ftab ? 8192 : 0);
    dim3 grid((unsigned)((te - tb + tt - 1) / tt), (unsigned)ub);
    // (cell: uint8_t weight sums while (nf + 1)^2 fits a byte, else uint16_t; ftab is null then)
    auto go = [&](auto cell) {
      return launch_lds_if(lds > 65536, k_smooth_bits2<decltype(cell)>, grid, dim3(SM2_THREADS), lds, st,
                           (const unsigned long long*)h->bits.p, g, wpr, nf, nt, (unsigned short*)h->K16.p, fast ? 1 : 0, tb, te, ftab, tt);
    };
    HIPCHK(h, small ? go(uint8_t{}) : go(uint16_t{}));
    note_smooth(h, SG_SMOOTH_BITS2, small ? 1 : 2, tt);
  } else if (h->p.smooth_mask) {
    const int rows = SM_TT + 2 * nt;
    const bool small = (nf + 1) * (nf + 1) <= 255;
    size_t lds = smooth_cf_bytes(rows, g.F, small ? 1 : 2) + (size_t)rows * wpr * 8;
    dim3 grid((unsigned)((g.T + SM_TT - 1) / SM_TT), (unsigned)ub);
    auto go = [&](auto cell) {
      return launch_lds_if(lds > 65536, k_smooth_bits<decltype(cell)>, grid, dim3(256), lds, st,
                           (const unsigned long long*)h->bits.p, g, wpr, nf, nt, (unsigned short*)h->K16.p, fast ? 1 : 0);
    };
    HIPCHK(h, small ? go(uint8_t{}) : go(uint16_t{}));
    note_smooth(h, SG_SMOOTH_BITS, small ? 1 : 2, SM_TT);
  } else {
    hipLaunchKernelGGL(k_bits_to_k16, dim3(grid_1d(cells, 256)), dim3(256), 0, st,
                       (const unsigned long long*)h->bits.p, g, wpr, (unsigned short*)h->K16.p, ub, fast ? 1 : 0);
    HIPCHK(h, hipGetLastError());
    note_smooth(h, SG_SMOOTH_OFF, 2, 0);
  }
  return SG_OK;
}

// Compare constants + per-unit floor flags + (rare) float64 floor pre-pass: what every decision kernel of
// the fused stationary path needs before it can run.
static int stage_prep_floor(sg_handle* h, const View& v, const Geom& g, int64_t ub, ThreshConsts* tc_out,
                            hipStream_t st, const View* v_exact = nullptr, unsigned* live_host = nullptr,
                            unsigned stamp = 0) {
  const int wpr = (g.F + 63) / 64;
  int rc;
  if ((rc = ensure(h, h->bits, (size_t)ub * g.T * wpr * 8))) return rc;
  // umax is kept clean by its consumer (k_prep_thresh zeroes what it read); pmax rows are zeroed by
  // k_prep_thresh for exactly the units whose floor can be live (the only rows anybody reads): no memset
  // launches on the critical path
  if ((rc = ensure_zeroed(h, h->umax, (size_t)ub * 4, st))) return rc;
  if ((rc = ensure_zeroed(h, h->need, (size_t)ub * 4, st))) return rc;
  if ((rc = ensure(h, h->T2, (size_t)g.FS * 8))) return rc;
  {
    ProfScope ps(h, SG_STAGE_PREP, st);
    hipLaunchKernelGGL(k_unit_absmax, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(64, 2048 / ub)), (unsigned)ub),
                       dim3(256), 0, st, v, ub, (unsigned*)h->umax.p);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_prep_thresh, dim3((unsigned)((ub + 255) / 256)), dim3(256), 0, st,
                       (const double*)h->thresh.p, g.F, h->mag_scale, h->sum_abs_w, h->p.top_db,
                       (unsigned*)h->umax.p, ub, (double*)h->T2.p, (int*)h->need.p, (double*)h->pmax.p, g.FS, live_host,
                       stamp);
    HIPCHK(h, hipGetLastError());
  }
  ThreshConsts tc{(const double*)h->T2.p, (const double*)h->thresh.p, (const double*)h->pmax.p,
                  (const int*)h->need.p};
  {
    ProfScope ps(h, SG_STAGE_STFT_MAX, st);
    // (float64 transform of the ORIGINAL samples when `v` is a float32 copy)
    HIPCHK(h, launch_bits_any<0>(h, v_exact ? *v_exact : v, g, ub, tc,
                             (unsigned long long*)h->pmax.p, (unsigned long long*)h->bits.p, wpr, st));
  }
  *tc_out = tc;
  return SG_OK;
}

// Fused stationary mask (variant S): STFT(f64) -> bits -> integer smoothing -> K16 -> float mask.
// pl.decide names the decision kernel; K in the fused apply kernel's lane order unless pl.pipe is the general FUSED one.
static int stage_fused_mask(sg_handle* h, const route::SPlan& pl, const View& v, const Geom& g, int64_t ub, int64_t tb,
                            int64_t te, hipStream_t st, Decided* dec) {
  using route::Decide;
  const bool fast = pl.pipe != route::Pipe::FUSED;
  // [tb, te): frames whose smoothed mask is needed; decisions are needed nt frames further out
  const int64_t nt_halo = h->p.smooth_mask ? h->p.n_grad_time : 0;
  const int64_t db = std::max<int64_t>(0, tb - nt_halo), de = std::min<int64_t>(g.T, te + nt_halo);
  dec->db = db; dec->de = de;   // (reported where k_decide_fast decides: every other kernel decides all frames)
  const int wpr = (g.F + 63) / 64;
  int rc;
  if ((rc = ensure(h, h->K16, (size_t)ub * g.T * g.FS * 2))) return rc;
  // (round 6) The register-transform decision kernels of n_fft = 512 / 256 / 2048 stage every sample of a unit's window: they
  // run the floor test themselves (thresh.hpp: FloorLazy -- the one-pass gate's protocol) instead of k_unit_absmax +
  // k_prep_thresh reading the recording once more before the gate.  Same prediction as the one-pass gates (floor_setup);
  // both end in exact band maxima.
  const RegGeom* r = pl.decide == Decide::REG ? h->reg : nullptr;
  FloorSetup fs;
  if (r && h->floor_test != 1 && (rc = floor_setup(h, g, ub, (g.FS + 63) / 64, st, &fs))) return rc;
  const bool lazy = fs.lazy;
  const ThreshConsts& tc = fs.tc;
  if (r) ++(lazy ? h->n_floor_lazy : h->n_floor_apriori);
  if (!lazy && (rc = stage_prep_floor(h, v, g, ub, &fs.tc, st, nullptr, r && h->err_dev ? h->err_dev + 1 : nullptr, h->epoch)))
    return rc;
  if (pl.decide == Decide::FAST) {
    ProfScope ps(h, SG_STAGE_DECIDE_FAST, st);
    constexpr int WAVES = 4;
    fast::DecideArgs D;
    D.view = v; D.g = g;
    D.win = (const float*)h->wa32.p;
    D.win64 = (const double*)h->wfull64.p;
    D.tw512 = (const fast::cf*)h->tw512.p;
    D.tw1024 = (const fast::cf*)h->tw32.p;
    D.tw64 = (const cx<double>*)h->tw64.p;
    D.tc = tc;
    D.mag_scale = h->mag_scale; D.top_db = h->p.top_db;
    D.bits = (unsigned long long*)h->bits.p;
    D.wpr = wpr;
    D.t_begin = db; D.t_end = de;
    D.quads_per_wave = 1;
    const int64_t quads = (D.t_end - D.t_begin + 3) / 4;
    const int64_t per_block = (int64_t)WAVES * D.quads_per_wave;
    size_t lds = (size_t)(fast::FN + WAVES * fast::WAVE_CX_H) * sizeof(fast::cf) + (T2_FLOATS + 1024) * sizeof(float);
    auto kern = fast::k_decide_fast<WAVES>;
    dim3 grid((unsigned)((quads + per_block - 1) / per_block), (unsigned)ub);
    HIPCHK(h, launch_lds(kern, grid, dim3(WAVES * 64), lds, st, D));
  } else if (r) {
    if ((rc = stage_decide_reg(h, r, v, g, ub, tc, (unsigned long long*)h->bits.p, st, fs.fl))) return rc;
  } else if (pl.decide == Decide::LDS) {
    // other power-of-two frame lengths: float32 LDS transform + exact refinement
    ProfScope ps(h, SG_STAGE_STFT_BITS, st);
    HIPCHK(h, launch_decide_lds(h, v, g, ub, tc, (unsigned long long*)h->bits.p, wpr, st));
  } else {
    ProfScope ps(h, SG_STAGE_STFT_BITS, st);
    HIPCHK(h, launch_bits_any<1>(h, v, g, ub, tc,
                             (unsigned long long*)h->pmax.p, (unsigned long long*)h->bits.p, wpr, st));
  }
  if (lazy) {
    // the units whose floor test fired: float64 band maxima, then their decisions again with them.  Both launches return at
    // once when no unit reported (the common case)
    {
      ProfScope ps(h, SG_STAGE_STFT_MAX, st);
      HIPCHK(h, launch_bits_any<0>(h, v, g, ub, tc, (unsigned long long*)h->pmax.p, (unsigned long long*)h->bits.p, wpr, st));
    }
    if ((rc = stage_decide_reg(h, r, v, g, ub, tc, (unsigned long long*)h->bits.p, st, fs.fl, true))) return rc;
  }
  { int rc2 = stage_smooth_bits(h, g, ub, fast, tb, te, st); if (rc2) return rc2; }
  const int nf = h->p.n_grad_freq, nt = h->p.n_grad_time;
  int64_t cells = ub * g.T * g.FS;
  // The fused apply kernel reads K directly; so do k_apply_fast512 / 256 / 2048<K> and (round 5) k_apply_istft (power-of-two
  // frames on the LDS transform): the float mask field is only written when somebody asks for it (sg_debug_fetch field 1
  // expands the K counts of the last batch then)
  if (!pl.k16_to_mask) return SG_OK;
  hipLaunchKernelGGL(k_k16_to_mask, dim3(grid_1d(cells / 8, 256)), dim3(256), 0, st, (const unsigned short*)h->K16.p,
                     g, nf, nt, 1.0f / (float)h->ktot, (float)h->p.prop_decrease, 1, h->p.smooth_mask ? 1 : 0,
                     (float*)h->M.p, ub);
  HIPCHK(h, hipGetLastError());
  return SG_OK;
}

// Fused apply (default geometry): FFT -> mask(K) -> IFFT -> overlap-add -> output, one kernel.
static int stage_apply_fast(sg_handle* h, const View& v, const Geom& g, int64_t ub, const OutMap& om,
                            const float* mask_f /* nullptr: uint16 counts in h->K16 */, int normalize,
                            hipStream_t st) {
  ProfScope ps(h, SG_STAGE_APPLY_FAST, st);
  constexpr int WAVES = SG_APPLY_WAVES;
  fast::ApplyArgs A;
  A.view = v; A.g = g; A.om = om;
  A.K = (const unsigned short*)h->K16.p;
  A.Mf = mask_f;
  A.normalize = normalize;
  A.win = (const float*)h->wa32.p;
  A.wsq = (const float*)h->wsq32.p;
  A.invn = (const float*)h->invn.p;
  A.tw512 = (const fast::cf*)h->tw512.p;
  A.tw1024 = (const fast::cf*)h->tw32.p;
  A.kscale = mask_f ? (float)(1.0 / 512.0) : (float)(1.0 / ((double)h->ktot * 512.0));
  const HopRange hr = hop_range(om, g, 256);
  A.h_begin = hr.h_begin;
  A.h_end = hr.h_end;
  const int64_t nh = hr.count();
  if (nh <= 0) return SG_OK;
  constexpr int NF = 4 * WAVES, NH = NF - 3;
  size_t lds = (size_t)(fast::FN + WAVES * fast::WAVE_CX) * sizeof(fast::cf);
  // seam mode: abutting tiles + k_ola_seam for the straddling hops (3/16 fewer transforms)
  const int64_t tiles_seam = abutting_tiles(nh, NF);
  const bool seam = !h->force_noseam && tiles_seam >= 2;
  const bool lean = !h->force_nolean;
  // lean kernel: the straddling hops are handed from tile to tile inside the launch; else partial sums + k_ola_seam
  const bool inkernel = seam && lean;
  A.part = nullptr;
  A.part2 = nullptr;
  A.epoch = 0;
  A.err = nullptr;
  A.n_tiles = 0;
  A.ticket = nullptr;
  if (inkernel) {
    int rc = ensure_zeroed(h, h->xpart, (size_t)ub * tiles_seam * 3 * 256 * 8, st);
    if (rc) return rc;
    if ((rc = handoff_prepare(h, st))) return rc;
    A.part2 = (unsigned long long*)h->xpart.p;
    A.epoch = h->epoch;
    A.err = h->err_dev;
    A.n_tiles = (int)tiles_seam;
    // tile = ticket (fastpath.hpp: ApplyArgs::ticket): one self-resetting counter per unit
    if ((rc = ensure_zeroed(h, h->xtick2, (size_t)ub * 64, st))) return rc;
    A.ticket = (unsigned*)h->xtick2.p;
  } else if (seam) {
    int rc = ensure(h, h->seam, (size_t)ub * tiles_seam * 6 * 256 * sizeof(float));
    if (rc) return rc;
    A.part = (float*)h->seam.p;
    A.n_tiles = (int)tiles_seam;
  }
  dim3 grid((unsigned)(seam ? tiles_seam : (nh + NH - 1) / NH), (unsigned)ub);
  auto go = [&](void (*kern)(fast::ApplyArgs), size_t lds_bytes) { return launch_lds(kern, grid, dim3(WAVES * 64), lds_bytes, st, A); };
  const size_t lds_lean = (size_t)(fast::FN + WAVES * fast::WAVE_CX_H) * sizeof(fast::cf) + 1024 * sizeof(float) + 16;
  const bool lose = inkernel && (h->lose_now & 4u);   // test hook: the instantiation whose hand-off polls give up at once
  if (mask_f) {
    if (lose) HIPCHK(h, go(fast::k_apply_fast<WAVES, false, true, true>, lds_lean));
    else if (lean) HIPCHK(h, go(fast::k_apply_fast<WAVES, false, true>, lds_lean));
    else HIPCHK(h, go(fast::k_apply_fast<WAVES, false, false>, lds));
  } else {
    if (lose) HIPCHK(h, go(fast::k_apply_fast<WAVES, true, true, true>, lds_lean));
    else if (lean) HIPCHK(h, go(fast::k_apply_fast<WAVES, true, true>, lds_lean));
    else HIPCHK(h, go(fast::k_apply_fast<WAVES, true, false>, lds));
  }
  if (seam && !inkernel) {
    hipLaunchKernelGGL(fast::k_ola_seam<NF>, dim3((unsigned)(tiles_seam - 1), (unsigned)ub), dim3(256), 0, st, A);
    HIPCHK(h, hipGetLastError());
  }
  return SG_OK;
}

// The -DOP_TRACE=1 development build of the n_fft = 1024 one-pass gate (onepass.hpp; tools/trace_onepass.py, tools/ab_persist.py):
// one process-wide device buffer that stage_onepass attaches to the first launch's arguments; sg_debug_counter 8 reads it back
// (onepass_dev_counter_impl).
#if OP_TRACE
static unsigned* g_trace_dev = nullptr;   // the one-pass gate's phase trace of the last first launch: sg_debug_counter 8
static size_t g_trace_tiles = 0;
static int g_trace_ntt = 1;
static size_t g_trace_slots = 0;
// at exit: the average shader cycles per wave and phase of the last traced launch (tools/trace_onepass.py --table reads these lines)
static void op_trace_report() {
  std::vector<unsigned> hst(g_trace_slots * 16);
  if (hipMemcpy(hst.data(), g_trace_dev, hst.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
  double sum[14] = {0}, w = 0, mx = 0;
  double wsum[4][14] = {{0}}, ww[4] = {0};   // the same per wave index (slot = ticket * 4 + wave)
  for (size_t i = 0; i < g_trace_slots; ++i) {
    if (hst[i * 16 + 15] != 1u) continue;
    w += 1;
    ww[i & 3] += 1;
    double tot = 0;
    for (int k = 0; k < 14; ++k) { sum[k] += hst[i * 16 + k]; wsum[i & 3][k] += hst[i * 16 + k]; tot += hst[i * 16 + k]; }
    mx = std::max(mx, tot);
  }
  for (int wv = 0; wv < 4; ++wv) {
    fprintf(stderr, "[OP_TRACE] wave %d (%.0f completed):", wv, ww[wv]);
    for (int k = 0; k < 14; ++k) fprintf(stderr, " %d:%.0f", k, wsum[wv][k] / (ww[wv] > 0 ? ww[wv] : 1));
    fprintf(stderr, "\n");
  }
  fprintf(stderr, "[OP_TRACE] completed waves %.0f; average shader cycles per wave and phase:", w);
  double tot = 0;
  for (int k = 0; k < 14; ++k) { fprintf(stderr, " %d:%.0f", k, sum[k] / (w > 0 ? w : 1)); tot += sum[k] / (w > 0 ? w : 1); }
  fprintf(stderr, "  sum %.0f  longest wave %.0f\n", tot, mx);
}
// one device trace [workgroup][wave][16] of `tiles` tiles (`ntt` per unit), overwritten by every launch
static hipError_t op_trace_attach(sg::fast::OnePassArgs& P, size_t tiles, int ntt, hipStream_t st) {
  const size_t slots = tiles * 4;
  if (!g_trace_dev || g_trace_slots < slots) {
    hipError_t e = hipMalloc((void**)&g_trace_dev, slots * 64);   // (the smaller one stays allocated, as the trace of a launch that may still run)
    if (e != hipSuccess) return e;
    g_trace_slots = slots;
    static const int registered = atexit(op_trace_report);
    (void)registered;
  }
  P.trace = g_trace_dev;
  g_trace_tiles = tiles; g_trace_ntt = ntt;
  return hipMemsetAsync(g_trace_dev, 0, slots * 64, st);
}
#endif

// One-pass stationary gate (default geometry, onepass.hpp): forward transform once per frame; decide,
// publish the tile's bits, smooth in LDS, x mask, inverse transform, overlap-add -- one kernel (+ the
// seam kernel for the 3 hops that straddle two tiles).  (route.hpp: onepass_ok -- a shape that is not eligible runs the
// three-kernel path.)

static int stage_onepass(sg_handle* h, const View& v, const View& vx, const Geom& g, int64_t ub, const OutMap& om,
                         hipStream_t st, Decided* dec) {
  constexpr int WAVES = 4;
  const OnePassGeom& S = OP1024;
  fast::OnePassArgs P{};
  P.x_exact = vx.x; P.stride_exact = vx.stride; P.dtype_exact = vx.dtype;
  fast::ApplyArgs& A = P.A;   // (K / Mf, part / part2, epoch, err, ticket stay null: the one-pass kernel has its own hand-off arguments)
  A.view = v; A.g = g;
  A.win = (const float*)h->wa32.p;
  A.wsq = (const float*)h->wsq32.p;
  A.invn = (const float*)h->invn.p;
  A.tw512 = (const fast::cf*)h->tw512.p;
  A.tw1024 = (const fast::cf*)h->tw32.p;
  const bool prop = h->p.prop_decrease != 1.0;
  A.kscale = prop ? (float)(1.0 / 512.0) : (float)(1.0 / ((double)h->ktot * 512.0));
  P.tab = (const char*)h->optab.p;
  P.mag_scale = h->mag_scale; P.top_db = h->p.top_db;
  P.inv_ktot = 1.0f / (float)h->ktot;
  bool persist = false;
  auto first = [&](fast::OnePassArgs& Q, OnePassCall& C) -> int {
    int rc;
    if ((rc = ensure_zeroed(h, h->xpart, (size_t)ub * C.n_tiles * 3 * 256 * 8, st))) return rc;
    Q.part2 = (unsigned long long*)h->xpart.p;
    Q.A.n_tiles = (int)C.n_tiles;
    Q.tc = C.fs.tc;
    Q.alim = C.fs.lazy ? (unsigned*)h->alim.p : nullptr;
    Q.total_tiles = C.total;
    {
      // the launch plan (onepass_plan.hpp): quotients as multiply-highs, the interior units and the tile ranges in which
      // blk_vec and tile_fast hold for them, folded source and output addresses
      fast::OpPlanIn I{};
      const View& w = Q.A.view;
      const OutMap& m = Q.A.om;
      I.x = (uint64_t)(uintptr_t)w.x; I.out = (uint64_t)(uintptr_t)m.out;
      I.in_dtype = w.dtype; I.out_dtype = m.dtype; I.normalize = Q.A.normalize;
      I.stride = w.stride; I.lo = w.lo; I.hi = w.hi; I.cs = w.cs; I.pad = w.pad; I.Lp = w.Lp; I.c0 = w.c0; I.unit0 = w.unit0;
      I.n_chunks = w.n_chunks;
      I.ostride = m.stride; I.p0 = m.p0; I.p1 = m.p1; I.g_step = m.g_step; I.g0 = m.g0; I.g_lo = m.g_lo; I.g_hi = m.g_hi;
      I.padL = Q.A.g.padL; I.T = Q.A.g.T; I.Lout = Q.A.g.Lout; I.h_begin = Q.A.h_begin; I.h_end = Q.A.h_end;
      I.n_tiles = Q.A.n_tiles; I.scan_q = Q.scan_q;
      Q.plan = fast::op_plan_build(I);
    }
    // persistent workgroups (onepass.hpp "PERSIST"): the lazy first launch only -- its compare constants do not depend on the unit
    persist = C.fs.lazy && h->tile_order == 0 && !(h->lose_now & 3u) && C.total >= 2;
    if (persist && h->n_cu == 0) {
      int dev = 0, cus = 0;
      HIPCHK(h, hipGetDevice(&dev));
      HIPCHK(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
      h->n_cu = cus > 0 ? cus : 256;
    }
    // three workgroups per CU (LDS) is what is resident at once; every workgroup ends on one ticket past the last tile
    static const int pg_per_cu = [] { const char* e = getenv("SG_ONEPASS_WG_PER_CU"); int v = e ? atoi(e) : 3; return v >= 1 && v <= 3 ? v : 3; }();   // (experiments: fewer resident workgroups)
    if (persist) {
      C.grid = (unsigned)std::min<int64_t>(C.total, (int64_t)pg_per_cu * h->n_cu);
      C.tickets = C.total + C.grid;
    }
    if (h->tile_order == 1) {   // SG_OPT_TILE_ORDER 1: tile = block index (no ticket)
      Q.ticket_base = 0xffffffffu;
      C.tickets = 0;
    }
#if OP_TRACE
    HIPCHK(h, op_trace_attach(Q, C.total, (int)C.n_tiles + 2, st));
#endif
    return SG_OK;
  };
  const size_t lds = S.lds + (prop ? OP_PROP_LDS : 0);
  auto launch = [&](const fast::OnePassArgs& Q, bool redo, dim3 grid) {
    // <WAVES, PROP, LOSE, REDO, PERSIST>.  (The order of these lines is the order of the kernels in the code object.)
    void (*kern)(fast::OnePassArgs);
    if (!redo && persist) {
      if (prop) kern = fast::k_gate_onepass<WAVES, true, false, false, true>;
      else kern = fast::k_gate_onepass<WAVES, false, false, false, true>;
    } else if (!redo && (h->lose_now & 3u)) kern = fast::k_gate_onepass<WAVES, false, true>;   // test hook (PROP-free shape only)
    else if (!redo && prop) kern = fast::k_gate_onepass<WAVES, true>;
    else if (!redo) kern = fast::k_gate_onepass<WAVES, false>;
    else if (prop) kern = fast::k_gate_onepass<WAVES, true, false, true>;
    else kern = fast::k_gate_onepass<WAVES, false, false, true>;
    return launch_lds(kern, grid, dim3(WAVES * 64), lds, st, Q);
  };
  // the floor fix-up of a lazy call as one launch (onepass.hpp: k_floor_fix): the larger of the two roles' LDS
  auto fix = [&](const fast::OnePassArgs& Q, const fast::FloorFixPlan& fp, bool lose) {
    fast::FloorFixArgs X{};
    X.P = Q;
    X.vx = vx;
    X.tw64 = (const cx<double>*)h->tw64.p;
    X.wfull64 = (const double*)h->wfull64.p;
    X.arrive = (unsigned long long*)h->farrive.p;
    X.n_max = fp.n_max; X.blocks = fp.blocks;
    X.lose = lose ? 1u : 0u;
    constexpr size_t lds_max = (size_t)(fast::FFX_N + fast::FFX_WAVES * lpn<double>(fast::FFX_N)) * sizeof(cx<double>);
    const size_t lds_fix = std::max(lds, lds_max);
    if (prop) return launch_lds(fast::k_floor_fix<WAVES, true>, dim3(fp.grid), dim3(WAVES * 64), lds_fix, st, X);
    return launch_lds(fast::k_floor_fix<WAVES, false>, dim3(fp.grid), dim3(WAVES * 64), lds_fix, st, X);
  };
  const int rc = onepass_run(h, v, vx, g, ub, om, st, S, OP_ALIM_BLOCKS, P, first, launch, fix, dec);
  if (!rc) note_smooth(h, SG_SMOOTH_ONEPASS, 1, S.NF);
  return rc;
}

// float64 fused apply (apply64.hpp): K counts of stage_fused_mask -> output samples, everything in double
template <int WAVES, bool KMASK>
static hipError_t launch_apply_fast64(fast::Apply64Args& A, int64_t nh, int64_t ub, hipStream_t st) {
  constexpr int NH = 4 * WAVES - 3;
  const size_t lds = (size_t)(fast::FN + WAVES * 4 * fast::FSLOTS_D + 17) * sizeof(fast::cd);
  return launch_lds(fast::k_apply_fast64<WAVES, KMASK>, dim3((unsigned)((nh + NH - 1) / NH), (unsigned)ub), dim3(WAVES * 64), lds, st, A);
}

// mask_f64 == nullptr: the uint16 counts in h->K16 (stationary gate); else a float64 mask field [units][T][FS]
static int stage_apply_fast64(sg_handle* h, const View& v, const Geom& g, int64_t ub, const OutMap& om, hipStream_t st,
                              const double* mask_f64 = nullptr) {
  ProfScope ps(h, SG_STAGE_APPLY_FAST, st);
  fast::Apply64Args A;
  A.view = v; A.g = g; A.om = om;
  A.K = (const unsigned short*)h->K16.p;
  A.Mf = mask_f64;
  A.win = (const double*)h->wfull64.p;
  A.norm = (const double*)h->norm64.p;
  A.tw1024 = (const fast::cd*)h->tw64.p;
  A.kscale = mask_f64 ? 1.0 / 512.0 : 1.0 / ((double)h->ktot * 512.0);
  A.prop = h->p.prop_decrease;
  A.nf = h->p.smooth_mask ? h->p.n_grad_freq : 0;
  A.nt = h->p.smooth_mask ? h->p.n_grad_time : 0;
  const HopRange hr = hop_range(om, g, 256);
  A.h_begin = hr.h_begin;
  A.h_end = hr.h_end;
  const int64_t nh = hr.count();
  if (nh <= 0) return SG_OK;
  // tiles overlap by three frames: 8 wavefronts (32 frames -> 29 hops, 10 % of the transforms redone) unless the rows are
  // short; either way two wavefronts per SIMD (256 VGPRs) and one (8) or two (4) workgroups per CU
  static const int waves_env = getenv("SG_APPLY64_WAVES") ? atoi(getenv("SG_APPLY64_WAVES")) : 0;
  const bool wide = waves_env ? waves_env == 8 : nh >= 64;
  if (mask_f64) {
    if (wide) HIPCHK(h, (launch_apply_fast64<8, false>(A, nh, ub, st)));
    else HIPCHK(h, (launch_apply_fast64<4, false>(A, nh, ub, st)));
  } else {
    if (wide) HIPCHK(h, (launch_apply_fast64<8, true>(A, nh, ub, st)));
    else HIPCHK(h, (launch_apply_fast64<4, true>(A, nh, ub, st)));
  }
  return SG_OK;
}

// The stationary gate in float64 WITHOUT materialised float64 fields (default geometry, full reduction): the mask comes
// from the fused bit path -- decisions bit-identical to float64 decisions (k_decide_fast: float32 transform + exact
// refinement of ambiguous cells on the ORIGINAL samples), integer smoothing -- and k_apply_fast64 does the transforms,
// the mask multiply and the overlap-add in double.  Integer outputs (trunc(float64 result), base.py:217-226) and
// precision="float64" take it (route.hpp: exact_fused_ok; any prop_decrease: k_apply_fast64 forms p K + (1 - p) edge);
// everything else of the float64 contract stays on run_S_exact.
static int run_S_exact_fused(sg_handle* h, const route::SPlan& pl, View v, const Geom& g, int64_t total_units, int64_t ub,
                             const OutMap& om, hipStream_t st) {
  int rc = ensure_ws(h, g, ub, true);
  if (rc) return rc;
  // (other sample types than float32 are NOT converted to a float32 copy here: k_decide_fast stages (float)sample per tile
  // anyway, and its exact refinement and the float64 apply must read the ORIGINAL samples -- an int32 or float64 sample
  // has no exact float32 copy)
  for (int64_t u0 = 0; u0 < total_units; u0 += ub) {
    const int64_t nb = std::min(ub, total_units - u0);
    v.unit0 = u0;
    const HopRange hr = hop_range(om, g, 256);
    const int64_t tb = std::max<int64_t>(0, hr.h_begin - 3), te = std::min<int64_t>(g.T, hr.h_end);
    Decided dec;
    if ((rc = stage_fused_mask(h, pl, v, g, nb, tb, std::max(te, tb + 1), st, &dec))) return rc;
    if ((rc = stage_apply_fast64(h, v, g, nb, om, st))) return rc;
    note_batch(h, pl.facts, nb, g, dec);
  }
  return SG_OK;
}

// ------------------------------------------------------------------------------------------
// exact path (exact.hpp): float64 fields, materialised -- integer outputs (base.py:217-226 truncates a float64 result)
// ------------------------------------------------------------------------------------------
template <int N>
static hipError_t launch_xapply_n(const View& v, const Geom& g, int64_t units, const void* tw, const double* win,
                                  const double* M, double* seg, hipStream_t st) {
  constexpr int NT = N >= SG_TEAM_N ? 256 : 64;
  constexpr int WAVES = N >= SG_TEAM_N ? 1 : ((N * sizeof(cx<double>) > 16384) ? 2 : 4);
  constexpr int FPW = 4;
  const size_t lds = (size_t)(N + WAVES * lpn<double>(N)) * sizeof(cx<double>);
  auto kern = exact::kx_apply_istft<N, WAVES, FPW, NT>;
  dim3 grid((unsigned)((g.T + WAVES * FPW - 1) / (WAVES * FPW)), (unsigned)units);
  return launch_lds_if(lds > 65536, kern, grid, dim3(WAVES * NT), lds, st, v, g, (const cx<double>*)tw, win, M, seg);
}

template <int M>
static hipError_t launch_xapply_czt_m(const View& v, const Geom& g, int64_t units, const CztTabs<double>& tb,
                                      const double* win, const double* Mk, double* seg, hipStream_t st) {
  constexpr int NT = CztShape<M>::NT, FR = CztShape<M>::FR;
  const size_t lds = (size_t)FR * lpn<double>(M) * sizeof(cx<double>);
  auto kern = exact::kx_apply_istft_czt<M, NT, FR>;
  const int fpb = 4;
  dim3 grid((unsigned)((g.T + FR * fpb - 1) / (FR * fpb)), (unsigned)units);
  return launch_lds_if(lds > 65536, kern, grid, dim3(NT * FR), lds, st, v, g, tb, win, Mk, seg, fpb);
}

static hipError_t xapply_any(sg_handle* h, const View& v, const Geom& g, int64_t units, const double* Mk, double* seg,
                             hipStream_t st) {
  const double* win = (const double*)h->wfull64.p;
  if (h->big_M) {
    const int rc = big_apply<double, double>(h, v, g, units, Mk, seg, st);
    return rc == SG_OK ? hipSuccess : (rc == SG_E_NOMEM ? hipErrorOutOfMemory : hipErrorUnknown);
  }
  if (h->czt_M) {
    const CztTabs<double> tb = czt_tabs<double>(h);
#define SG_CALL(M) launch_xapply_czt_m<M>(v, g, units, tb, win, Mk, seg, st)
    SG_CZT_SWITCH(h->czt_M, SG_CALL);
#undef SG_CALL
  }
  switch (h->N) {
    case 32: return launch_xapply_n<32>(v, g, units, h->tw64.p, win, Mk, seg, st);
    case 64: return launch_xapply_n<64>(v, g, units, h->tw64.p, win, Mk, seg, st);
    case 128: return launch_xapply_n<128>(v, g, units, h->tw64.p, win, Mk, seg, st);
    case 256: return launch_xapply_n<256>(v, g, units, h->tw64.p, win, Mk, seg, st);
    case 512: return launch_xapply_n<512>(v, g, units, h->tw64.p, win, Mk, seg, st);
    case 1024: return launch_xapply_n<1024>(v, g, units, h->tw64.p, win, Mk, seg, st);
    case 2048: return launch_xapply_n<2048>(v, g, units, h->tw64.p, win, Mk, seg, st);
    case 4096: return launch_xapply_n<4096>(v, g, units, h->tw64.p, win, Mk, seg, st);
  }
  return hipErrorInvalidValue;
}

// float64 pipeline (exact.hpp; bytes per unit and units per batch: route.hpp, exact_unit_bytes)
static int run_S_exact(sg_handle* h, const route::SPlan& pl, View v, const Geom& g, int64_t total_units, int64_t ub,
                       const OutMap& om, hipStream_t st) {
  const size_t cells1 = (size_t)g.T * g.FS;
  int rc;
  const size_t cells = (size_t)ub * cells1;
  if ((rc = ensure(h, h->xP, cells * 8))) return rc;
  if ((rc = ensure(h, h->xraw, cells * 8))) return rc;
  if ((rc = ensure(h, h->xM, cells * 8))) return rc;
  if ((rc = ensure(h, h->xtmp, cells * 8))) return rc;
  // default geometry: k_apply_fast64 reads the float64 mask field and writes samples (no masked frames through HBM)
  const bool apply64 = pl.apply == route::Apply::FAST64_M;
  if (!apply64 && (rc = ensure(h, h->xseg, (size_t)ub * g.T * g.n * 8))) return rc;
  if ((rc = ensure(h, h->pmax, (size_t)ub * g.FS * 8))) return rc;
  const int nf = h->p.n_grad_freq, nt = h->p.n_grad_time;
  const double p = h->p.prop_decrease;
  double* P = (double*)h->xP.p;
  for (int64_t u0 = 0; u0 < total_units; u0 += ub) {
    const int64_t nb = std::min(ub, total_units - u0);
    v.unit0 = u0;
    const int64_t ncell = nb * g.T * g.FS;
    {
      ProfScope ps(h, SG_STAGE_STFT_POWER, st);
      if (h->p.stationary) HIPCHK(h, hipMemsetAsync(h->pmax.p, 0, (size_t)nb * g.FS * 8, st));
      HIPCHK(h, stft_any<double>(h, v, g, nb, P, nullptr, nullptr, 1.0, st,
                                 h->p.stationary ? (unsigned long long*)h->pmax.p : nullptr));
    }
    const int prop_before = h->p.stationary ? 1 : 0;
    if (h->p.stationary) {
      ProfScope ps(h, SG_STAGE_DECIDE, st);
      hipLaunchKernelGGL(k_decide, dim3(grid_1d(ncell, 256)), dim3(256), 0, st, (const double*)P, g,
                         (const double*)h->pmax.p, (const double*)h->thresh.p, (int64_t)0, h->mag_scale, h->p.top_db,
                         (float*)h->xraw.p, nb);
      HIPCHK(h, hipGetLastError());
    } else if (g.T >= 4 * exact::XIIR_TT && nb <= 65535 && pl.exact_tiled) {
      // (round 5) tile-parallel: partials of 32-frame tiles -> chain -> both sweeps per tile from the entering states
      ProfScope ps(h, SG_STAGE_NONSTAT_MASK, st);
      NsTiling tl{g.T, 0};
      tl.tt = exact::XIIR_TT;
      const int64_t nk = tl.n_tiles();
      const size_t bytes = (size_t)nb * nk * 2 * g.FS * sizeof(double);
      if ((rc = ensure(h, h->nsp, bytes))) return rc;
      if ((rc = ensure(h, h->nsc, bytes))) return rc;
      const dim3 gp((unsigned)((nk * g.FS + 255) / 256), (unsigned)nb);
      hipLaunchKernelGGL(exact::kx_iir_part, gp, dim3(256), 0, st, (const double*)P, g, tl, h->p.iir_b, (double*)h->nsp.p);
      HIPCHK(h, hipGetLastError());
      hipLaunchKernelGGL((k_iir_chain<double, true>), dim3((unsigned)((nb * g.FS + 63) / 64)), dim3(64), 0, st, (const double*)P,
                         (const double*)h->nsp.p, g, tl, h->p.iir_b, (double*)h->nsc.p, nb);
      HIPCHK(h, hipGetLastError());
      hipLaunchKernelGGL(exact::kx_iir_apply, gp, dim3(256), 0, st, (const double*)P, (const double*)h->nsc.p, g, tl, h->p.iir_b,
                         h->p.nonstat_thresh, h->p.nonstat_slope, (double*)h->xraw.p);
      HIPCHK(h, hipGetLastError());
    } else {
      ProfScope ps(h, SG_STAGE_NONSTAT_MASK, st);
      hipLaunchKernelGGL(exact::kx_iir_sigmoid, dim3((unsigned)((g.F + 63) / 64), (unsigned)nb), dim3(64), 0, st,
                         (const double*)P, g, h->p.iir_b, h->p.nonstat_thresh, h->p.nonstat_slope, (double*)h->xraw.p);
      HIPCHK(h, hipGetLastError());
    }
    {
      ProfScope ps(h, SG_STAGE_SMOOTH, st);
      const dim3 gr(grid_1d(ncell, 256));
      if (!h->p.smooth_mask) {
        if (h->p.stationary)
          hipLaunchKernelGGL(exact::kx_prop_only<float>, gr, dim3(256), 0, st, (const float*)h->xraw.p, g, p, (double*)h->xM.p, nb);
        else
          hipLaunchKernelGGL(exact::kx_prop_only<double>, gr, dim3(256), 0, st, (const double*)h->xraw.p, g, p, (double*)h->xM.p, nb);
        note_smooth(h, SG_SMOOTH_OFF, 8, 0);
      } else if (pl.exact_tiled && exact::xsm_lds_bytes(nf, nt) <= 150 * 1024 && 2 * nf < exact::XSM_KMAX && 2 * nt < exact::XSM_KMAX && nb <= 65535 &&
                 (g.T + exact::XSM_TT - 1) / exact::XSM_TT <= 65535) {
        // (round 5) both passes in one LDS-tiled kernel, taps computed once per block
        const size_t lds = exact::xsm_lds_bytes(nf, nt);
        note_smooth(h, SG_SMOOTH_X_TILED, 8, exact::XSM_TT);
        const dim3 gt((unsigned)((g.F + exact::XSM_FB - 1) / exact::XSM_FB), (unsigned)((g.T + exact::XSM_TT - 1) / exact::XSM_TT), (unsigned)nb);
        if (h->p.stationary)
          HIPCHK(h, launch_lds(exact::kx_smooth_tiled<float>, gt, dim3(exact::XSM_THREADS), lds, st, (const float*)h->xraw.p, g, nf, nt, p, prop_before, (double*)h->xM.p));
        else
          HIPCHK(h, launch_lds(exact::kx_smooth_tiled<double>, gt, dim3(exact::XSM_THREADS), lds, st, (const double*)h->xraw.p, g, nf, nt, p, prop_before, (double*)h->xM.p));
      } else {
        if (h->p.stationary)
          hipLaunchKernelGGL(exact::kx_smooth_f<float>, gr, dim3(256), 0, st, (const float*)h->xraw.p, g, nf, (double*)h->xtmp.p, nb);
        else
          hipLaunchKernelGGL(exact::kx_smooth_f<double>, gr, dim3(256), 0, st, (const double*)h->xraw.p, g, nf, (double*)h->xtmp.p, nb);
        HIPCHK(h, hipGetLastError());
        note_smooth(h, SG_SMOOTH_X_SEPARATE, 8, 0);
        hipLaunchKernelGGL(exact::kx_smooth_t, gr, dim3(256), 0, st, (const double*)h->xtmp.p, g, nt, nf, p, prop_before,
                           (double*)h->xM.p, nb);
      }
      HIPCHK(h, hipGetLastError());
    }
    // default geometry: transforms, mask multiply and overlap-add in ONE float64 kernel reading the mask field (round 5)
    // instead of masked frames through HBM + a gather
    if (apply64) {
      if ((rc = stage_apply_fast64(h, v, g, nb, om, st, (const double*)h->xM.p))) return rc;
      note_batch(h, pl.facts, nb, g);
      continue;
    }
    {
      ProfScope ps(h, SG_STAGE_APPLY_ISTFT, st);
      HIPCHK(h, xapply_any(h, v, g, nb, (const double*)h->xM.p, (double*)h->xseg.p, st));
    }
    const int64_t np = om.p1 - om.p0;
    if (np > 0) {
      ProfScope ps(h, SG_STAGE_OLA, st);
      hipLaunchKernelGGL(exact::kx_ola, dim3((unsigned)((np + 255) / 256), (unsigned)nb), dim3(256), 0, st, v, g, om,
                         (const double*)h->xseg.p, (const double*)h->wfull64.p);
      HIPCHK(h, hipGetLastError());
    }
    note_batch(h, pl.facts, nb, g);   // the exact path keeps no debug fields
  }
  return SG_OK;
}

// Variant S over a set of units described by `v` (unit0 filled per batch).  The route -- pipeline, stages, workspace form --
// is planned once (route.hpp: plan_S) and holds for every batch of the call.
static int run_S(sg_handle* h, View v, int64_t total_units, const OutMap& om, hipStream_t st) {
  using route::Pipe;
  using route::Apply;
  using route::NsMask;
  h->smooth_route = 0;   // (sg_debug_counter 17 speaks of THIS call: a path that notes nothing reports "none", not the call before)
  Geom g = make_geom(h, v.Lp);
  if (v.Lp < h->W) FAIL(h, SG_E_INVALID, "signal window of %lld samples is shorter than win_length=%d",
                        (long long)v.Lp, h->W);
  if (h->p.stationary && !h->has_thresh)
    FAIL(h, SG_E_STATE, "stationary gate: call sg_noise_stats or sg_set_noise_threshold first");
  const route::RouteCaps caps = route_caps(h);
  const route::RouteShape shape = route_shape(caps, g, om.p0, om.p1, v.dtype, om.dtype, total_units);
  const route::SPlan pl = route::plan_S(caps, shape);
  const int64_t ub = route::workspace_S(caps, pl, shape, total_units).ub;
  // integer outputs are the TRUNCATED float64 result of the reference (base.py:217-226): float64 pipeline
  if (pl.pipe == Pipe::EXACT_FUSED) return run_S_exact_fused(h, pl, v, g, total_units, ub, om, st);
  if (pl.pipe == Pipe::EXACT) return run_S_exact(h, pl, v, g, total_units, ub, om, st);
  // lean -- the one-pass gates (any prop_decrease) or, with prop_decrease == 1, the three-kernel bit-mask path: only bit /
  // count fields in the workspace
  int rc = ensure_ws(h, g, ub, pl.lean);
  if (rc) return rc;
  // Samples that are not float32: the register-FFT kernels would take the checked per-sample path for every
  // frame (in every kernel).  Convert the readable part of the rows ONCE -- (float)sample is what those kernels
  // compute anyway -- and keep the original view for the float64 work (exact refinement, floor pre-pass).
  const View vx = v;
  if (pl.f32_copy) {
    const int64_t rows = total_units / std::max<int64_t>(1, v.n_chunks), len = v.hi - v.lo;
    const size_t bytes = (size_t)rows * len * sizeof(float);
    if (len > 0 && bytes <= ((size_t)16 << 30)) {
      if ((rc = ensure(h, h->xin, bytes))) return rc;
      ProfScope ps(h, SG_STAGE_PREP, st);
      hipLaunchKernelGGL(k_to_f32, dim3(grid_1d(rows * len, 256)), dim3(256), 0, st, v.x, v.dtype, v.stride, v.lo, len, rows,
                         (float*)h->xin.p);
      HIPCHK(h, hipGetLastError());
      v.x = (const float*)h->xin.p - v.lo;   // index g of row r -> xin[r * len + (g - lo)]
      v.dtype = SG_F32;
      v.stride = len;
    }
  }
  const RegGeom* r = pl.reg ? h->reg : nullptr;
  const float* const Mf = (const float*)h->M.p;
  PiecePows pows;
  for (int64_t u0 = 0; u0 < total_units; u0 += ub) {
    int64_t nb = std::min(ub, total_units - u0);
    v.unit0 = u0;
    Decided dec;
    if (pl.pipe == Pipe::ONEPASS || pl.pipe == Pipe::ONEPASS_REG) {
      View vxb = vx;
      vxb.unit0 = u0;
      if (pl.pipe == Pipe::ONEPASS) rc = stage_onepass(h, v, vxb, g, nb, om, st, &dec);
      else rc = stage_onepass_reg(h, r, v, vxb, g, nb, om, pl.seam, st, &dec);
      if (rc) return rc;
      note_batch(h, pl.facts, nb, g, dec);
      continue;
    }
    if (pl.pipe == Pipe::BITS3) {
      // frames the fused apply kernel touches: hops [h_begin, h_end) need frames h-3 .. h
      const HopRange hr = hop_range(om, g, 256);
      const int64_t tb = std::max<int64_t>(0, hr.h_begin - 3), te = std::min<int64_t>(g.T, hr.h_end);
      if ((rc = stage_fused_mask(h, pl, v, g, nb, tb, std::max(te, tb + 1), st, &dec))) return rc;
    } else if (pl.pipe == Pipe::FUSED) {
      // float mask field (natural bin order for the general apply kernels, lane order for the fused one), or K counts
      if ((rc = stage_fused_mask(h, pl, v, g, nb, 0, g.T, st, &dec))) return rc;
    } else {
      if (pl.ns == NsMask::NONE) {
        if ((rc = stage_power(h, v, g, nb, st))) return rc;
        if ((rc = stage_decide(h, g, nb, (const double*)h->thresh.p, 0, st))) return rc;
      } else if (pl.ns == NsMask::RAW) {
        if ((rc = stage_nonstat_raw(h, v, g, nb, st))) return rc;
      } else {
        if ((rc = stage_nonstat_mask2(h, v, g, nb, pl.ns == NsMask::SMOOTHED, st, &pows))) return rc;
      }
      if (pl.smooth_stage && (rc = stage_smooth(h, g, nb, st))) return rc;
    }
    switch (pl.apply) {
      case Apply::FAST_K: rc = stage_apply_fast(h, v, g, nb, om, nullptr, 1, st); break;
      case Apply::FAST_M: rc = stage_apply_fast(h, v, g, nb, om, Mf, 1, st); break;
      case Apply::REG_K: rc = stage_apply_reg(h, r, v, g, nb, om, nullptr, 1, st); break;   // the bit-mask stages left uint16 sums, no float mask
      case Apply::REG_M: rc = stage_apply_reg(h, r, v, g, nb, om, Mf, 1, st); break;
      case Apply::OLA_K: rc = stage_apply_ola(h, v, g, nb, nullptr, om, 1, st, (const unsigned short*)h->K16.p, 1.0f / (float)h->ktot); break;
      default: rc = stage_apply_ola(h, v, g, nb, Mf, om, 1, st); break;
    }
    if (rc) return rc;
    note_batch(h, pl.facts, nb, g, dec);
  }
  return SG_OK;
}

// (TorchGate.forward of whole rows in one kernel, rowgate.hpp: route.hpp, rowgate_ok)
static int stage_row_gate(sg_handle* h, const View& v, const Geom& g, int64_t nb, const OutMap& om, float* mask_out,
                          hipStream_t st) {
  int rc;
  if ((rc = ensure(h, h->bits, (size_t)nb * g.T * 9 * 8))) return rc;
  if ((rc = ensure_zeroed(h, h->rg_count, 64, st))) return rc;
  fast::RowGateArgs A;
  A.view = v; A.g = g; A.om = om;
  A.win = (const float*)h->wa32.p;
  A.wsq = (const float*)h->wsq32.p;
  A.invn = (const float*)h->invn.p;
  A.tw512 = (const fast::cf*)h->tw512.p;
  A.tw1024 = (const fast::cf*)h->tw32.p;
  A.win64 = (const double*)h->wfull64.p;
  A.tw64 = (const cx<double>*)h->tw64.p;
  A.mag_scale = h->mag_scale; A.top_db = h->p.top_db; A.n_std = h->p.n_std_thresh; A.ddof = h->p.ddof;
  A.nf = h->p.n_grad_freq; A.nt = h->p.n_grad_time;
  A.kscale = (float)(1.0 / ((double)h->ktot * 512.0));
  A.inv_ktot = 1.0f / (float)h->ktot;
  A.mask_out = mask_out;
  A.bits_out = (unsigned long long*)h->bits.p;
  A.n_exact = (unsigned*)h->rg_count.p;
  A.ptile_out = nullptr;
  if (h->rg_tap) {   // SG_OPT_ROWGATE_TAP: float32 powers of pass 1 -> h->M ([rows][64][528] floats), fetched with sg_debug_fetch(4)
    if ((rc = ensure(h, h->M, (size_t)nb * 64 * fast::RG_PP * 4))) return rc;
    A.ptile_out = (float*)h->M.p;
  }
#if RG_TRACE
  {
    // development builds: [rows][16] stamps of the LAST launch, averaged per phase at exit
    static unsigned long long* tr = nullptr;
    static size_t tr_rows = 0;
    if (!tr || tr_rows < (size_t)nb) {
      HIPCHK(h, hipMalloc((void**)&tr, (size_t)nb * 128));
      tr_rows = (size_t)nb;
      static unsigned long long** trp = &tr;
      static size_t* trn = &tr_rows;
      static bool reg = false;
      if (!reg) {
        reg = true;
        atexit([] {
          std::vector<unsigned long long> hst(*trn * 16);
          if (hipMemcpy(hst.data(), *trp, hst.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
          double sum[12] = {0};
          for (size_t i = 0; i < *trn; ++i)
            for (int k = 1; k < 12; ++k) sum[k] += (double)(hst[i * 16 + k] - hst[i * 16 + k - 1]);
          {
            double a = 0, b = 0, c = 0, d = 0;
            for (size_t i = 0; i < *trn; ++i) {
              d += (double)(hst[i * 16 + 14] - hst[i * 16 + 6]);
              a += (double)(hst[i * 16 + 12] - hst[i * 16 + 14]); b += (double)(hst[i * 16 + 13] - hst[i * 16 + 12]);
              c += (double)(hst[i * 16 + 7] - hst[i * 16 + 13]);
            }
            fprintf(stderr, "[RG_TRACE] phase 7 of wave 0: after barrier %.0f, zero fill %.0f, tasks %.0f, barrier wait %.0f\n", d / *trn, a / *trn, b / *trn, c / *trn);
          }
          fprintf(stderr, "[RG_TRACE] rows %zu; average shader cycles per phase:", *trn);
          double tot = 0;
          for (int k = 1; k < 12; ++k) { fprintf(stderr, " %d:%.0f", k, sum[k] / *trn); tot += sum[k] / *trn; }
          fprintf(stderr, "  sum %.0f\n", tot);
        });
      }
    }
    A.trace = tr;
  }
#endif
  ProfScope ps(h, SG_STAGE_ROW_GATE, st);
  const size_t lds = fast::rowgate_lds_bytes();
  if (h->rg_shape == 8) {     // SG_OPT_ROWGATE_SHAPE: 8 waves x 2 quads (256 VGPRs, no scratch)
    HIPCHK(h, launch_lds(fast::k_row_gate<8, 2>, dim3((unsigned)nb), dim3(512), lds, st, A));
  } else {                    // default: 16 waves x 1 quad
    HIPCHK(h, launch_lds(fast::k_row_gate<16, 1>, dim3((unsigned)nb), dim3(1024), lds, st, A));
  }
  note_smooth(h, SG_SMOOTH_ROW_GATE, 1, fast::RG_FRAMES);
  return SG_OK;
}

// Rows of L samples read whole: one unit per row, no chunks, no padding, no halos, first unit 0.
static View rows_view(const void* ptr, int dtype, int64_t stride, int64_t L) {
  View v{};
  v.x = ptr; v.dtype = dtype; v.stride = stride; v.N = L; v.lo = 0; v.hi = L; v.cs = 0; v.pad = 0; v.Lp = L; v.n_chunks = 1;
  return v;
}

// Rows of n samples written whole: positions [0, n) of a unit to [0, n) of its row.
static OutMap whole_out(void* ptr, int dtype, int64_t stride, int64_t n) {
  OutMap om{};
  om.out = ptr; om.dtype = dtype; om.stride = stride;
  om.p0 = 0; om.p1 = n; om.g_step = 0; om.g0 = 0; om.g_lo = 0; om.g_hi = n;
  return om;
}

extern "C" int sg_workspace_bytes(const sg_handle* h, int64_t C, int64_t N, int32_t chunked, int64_t* bytes) {
  if (!h || !bytes || C < 1 || N < 1) return SG_E_INVALID;
  const int64_t cs = h->p.chunk_size, pad = h->p.padding;
  const int64_t Lp = chunked ? cs + 2 * pad : N + 2 * pad;
  const int64_t units = chunked ? C * ((N + cs - 1) / cs) : C;
  if (Lp < h->W) return SG_E_INVALID;
  const Geom g = make_geom(h, Lp);
  // What run_S's route allocates (route.hpp: plan_S, workspace_S), for the whole range of the recording: the fields of a
  // batch, the exchange buffers of the in-launch hand-offs and seams, the float32 copy of a recording that is not float32
  // (UPPER bound: the entry point has no dtype argument, and float32 recordings do not pay it), the long frames' two work
  // buffers of <= 256 MB (big.hpp).
  const route::RouteCaps caps = route_caps(h);
  route::RouteShape shape = route_shape(caps, g, pad, pad + (chunked ? cs : N), SG_I16, SG_F32, units);
  auto figure = [&](route::SPlan pl) {
    // (the float64 pipeline at its materialised figure, 32 B per cell + float64 frames, whichever of its forms would run)
    if (pl.pipe == route::Pipe::EXACT_FUSED) { pl = route::SPlan{}; pl.pipe = route::Pipe::EXACT; }
    const route::Workspace w = route::workspace_S(caps, pl, shape, units);
    int64_t t = w.total();
    if (pl.f32_copy) t += C * N * (int64_t)sizeof(float);
    if (caps.geom == route::GeomClass::LONG) t += 2 * big_batch(h, units * g.T) * (int64_t)h->big_M * (int64_t)sizeof(big::cd);
    return t;
  };
  int64_t total = figure(route::plan_S(caps, shape));
  // Integer (SG_I16 / SG_I32) outputs take the float64 pipeline by default, SG_OPT_FORCE_EXACT selects it for every dtype.
  // No dtype argument here either, so the figure is the LARGER of the two outputs' routes (they are one route when the
  // handle can never take the float64 pipeline for this call, SG_OPT_FAST_INTEGER, or always does) -- an upper bound, as
  // documented in the header.
  shape.out_dtype = SG_I16;
  if (caps.variant == SG_VARIANT_S) total = std::max(total, figure(route::plan_S(caps, shape)));
  *bytes = total;
  return SG_OK;
}

// ------------------------------------------------------------------------------------------
// variant S entry points
// ------------------------------------------------------------------------------------------
extern "C" int sg_noise_stats(sg_handle* h, const void* noise_dev, int dtype, int64_t C, int64_t n,
                              int64_t row_stride, void* stream) {
  if (!h) return SG_E_INVALID;
  if (!noise_dev || !dtype_ok(dtype) || C < 1 || n < 1) FAIL(h, SG_E_INVALID, "sg_noise_stats: bad argument");
  if (h->p.variant != SG_VARIANT_S) FAIL(h, SG_E_INVALID, "sg_noise_stats is a variant-S entry point");
  if (n < h->W) FAIL(h, SG_E_INVALID, "noise clip of %lld samples is shorter than win_length=%d", (long long)n, h->W);
  hipStream_t st = (hipStream_t)stream;
  struct Tag {
    sg_handle* h;
    explicit Tag(sg_handle* h_) : h(h_) { h->prof_override = SG_STAGE_NOISE_STATS; }
    ~Tag() { h->prof_override = -1; }
  } tag(h);
  int rc = SG_OK;
  View v = rows_view(noise_dev, dtype, row_stride, n);  // one channel: its mean is the channel itself
  if (C > 1) {
    if ((rc = ensure(h, h->yn, (size_t)n * sizeof(double)))) return rc;
    ProfScope ps(h, SG_STAGE_CHANNEL_MEAN, st);
    hipLaunchKernelGGL(k_channel_mean, dim3(grid_1d(n, 256)), dim3(256), 0, st, noise_dev, dtype, C, n,
                       row_stride, (double*)h->yn.p);
    HIPCHK(h, hipGetLastError());
    v = rows_view(h->yn.p, SG_F64, n, n);
  }
  Geom g = make_geom(h, n);
  if ((rc = ensure_ws(h, g, 1))) return rc;
  h->t2_ready = false;
  if ((rc = stage_stats(h, v, g, 1, (double*)h->thresh.p, st, /*gate_consts=*/h->fast_ok || h->reg))) return rc;
  h->has_thresh = true;
  return SG_OK;
}

extern "C" int sg_get_noise_threshold(sg_handle* h, double* thresh_host, int32_t n_bins, void* stream) {
  if (!h) return SG_E_INVALID;
  if (!thresh_host || n_bins != h->F) FAIL(h, SG_E_INVALID, "sg_get_noise_threshold: n_bins must be %d", h->F);
  if (!h->has_thresh) FAIL(h, SG_E_STATE, "no noise threshold set");
  HIPCHK(h, hipMemcpyAsync(thresh_host, h->thresh.p, (size_t)h->F * sizeof(double), hipMemcpyDeviceToHost,
                           (hipStream_t)stream));
  HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
  return handoff_verdict(h);
}

extern "C" int sg_set_noise_threshold(sg_handle* h, const double* thresh_host, int32_t n_bins, void* stream) {
  if (!h) return SG_E_INVALID;
  if (!thresh_host || n_bins != h->F) FAIL(h, SG_E_INVALID, "sg_set_noise_threshold: n_bins must be %d", h->F);
  h->t2_ready = false;
  HIPCHK(h, hipMemcpyAsync(h->thresh.p, thresh_host, (size_t)h->F * sizeof(double), hipMemcpyHostToDevice,
                           (hipStream_t)stream));
  HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
  h->has_thresh = true;
  return SG_OK;
}

extern "C" int sg_get_noise_threshold_dev(sg_handle* h, double* thresh_dev, int32_t n_bins, void* stream) {
  if (!h) return SG_E_INVALID;
  if (!thresh_dev || n_bins != h->F) FAIL(h, SG_E_INVALID, "sg_get_noise_threshold_dev: n_bins must be %d", h->F);
  if (!h->has_thresh) FAIL(h, SG_E_STATE, "no noise threshold set");
  HIPCHK(h, hipMemcpyAsync(thresh_dev, h->thresh.p, (size_t)h->F * sizeof(double), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
  return SG_OK;
}

extern "C" int sg_set_noise_threshold_dev(sg_handle* h, const double* thresh_dev, int32_t n_bins, void* stream) {
  if (!h) return SG_E_INVALID;
  if (!thresh_dev || n_bins != h->F) FAIL(h, SG_E_INVALID, "sg_set_noise_threshold_dev: n_bins must be %d", h->F);
  h->t2_ready = false;
  HIPCHK(h, hipMemcpyAsync(h->thresh.p, thresh_dev, (size_t)h->F * sizeof(double), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
  h->has_thresh = true;
  return SG_OK;
}

extern "C" int sg_process_chunks(sg_handle* h, const void* in_dev, int in_dtype, void* out_dev, int out_dtype,
                                 int64_t C, int64_t N, int64_t in_stride, int64_t out_stride,
                                 int64_t start_frame, int64_t end_frame, int32_t chunked, int64_t halo_left,
                                 int64_t halo_right, void* stream) {
  if (!h) return SG_E_INVALID;
  if (h->p.variant != SG_VARIANT_S) FAIL(h, SG_E_INVALID, "sg_process_chunks is a variant-S entry point");
  if (!in_dev || !out_dev || !dtype_ok(in_dtype) || !dtype_ok(out_dtype) || C < 1 || N < 1)
    FAIL(h, SG_E_INVALID, "sg_process_chunks: bad argument");
  if (start_frame < 0 || end_frame > N || start_frame >= end_frame)
    FAIL(h, SG_E_INVALID, "sg_process_chunks: bad frame range [%lld, %lld)", (long long)start_frame,
         (long long)end_frame);
  const int64_t cs = h->p.chunk_size, pad = h->p.padding;
  if (halo_left < 0 || halo_right < 0) FAIL(h, SG_E_INVALID, "sg_process_chunks: negative halo");
  View v{};
  v.x = in_dev; v.dtype = in_dtype; v.stride = in_stride; v.N = N; v.pad = pad;
  v.lo = -halo_left; v.hi = N + halo_right;
  OutMap om{};
  om.out = out_dev; om.dtype = out_dtype; om.stride = out_stride; om.g0 = start_frame;
  om.g_lo = start_frame; om.g_hi = end_frame;
  int64_t units;
  if (chunked) {
    // base.py:175-216: chunks ich1..ich2, each filtered over [i*cs - pad, (i+1)*cs + pad)
    // only the chunks that overlap [start_frame, end_frame) become units
    int64_t ich1 = start_frame / cs, ich2 = (end_frame - 1) / cs;
    int64_t n_chunks = ich2 - ich1 + 1;
    v.cs = cs; v.Lp = cs + 2 * pad; v.n_chunks = (int32_t)n_chunks; v.c0 = ich1;
    om.p0 = pad; om.p1 = pad + cs; om.g_step = cs;
    units = C * n_chunks;
  } else {
    // base.py:222: one window [-pad, end_frame + pad) -- start_frame is ignored by the reference
    v.cs = 0; v.Lp = end_frame + 2 * pad; v.n_chunks = 1;  // _read_chunk may read past end_frame (base.py:136-141)
    om.p0 = pad; om.p1 = pad + end_frame; om.g_step = 0;
    om.g_lo = 0; om.g0 = 0;
    units = C;
  }
  return run_S(h, v, units, om, (hipStream_t)stream);
}

extern "C" int sg_filter_padded(sg_handle* h, const void* chunk_dev, int in_dtype, void* out_dev, int out_dtype,
                                int64_t C, int64_t Lp, int64_t in_stride, int64_t out_stride, void* stream) {
  if (!h) return SG_E_INVALID;
  if (h->p.variant != SG_VARIANT_S) FAIL(h, SG_E_INVALID, "sg_filter_padded is a variant-S entry point");
  if (!chunk_dev || !out_dev || !dtype_ok(in_dtype) || !dtype_ok(out_dtype) || C < 1 || Lp < 1)
    FAIL(h, SG_E_INVALID, "sg_filter_padded: bad argument");
  return run_S(h, rows_view(chunk_dev, in_dtype, in_stride, Lp), C, whole_out(out_dev, out_dtype, out_stride, Lp),
               (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// variant T
// ------------------------------------------------------------------------------------------
// The gated spectrogram of one sub-batch (spec.hpp): rfft(window * frame) * mask -> spec_dev[u0 ..][T][F], mask in natural bin order.
static int stage_spectrum(sg_handle* h, const View& v, const Geom& g, int64_t u0, int64_t nb, const float* mask, void* spec_dev,
                          int dtype, hipStream_t st) {
  ProfScope ps(h, SG_STAGE_APPLY_ISTFT, st);
  char* dst = (char*)spec_dev + (size_t)u0 * g.T * g.F * 2 * elem_bytes(dtype);
  HIPCHK(h, spec_forward(v, g, nb, h->tw32.p, (const float*)h->wa32.p, mask, dst, dtype, st));
  return SG_OK;
}

// What sg_gate_features asks of process_batch_impl: the features of the masked spectrogram instead of the spectrogram.
struct FeatSink {
  void* feat_dev;   // [B][T][M] of the input's dtype
  int power, take_log;
  double eps;
};

// The filterbank features of one sub-batch (feat.hpp), where stage_spectrum stores the spectrogram: -> feat_dev[u0 ..][T][M].
static int stage_features(sg_handle* h, const View& v, const Geom& g, int64_t u0, int64_t nb, const float* mask,
                          const FeatSink& fs, int dtype, hipStream_t st) {
  ProfScope ps(h, SG_STAGE_APPLY_ISTFT, st);
  char* dst = (char*)fs.feat_dev + (size_t)u0 * g.T * h->n_filters * elem_bytes(dtype);
  HIPCHK(h, feat_forward(v, g, nb, h->tw32.p, (const float*)h->wa32.p, mask, feat_bank(h), fs.power, fs.take_log, fs.eps, dst,
                         dtype, st));
  return SG_OK;
}

// Where process_batch_impl sends a gated batch: through the inverse transform to a waveform, or the masked spectrogram
// itself, or its filterbank features.
struct Sink {
  enum Kind { WAVEFORM, SPECTRUM, FEATURES } kind;
  void* out; int dtype; int64_t stride;   // WAVEFORM: [B][stride] of dtype
  void* spec;                             // SPECTRUM: [B][T][F] pairs of the input's dtype
  FeatSink feat;                          // FEATURES
};

// The stationary decisions of one sub-batch (v.unit0 = u0): the thresholds (pl.thresh: the shared noise row's in h->thresh,
// each row's own noise, or the rows themselves), the power field and the compare.  With pl.bits_path (default geometry, full
// reduction: the stages of the variant-S fused path) the decisions are bits in h->bits, and with pl.to_raw also the 0 / 1
// float field in h->raw; without it the float field of stage_decide.  *branch: which statement decided (sg_debug_counter
// 18), 0 when the bits are all that is left.
static int decide_stationary(sg_handle* h, const route::TPlan& pl, const View& v, View vn, const Geom& g, const Geom& gn,
                             int64_t nb, hipStream_t st, int64_t* branch) {
  int rc;
  double* thr = (double*)h->thr_rows.p;
  const double* th;
  int64_t ustride;
  const bool bits_path = pl.bits_path, row_fused = pl.row_fused, to_raw = pl.to_raw;
  if (pl.thresh == route::Thresh::SHARED) {
    th = (const double*)h->thresh.p; ustride = 0;
  } else if (pl.thresh == route::Thresh::PER_ROW) {
    vn.unit0 = v.unit0;
    if ((rc = stage_stats(h, vn, gn, nb, thr, st))) return rc;
    th = thr; ustride = g.FS;
  } else {
    th = nullptr; ustride = g.FS;
  }
  // short rows: statistics + constants + decisions of a (row, 64 bands) tile in one kernel
  const size_t tile_bytes = (size_t)g.T * 64 * sizeof(double);
  if (row_fused) {
    ProfScope ps(h, SG_STAGE_STFT_POWER, st);
    HIPCHK(h, stft_any<double>(h, v, g, nb, (double*)h->P.p, nullptr, nullptr, 1.0, st));
  } else {
    if ((rc = stage_power(h, v, g, nb, st))) return rc;
    if (!th) {
      if ((rc = stage_colstats(h, g, nb, thr, st))) return rc;
      th = thr;
    }
  }
  if (!bits_path) {
    *branch = SG_SPEC_DECIDE;
    return stage_decide(h, g, nb, th, ustride, st);
  }
  const int wpr = (g.F + 63) / 64;
  if ((rc = ensure(h, h->bits, (size_t)nb * g.T * wpr * 8))) return rc;
  if ((rc = ensure(h, h->K16, (size_t)nb * g.T * g.FS * 2))) return rc;
  if ((rc = ensure(h, h->T2, (size_t)nb * g.FS * 8))) return rc;
  if (row_fused) {
    ProfScope ps(h, SG_STAGE_DECIDE, st);
    hipLaunchKernelGGL(k_row_decide, dim3((unsigned)wpr, (unsigned)nb), dim3(64 * STAT_TG), tile_bytes, st,
                       (const double*)h->P.p, g, th, ustride, h->mag_scale, h->p.top_db, h->p.n_std_thresh,
                       h->p.ddof, (double*)h->pmax.p, th ? nullptr : thr, (unsigned long long*)h->bits.p,
                       wpr, db_fast_consts(h));
    HIPCHK(h, hipGetLastError());
  } else {
    ProfScope ps(h, SG_STAGE_DECIDE, st);
    // compare constants in the power domain per (row, band), then a pure compare per cell
    hipLaunchKernelGGL(k_t2_rows, dim3(grid_1d(nb * g.FS, 256)), dim3(256), 0, st, th, ustride,
                       (const double*)h->pmax.p, g, h->mag_scale, h->p.top_db, (double*)h->T2.p, nb);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_decide_bits_t2, dim3(grid_1d(nb * g.T * wpr * 64, 256)), dim3(256), 0, st,
                       (const double*)h->P.p, g, (const double*)h->T2.p, (unsigned long long*)h->bits.p, wpr,
                       nb);
    HIPCHK(h, hipGetLastError());
  }
  *branch = 0;
  if (!to_raw) return SG_OK;
  // the spectrogram kernel reads a float mask in natural bin order: the decision bits as a 0 / 1 field, smoothed by
  // the float kernels -- bitwise the mask process_batch_impl writes without the bit-mask route, at every geometry
  ProfScope ps(h, SG_STAGE_DECIDE, st);
  HIPCHK(h, spec_bits_to_raw((const unsigned long long*)h->bits.p, g, wpr, (float*)h->raw.p, nb, st));
  *branch = (row_fused ? SG_SPEC_ROW_DECIDE : SG_SPEC_T2_BITS) | SG_SPEC_BITS_TO_RAW;
  return SG_OK;
}

// sg_process_batch, sg_gate_spectrum and sg_gate_features: per sub-batch the decisions, the smoothing and the sink.  With
// a spectrum or feature sink the one-launch row gate is not taken, and the bit-mask route hands its decisions to the
// float smoothing kernels instead of the integer ones: the mask is then the float field of the general route (h->M) at
// every geometry.
static int process_batch_impl(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                              const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride, const Sink& sink,
                              float* mask_out_dev, void* stream) {
  const bool field = sink.kind != Sink::WAVEFORM;   // the mask is wanted as a float field in natural bin order
  int rc;
  if ((rc = t_min_lengths(h, B, L, xn_dev, Bn, Ln))) return rc;
  hipStream_t st = (hipStream_t)stream;
  h->smooth_route = 0;   // (as in run_S)
  View v = rows_view(x_dev, dtype, x_stride, L);
  Geom g = make_geom(h, L);
  const OutMap om = whole_out(sink.out, sink.dtype, sink.stride, g.Lout);
  const bool noise = xn_dev && h->p.stationary;
  View vn{};
  Geom gn{};
  if (noise) {
    vn = rows_view(xn_dev, dtype, xn_stride, Ln);
    gn = make_geom(h, Ln);
  }
  // size the workspace for the larger of the two geometries
  Geom gbig = (noise && gn.T > g.T) ? gn : g;
  int64_t ub = units_per_batch(h, gbig, B);
  if ((rc = ensure_ws(h, gbig, ub))) return rc;
  if (noise && Bn == 1 && (rc = stage_stats(h, vn, gn, 1, (double*)h->thresh.p, st))) return rc;
  const route::RouteCaps caps = route_caps(h);
  route::RouteShape shape = route_shape(caps, g, om.p0, om.p1, dtype, sink.dtype, B);
  shape.field = field; shape.noise_rows = xn_dev ? Bn : 0;
  const route::TPlan pl = route::plan_T(caps, shape);
  const bool smooths = pl.smooths;
  int64_t n_sub = 0;
  for (int64_t u0 = 0; u0 < B; u0 += ub) {
    int64_t nb = std::min(ub, B - u0);
    int64_t branch = 0;   // (host bookkeeping behind sg_debug_counter 18: which statement below decided this sub-batch)
    float* const mask_out = mask_out_dev ? mask_out_dev + (size_t)u0 * g.T * g.FS : nullptr;
    v.unit0 = u0;
    // 1. the decisions
    if (pl.rowgate) {
      // one kernel per call: a workgroup per row (rowgate.hpp)
      if ((rc = stage_row_gate(h, v, g, nb, om, mask_out, st))) return rc;
      note_batch(h, pl.facts, nb, g);
      continue;
    }
    if (pl.ns == route::NsMask::NONE) {
      if ((rc = decide_stationary(h, pl, v, vn, g, gn, nb, st, &branch))) return rc;
      if (pl.apply == route::Apply::FAST_K) {
        // the bits straight through the integer smoothing into the fused apply kernel
        if ((rc = stage_smooth_bits(h, g, nb, true, 0, g.T, st))) return rc;
        if (mask_out) {  // float mask (natural bin order) for the backward pass
          hipLaunchKernelGGL(k_k16_to_mask_perm, dim3(grid_1d(nb * g.T * g.FS, 256)), dim3(256), 0, st,
                             (const unsigned short*)h->K16.p, g, 1.0f / (float)h->ktot, mask_out, nb);
          HIPCHK(h, hipGetLastError());
        }
        if ((rc = stage_apply_fast(h, v, g, nb, om, nullptr, 1, st))) return rc;
        note_batch(h, pl.facts, nb, g);
        continue;
      }
    } else if (pl.ns == route::NsMask::BOX) {
      if ((rc = stage_box_mask(h, v, g, nb, st))) return rc;
      branch = SG_SPEC_BOX_MASK;
    } else {
      if ((rc = stage_nonstat_raw(h, v, g, nb, st))) return rc;
      branch = SG_SPEC_NONSTAT_RAW;
    }
    // 2. the smoothing.  The spectrogram reads the mask wherever it lies: smoothed straight into the caller's buffer,
    // without the copy below
    float* const mask_direct = (field && smooths) ? mask_out : nullptr;
    if (smooths && (rc = stage_smooth(h, g, nb, st, mask_direct))) return rc;
    if (mask_out && !mask_direct)
      HIPCHK(h, hipMemcpyAsync(mask_out, h->M.p, (size_t)nb * g.T * g.FS * 4, hipMemcpyDeviceToDevice, st));
    // 3. the sink
    const float* const mask = mask_direct ? mask_direct : (const float*)h->M.p;
    if (sink.kind == Sink::SPECTRUM) {
      if ((rc = stage_spectrum(h, v, g, u0, nb, mask, sink.spec, dtype, st))) return rc;
      h->spec_route = branch | (mask_direct ? SG_SPEC_MASK_DIRECT : 0) | (++n_sub << 16);
    } else if (sink.kind == Sink::FEATURES) {
      if ((rc = stage_features(h, v, g, u0, nb, mask, sink.feat, dtype, st))) return rc;
    } else if (pl.apply == route::Apply::FAST_M) {
      if ((rc = stage_apply_fast(h, v, g, nb, om, (const float*)h->M.p, 1, st))) return rc;
    } else if (pl.apply == route::Apply::REG_M) {
      if ((rc = stage_apply_reg(h, h->reg, v, g, nb, om, (const float*)h->M.p, 1, st))) return rc;
    } else {
      if ((rc = stage_apply_ola(h, v, g, nb, (const float*)h->M.p, om, 1, st))) return rc;
    }
    note_batch(h, pl.facts, nb, g);
  }
  return SG_OK;
}

extern "C" int sg_process_batch(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride, void* out_dev,
                                int out_dtype, int64_t out_stride, float* mask_out_dev, void* stream) {
  if (int rc = t_entry(h, "sg_process_batch")) return rc;
  if (!x_dev || !out_dev || !dtype_ok(dtype) || !dtype_ok(out_dtype) || B < 1)
    FAIL(h, SG_E_INVALID, "sg_process_batch: bad argument");
  const Sink sink{Sink::WAVEFORM, out_dev, out_dtype, out_stride, nullptr, {}};
  return process_batch_impl(h, x_dev, dtype, B, L, x_stride, xn_dev, Bn, Ln, xn_stride, sink, mask_out_dev, stream);
}

// TorchGate.gated_stft: X * mask in torch.stft's layout (spec.hpp)
extern "C" int sg_gate_spectrum(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride, void* spec_dev,
                                float* mask_out_dev, void* stream) {
  if (int rc = t_entry(h, "sg_gate_spectrum")) return rc;
  h->spec_route = 0;   // (sg_debug_counter 18 speaks of THIS call; only a variant-T handle ever sets it)
  if (!x_dev || !spec_dev || (dtype != SG_F32 && dtype != SG_F64) || B < 1)
    FAIL(h, SG_E_INVALID, "sg_gate_spectrum: bad argument");
  if (!spectrum_geom_ok(h))
    FAIL(h, SG_E_UNSUPPORTED, "sg_gate_spectrum: n_fft=%d (powers of two from 256 to 4096 only)", h->n);
  const Sink sink{Sink::SPECTRUM, nullptr, dtype, 0, spec_dev, {}};
  return process_batch_impl(h, x_dev, dtype, B, L, x_stride, xn_dev, Bn, Ln, xn_stride, sink, mask_out_dev, stream);
}

// The backward of the spectrum and feature outputs, per sub-batch: `frames(u0, nb, mask, seg)` launches the windowed adjoint
// frames of rows [u0, u0 + nb) into h->seg (mask: theirs), then one gather (the adjoint of an STFT: every bin with weight 1
// and no envelope division) adds them onto grad_x.
template <class Frames>
static int spectrum_backward_loop(sg_handle* h, int dtype, int64_t B, int64_t L, const float* mask_dev, void* grad_x_dev,
                                  int64_t gx_stride, hipStream_t st, Frames frames) {
  const Geom g = make_geom(h, L);
  const int64_t ub = units_per_batch(h, g, B);
  int rc;
  if ((rc = ensure(h, h->seg, (size_t)ub * g.T * g.n * 4))) return rc;
  for (int64_t u0 = 0; u0 < B; u0 += ub) {
    const int64_t nb = std::min(ub, B - u0);
    {
      ProfScope ps(h, SG_STAGE_APPLY_ISTFT, st);
      HIPCHK(h, frames(g, u0, nb, mask_dev + (size_t)u0 * g.T * g.FS, (float*)h->seg.p));
    }
    ProfScope ps(h, SG_STAGE_OLA, st);
    HIPCHK(h, spec_backward_ola(g, nb, L, (const float*)h->seg.p, (char*)grad_x_dev + (size_t)u0 * gx_stride * elem_bytes(dtype),
                                dtype, gx_stride, st));
  }
  return SG_OK;
}

// Adjoint of Y = M .* rfft( Wa frames(x) ) with M fixed: g_x = frames^T( Wa Re sum_k M[k] g[k] e^{+2 pi i k j / n} ).
extern "C" int sg_gate_spectrum_backward(sg_handle* h, const void* grad_spec_dev, int dtype, int64_t B, int64_t L,
                                         const float* mask_dev, void* grad_x_dev, int64_t gx_stride, void* stream) {
  if (int rc = t_entry(h, "sg_gate_spectrum_backward")) return rc;
  if (!grad_spec_dev || !grad_x_dev || !mask_dev || B < 1 || (dtype != SG_F32 && dtype != SG_F64))
    FAIL(h, SG_E_INVALID, "sg_gate_spectrum_backward: bad argument");
  if (L < 2 * (int64_t)h->W) FAIL(h, SG_E_INVALID, "x must be bigger than %d", 2 * h->W);
  if (!spectrum_geom_ok(h))
    FAIL(h, SG_E_UNSUPPORTED, "sg_gate_spectrum_backward: n_fft=%d (powers of two from 256 to 4096 only)", h->n);
  hipStream_t st = (hipStream_t)stream;
  return spectrum_backward_loop(h, dtype, B, L, mask_dev, grad_x_dev, gx_stride, st,
                                [&](const Geom& g, int64_t u0, int64_t nb, const float* mask, float* seg) {
    return spec_backward_frames(g, nb, h->tw32.p, (const float*)h->wa32.p, mask,
                                (const char*)grad_spec_dev + (size_t)u0 * g.T * g.F * 2 * elem_bytes(dtype), dtype, seg, st);
  });
}

// TorchGate.gated_filterbank (feat.hpp).  The bank is host data: validated, transposed and given its hull tables here.
extern "C" int sg_set_filterbank(sg_handle* h, const float* fb_host, int32_t n_filters) {
  if (int rc = t_entry(h, "sg_set_filterbank")) return rc;
  if (!fb_host || n_filters < 1 || n_filters > FEAT_MAX_FILTERS)
    FAIL(h, SG_E_INVALID, "sg_set_filterbank: bad argument (1 <= n_filters <= %d)", FEAT_MAX_FILTERS);
  if (!spectrum_geom_ok(h))
    FAIL(h, SG_E_UNSUPPORTED, "sg_set_filterbank: n_fft=%d (powers of two from 256 to 4096 only)", h->n);
  const int F = h->F, M = n_filters;
  std::vector<float> fbT((size_t)F * M);
  std::vector<int32_t> khull(2 * (size_t)M), mhull(2 * (size_t)F);
  if (!feat_tables(fb_host, F, M, fbT.data(), khull.data(), mhull.data()))
    FAIL(h, SG_E_INVALID, "sg_set_filterbank: the filterbank has a non-finite entry");
  // launches of an earlier call may still read the tables about to be overwritten
  if (h->n_filters) HIPCHK(h, hipDeviceSynchronize());
  h->n_filters = 0;
  int rc;
  if ((rc = upload(h, h->fb_d, fb_host, (size_t)F * M * 4))) return rc;
  if ((rc = upload(h, h->fbT_d, fbT.data(), (size_t)F * M * 4))) return rc;
  if ((rc = upload(h, h->fb_khull, khull.data(), khull.size() * 4))) return rc;
  if ((rc = upload(h, h->fb_mhull, mhull.data(), mhull.size() * 4))) return rc;
  h->n_filters = M;
  return SG_OK;
}

extern "C" int sg_gate_features(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                const void* xn_dev, int64_t Bn, int64_t Ln, int64_t xn_stride, int32_t power, int32_t take_log,
                                double eps, void* feat_dev, float* mask_out_dev, void* stream) {
  if (int rc = t_entry(h, "sg_gate_features")) return rc;
  if (!x_dev || !feat_dev || (dtype != SG_F32 && dtype != SG_F64) || B < 1)
    FAIL(h, SG_E_INVALID, "sg_gate_features: bad argument");
  int rc;
  if ((rc = features_args_ok(h, "sg_gate_features", power, eps))) return rc;
  const Sink sink{Sink::FEATURES, nullptr, dtype, 0, nullptr, FeatSink{feat_dev, power, take_log != 0, eps}};
  return process_batch_impl(h, x_dev, dtype, B, L, x_stride, xn_dev, Bn, Ln, xn_stride, sink, mask_out_dev, stream);
}

// Adjoint of sg_gate_features w.r.t. x with mask and bank fixed: the frames are transformed again from x, G = dL/dX formed
// in LDS, windowed adjoint frames into h->seg, then the gather of sg_gate_spectrum_backward.
extern "C" int sg_gate_features_backward(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t x_stride,
                                         const void* grad_feat_dev, const float* mask_dev, int32_t power, int32_t take_log,
                                         double eps, void* grad_x_dev, int64_t gx_stride, void* stream) {
  if (int rc = t_entry(h, "sg_gate_features_backward")) return rc;
  if (!x_dev || !grad_feat_dev || !grad_x_dev || !mask_dev || B < 1 || (dtype != SG_F32 && dtype != SG_F64) || x_stride < L ||
      gx_stride < L)
    FAIL(h, SG_E_INVALID, "sg_gate_features_backward: bad argument");
  if (L < 2 * (int64_t)h->W) FAIL(h, SG_E_INVALID, "x must be bigger than %d", 2 * h->W);
  int rc;
  if ((rc = features_args_ok(h, "sg_gate_features_backward", power, eps))) return rc;
  hipStream_t st = (hipStream_t)stream;
  View v = rows_view(x_dev, dtype, x_stride, L);
  return spectrum_backward_loop(h, dtype, B, L, mask_dev, grad_x_dev, gx_stride, st,
                                [&](const Geom& g, int64_t u0, int64_t nb, const float* mask, float* seg) {
    v.unit0 = u0;
    return feat_backward_frames(v, g, nb, h->tw32.p, (const float*)h->wa32.p, mask, feat_bank(h), power, take_log != 0, eps,
                                (const char*)grad_feat_dev + (size_t)u0 * g.T * h->n_filters * elem_bytes(dtype), dtype, seg,
                                st);
  });
}

// Adjoint of y = D^-1 OLA( Ws irfft( M .* rfft( Wa frames(x) ) ) ) with M fixed:
//   g_x = frames^T( Wa irfft( M .* rfft( Ws frames( D^-1 g_y ) ) ) )
// (irfft(M .* rfft(.)) is self-adjoint for a real mask; Wa and Ws are the same window up to the
// 1/N scale), i.e. the forward kernels run on g_y / env with an un-normalised overlap-add.
extern "C" int sg_process_batch_backward(sg_handle* h, const void* grad_out_dev, int dtype, int64_t B, int64_t L,
                                         int64_t go_stride, const float* mask_dev, void* grad_x_dev,
                                         int64_t gx_stride, void* stream) {
  if (int rc = t_entry(h, "sg_process_batch_backward")) return rc;
  if (!grad_out_dev || !grad_x_dev || !mask_dev || B < 1 || (dtype != SG_F32 && dtype != SG_F64))
    FAIL(h, SG_E_INVALID, "sg_process_batch_backward: bad argument");
  hipStream_t st = (hipStream_t)stream;
  Geom g = make_geom(h, L);
  const int64_t Lq = g.Lout;
  int rc;
  if (h->fast_ok && !h->force_nofast && h->rowgate_mode != 1 && g.F == 513 && g.T >= 1 && g.T <= fast::RG_FRAMES) {
    // rows of at most 64 frames: the whole backward of a row in one workgroup (rowbwd.hpp) -- no grad_out / envelope copy,
    // no tiles, no hand-offs
    h->dbg_bwd_route = SG_BWD_ROW;
    ProfScope ps(h, SG_STAGE_APPLY_FAST, st);
    fast::RowBwdArgs A;
    A.view = rows_view(grad_out_dev, dtype, go_stride, Lq);
    A.g = g;
    A.g.Lout = L;   // the adjoint scatters back onto all L input samples
    A.om = whole_out(grad_x_dev, dtype, gx_stride, L);
    A.win = (const float*)h->wa32.p;
    A.wsq = (const float*)h->wsq32.p;
    A.invn = (const float*)h->invn.p;
    A.tw512 = (const fast::cf*)h->tw512.p;
    A.tw1024 = (const fast::cf*)h->tw32.p;
    A.mask = mask_dev;
    A.kscale = (float)(1.0 / 512.0);
    const size_t lds = fast::rowbwd_lds_bytes();
    HIPCHK(h, launch_lds(fast::k_row_backward, dim3((unsigned)B), dim3(1024), lds, st, A));
    return SG_OK;
  }
  int64_t ub = units_per_batch(h, g, B);
  rc = ensure_ws(h, g, ub);
  if (rc) return rc;
  if ((rc = ensure(h, h->yn, (size_t)ub * Lq * sizeof(float)))) return rc;
  for (int64_t u0 = 0; u0 < B; u0 += ub) {
    const int64_t nb = std::min(ub, B - u0);
    {
      dim3 grid((unsigned)((Lq + 255) / 256), (unsigned)nb);
      const char* src = (const char*)grad_out_dev + (size_t)u0 * go_stride * elem_bytes(dtype);
      hipLaunchKernelGGL(k_env_scale, grid, dim3(256), 0, st, (const void*)src, dtype, go_stride, g,
                         (const float*)h->wsq32.p, (float*)h->yn.p, Lq);
      HIPCHK(h, hipGetLastError());
    }
    const View v = rows_view(h->yn.p, SG_F32, Lq, Lq);
    Geom gb = g;
    gb.Lout = L;  // the adjoint scatters back onto all L input samples
    const OutMap om = whole_out((char*)grad_x_dev + (size_t)u0 * gx_stride * elem_bytes(dtype), dtype, gx_stride, L);
    const float* mk = mask_dev + (size_t)u0 * g.T * g.FS;
    if (h->fast_ok && !h->force_nofast) {
      h->dbg_bwd_route = SG_BWD_FAST;
      if ((rc = stage_apply_fast(h, v, gb, nb, om, mk, 0, st))) return rc;
    } else if (const RegGeom* r = reg_geom(h)) {
      h->dbg_bwd_route = SG_BWD_REG;
      if ((rc = stage_apply_reg(h, r, v, gb, nb, om, mk, 0, st))) return rc;
    } else {
      h->dbg_bwd_route = SG_BWD_OLA;
      if ((rc = stage_apply_ola(h, v, gb, nb, mk, om, 0, st))) return rc;
    }
  }
  return SG_OK;
}

// ------------------------------------------------------------------------------------------
// stage taps
// ------------------------------------------------------------------------------------------
extern "C" int sg_stft(sg_handle* h, const void* x_dev, int dtype, int64_t B, int64_t L, int64_t stride,
                       double* z_dev, void* stream) {
  if (!h) return SG_E_INVALID;
  if (!x_dev || !z_dev || !dtype_ok(dtype) || B < 1 || L < h->W) FAIL(h, SG_E_INVALID, "sg_stft: bad argument");
  Geom g = make_geom(h, L);
  HIPCHK(h, stft_any<double>(h, rows_view(x_dev, dtype, stride, L), g, B, nullptr, nullptr, z_dev, h->mag_scale, (hipStream_t)stream));
  return SG_OK;
}

// ---- what debug.hip's taps need of this unit (handle.hpp) ----
int sg::host::expand_k16_mask(sg_handle* h, size_t cells, hipStream_t st) {
  // same kernel, same arithmetic as the materialising path.
  // (a debug entry point: whatever stream produced the counts has to be done first)
  HIPCHK(h, hipDeviceSynchronize());
  hipLaunchKernelGGL(k_k16_to_mask, dim3(grid_1d((int64_t)cells / 8, 256)), dim3(256), 0, st,
                     (const unsigned short*)h->K16.p, h->last.g, h->p.n_grad_freq, h->p.n_grad_time, 1.0f / (float)h->ktot,
                     (float)h->p.prop_decrease, 1, h->p.smooth_mask ? 1 : 0, (float*)h->M.p, (int64_t)h->last.units);
  HIPCHK(h, hipGetLastError());
  return SG_OK;
}

#if OP_TRACE
static int onepass_dev_counter_impl(sg_handle* h, int which, int64_t* value, void* stream, bool* done) {
  *done = true;
  if (which == 8) {
    // (diagnosis) after a call that lost a hand-off: the tiles of the last first launch that did not run to the end -- who took
    // their ticket (workgroup, iteration) and the last phase each of their four waves stamped -- on stderr; *value = their number
    HIPCHK(h, hipStreamSynchronize((hipStream_t)stream));
    std::vector<unsigned> t(g_trace_tiles * 64);
    HIPCHK(h, hipMemcpy(t.data(), g_trace_dev, t.size() * 4, hipMemcpyDeviceToHost));
    int64_t bad = 0;
    auto last_phase = [&](size_t tk, int w) { int lp = -1; for (int k = 0; k < 14; ++k) if (t[(tk * 4 + w) * 16 + k]) lp = k; return lp; };
    for (size_t tk = 0; tk < g_trace_tiles; ++tk) {
      const int jt = (int)(tk % g_trace_ntt) - 1;
      const bool halo = jt < 0 || jt >= g_trace_ntt - 2;
      bool ok = true;
      for (int w = 0; w < 4; ++w) ok = ok && (halo ? last_phase(tk, w) >= 5 : t[(tk * 4 + w) * 16 + 15] == 1u);
      if (ok) continue;
      if (++bad > 8) continue;
      fprintf(stderr, "[trace] ticket %zu (unit %zu tile %d%s):", tk, tk / g_trace_ntt, jt, halo ? " halo" : "");
      for (int w = 0; w < 4; ++w) {
        const unsigned who = t[(tk * 4 + w) * 16 + 14];
        fprintf(stderr, "  w%d wg %d iter %u last phase %d", w, (int)(who & 0xffffu) - 1, who >> 16, last_phase(tk, w));
      }
      fprintf(stderr, "\n");
    }
    *value = bad;
    return SG_OK;
  }
  *done = false;
  return SG_OK;
}
#endif
bool sg::host::onepass_dev_counter(sg_handle* h, int which, int64_t* value, hipStream_t st, int* rc) {
#if OP_TRACE
  bool done = false;
  *rc = onepass_dev_counter_impl(h, which, value, (void*)st, &done);
  return done;
#else
  (void)h; (void)which; (void)value; (void)st; (void)rc;
  return false;
#endif
}

