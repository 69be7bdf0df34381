// The handle behind the C ABI of include/mi355gate.h and what the host units that see it share: api.hip (the gate
// engine), create.hip, debug.hip and shims.hip.  Holds no kernels and includes no header that defines one.  The
// table-driven units (ragged.hip, rows.hip, stream.hip, ...) do not include it: they see an RgCtx (ragged.hpp) only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mi355gate_debug.h"
#include "devbuf.hpp"
#include "feat.hpp"
#include "geom.hpp"
#include "mixed.hpp"
#include "ragged.hpp"
#include "route.hpp"
#include "rows.hpp"
#include "spec.hpp"

namespace sg {
namespace fast {
struct RegArgs;
struct OnePassRegArgs;
struct SeamArgs;
}  // namespace fast
namespace host {

inline std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

// (OnePassGeom, the geometry constants of a one-pass gate: route.hpp)
struct RegGeom {
  int n_fft, hop;
  int frames;                 // frames per decide / magnitude tile and per abutting apply tile
  int hops;                   // complete hops per overlapping apply tile (frames - 3)
  size_t lds;                 // dynamic LDS of the decide / magnitude / apply kernels
  DevBuf sg_handle::*tw;      // twiddle table (RegArgs::tw): tw512, or tw32 at n_fft = 2048
  OnePassGeom op, op_seam;    // one-pass gate on overlapping tiles (SG_OPT_FORCE_NOSEAM) / abutting tiles + k_ola_seam
  bool abut;                  // the one-pass gate needs abutting tiles (2048: op_seam only)
  int tab_kb;                 // k-blocks of time weights in the gate's MFMA table (sg_create; 2048 lays its table out apart)
  void (*decide[2])(fast::RegArgs);        // <4, false>, <4, true>: REDO (the units whose floor test fired)
  void (*mag)(fast::RegArgs);
  void (*apply[2])(fast::RegArgs);         // <4, false>: float mask, <4, true>: uint16 weight sums in K
  void (*gate[2])(fast::OnePassRegArgs);   // <4, false>, <4, true>: REDO
  void (*seam)(fast::SeamArgs);            // k_ola_seam<hop, frames>
};
// (defined next to the kernels they point to: api.hip)
extern const RegGeom REG512, REG256, REG2048;

// What only a stage knows of the batch it ran: the frames whose mask bits it decided and, for a one-pass gate, how its tiles
// lie in the exchange buffer xbits -- tiles of `rows` frames every `step` frames, `words` granule halves each, `xw` words per
// row, tile 0 starting at frame f0, ntt tiles per unit incl. the two halo tiles
struct TileLayout {
  int rows = 16, step = 16, words = 0, xw = 9, ntt = 0;
  int64_t f0 = 0;
};
struct Decided {
  int64_t db = 0, de = 0;
  TileLayout tiles;
};
// What the last batch left in the workspace: the state behind sg_debug_fetch, sg_debug_dims and sg_debug_range (debug.hip).
// Written by note_batch (api.hip) and nowhere else, from the plan's BatchFacts (route.hpp) and the stage's Decided.
struct LastBatch {
  int64_t units = 0, T = 0;
  bool has_P = false;
  bool has_raw = true;    // the unsmoothed mask field exists (not when k_iir_mask / k_box_mask produced the mask in one kernel)
  bool fused = false, fast = false;
  bool k16_only = false;  // a fused general-geometry batch that left K counts only (no float mask field): g is its geometry
  bool rg = false;        // the batch ran on the row gate
  bool xbits = false;     // the mask bits live in xbits, tile-blocked as `tiles` says
  int64_t db = 0, de = 0; // frames whose mask bits were decided
  TileLayout tiles;
  sg::Geom g{};
};

}  // namespace host
}  // namespace sg

struct sg_handle {
  using DevBuf = sg::host::DevBuf;
  using RegGeom = sg::host::RegGeom;
  using MrPlan = sg::MrPlan;
  using Geom = sg::Geom;
  sg_params p{};
  int n = 0, N = 0, W = 0, H = 0, F = 0, FS = 0, padL = 0;
  double sum_w = 0.0;   // sum of the analysis window (scipy 'spectrum' scaling)
  double mag_scale = 1; // |Z| = sqrt(P) * mag_scale  (S: 1/sum_w, T: 1)
  // device tables
  DevBuf tw64, tw32, wfull64, wa32, ws32, wsq32, kf, kt;
  // per-band threshold (S stationary): double[FS]
  DevBuf thresh;
  bool has_thresh = false;
  // workspace
  DevBuf P, pmax, thr_rows, raw, M, seg, yn;
  DevBuf bits, K16, umax, need, T2;  // fused stationary path
  DevBuf nss;                        // non-stationary gate: recurrence partials of k_mag_fast's 16-frame blocks
  DevBuf alim;                       // one-pass gate, in-kernel floor test: [1] tag of the last call that reported, [2..11) bounds on max|x| (k_colstats1_final / k_prep_thresh_lazy)
  bool t2_ready = false;             // T2 / alim hold the compare constants of the CURRENT threshold (any writer of thresh clears it)
  DevBuf logtab;                     // db_fast (kernels.hpp): {rd(1 / c_i), -log2 of it} for 128 mantissa centres
  DevBuf part;                       // partial reductions of the column statistics
  DevBuf tw512, invn;                // fast path tables (n_fft = 1024, hop = 256; 512 / 256 / 2048, hop = n_fft / 4): invn = 1 / window envelope per hop phase
  DevBuf seam;                       // partial seam hops of abutting apply tiles
  DevBuf ftab;                       // k_smooth_bits2 phase-1 lookup tables (nf <= 5)
  int sm2_tt = 64;                   // k_smooth_bits2 tile height (frames)
  bool t_sm2_ok = true;              // variant T: the smoothing filter's tile of k_smooth_bits2 fits the LDS (sg_process_batch's bit-mask route)
  // one-pass gate (onepass.hpp): published mask bits per tile, publication flags, work counter, tables
  DevBuf xbits, xpart, xticket, xtick2, ftab3, xexp, optab;
  DevBuf xin;                        // float32 copy of a recording held in another sample dtype
  DevBuf nsp, nsc;                   // non-stationary mask: per-sub-tile partials / carries (nonstat.hpp)  // ftab3: per-lane MFMA operands, xexp: bit -> byte table
  unsigned* err_host = nullptr;      // host-mapped error word written by k_gate_onepass when a hand-off times out
  unsigned* err_dev = nullptr;
  unsigned inject_fault = 0;         // SG_OPT_INJECT_HANDOFF_FAULT (tests): error bits the next hand-off launch reports
  unsigned lose_now = 0;             // bits 3..6 of the option, consumed by the next hand-off launch: the kernel itself treats
                                     // the hand-off as lost (bounded-poll timeout path: error word + NaN-poisoned hops)
  unsigned ticket_base = 0;          // tickets handed out by all previous launches
  unsigned epoch = 0;                // launch counter: the value a tile's flag must carry to be current
  bool fast_integer = false;         // SG_OPT_FAST_INTEGER: integer outputs from the float32 kernels (<= 1 LSB off)
  bool force_exact = false;          // SG_OPT_FORCE_EXACT: float64 pipeline (exact.hpp) whatever the output dtype
  bool exact_materialised = false;   // SG_OPT_EXACT_MATERIALISED: the float64 pipeline always through exact.hpp's materialised fields
  DevBuf norm64;                     // sum_q win^2[256 q + s] as doubles (default geometry: k_apply_fast64's window envelope)
  unsigned need_era = 0;             // epoch >> 30 of the last one-pass gate call (tagged floor-test flags, stage_onepass)
  DevBuf xP, xraw, xM, xtmp, xseg;   // fields of the exact path
  bool force_split = false;          // SG_OPT_FORCE_SPLIT: decide / smooth / apply as three kernels
  int rowgate_mode = 0;              // SG_OPT_FORCE_NOROWGATE: 0 = by batch size, 1 = never, 2 = whenever the shape is eligible
  int64_t n_floor_lazy = 0, n_floor_apriori = 0;   // sg_debug_counter 1 / 2
  int64_t smooth_route = 0;   // sg_debug_counter 17: SG_SMOOTH_* of the last smoothing launch | cell bytes << 8 | tile frames << 16
  DevBuf fb_d, fbT_d, fb_khull, fb_mhull;   // sg_set_filterbank: the bank [F][M], its transpose and the two hull tables (feat.hpp)
  int n_filters = 0;                        // 0: no bank set
  bool stats_three = false;   // SG_OPT_STATS_THREE_LAUNCH: the noise statistics always as k_stft<double> + k_colstats1 + k_colstats1_final
  int64_t stats_route = 0;    // sg_debug_counter 19: SG_STATS_* form of the last stage_stats call of fewer than 16 units
  bool floor_two = false;     // SG_OPT_FLOOR_TWO_LAUNCH: a lazy one-pass call's floor fix-up always as k_stft_bits<max> + the REDO launch
  int64_t floor_route = 0;    // sg_debug_counter 20: SG_FLOOR_* form of the last one-pass gate call's floor fix-up (0: a-priori floor test)
  DevBuf farrive;             // k_floor_fix: per-unit arrival words {count, epoch} of the maxima workgroups
  int64_t spec_route = 0;     // sg_debug_counter 18: SG_SPEC_* decide branch of the last sg_gate_spectrum call | flags | sub-batches << 16
  int tile_order = 0;                // SG_OPT_TILE_ORDER: 0 (default) = persistent workgroups looping over tickets (onepass.hpp PERSIST),
                                     // 1 = tile = block index (no ticket), 2 = one ticket-drawn tile per workgroup
  int n_cu = 0;                      // compute units of the handle's device (persistent grids)
  int floor_test = 0;                // SG_OPT_FLOOR_TEST: one-pass gate's floor test 0 = predicted, 1 = a priori, 2 = in the gate kernel
  int rg_shape = 16;                 // SG_OPT_ROWGATE_SHAPE: waves per workgroup of the row gate (16 x 1 quad, or 8 x 2 quads)
  bool rg_tap = false;               // SG_OPT_ROWGATE_TAP: keep the row gate's float32 power tile (stage tap 4)
  int dbg_bwd_route = 0;             // sg_debug_backward_route: SG_BWD_* of the last backward call (0: none yet)
  DevBuf rg_count;                   // k_row_gate: number of (row, band) pairs that took the exact path (one counter, never reset)
  int big_M = 0;                     // > 0: long frames (n_fft > 8192, or > 4096 and not a power of two): four-step
                                     // transform of size M through HBM (big.hpp); big_czt: chirp-z on top of it
  int big_czt = 0;
  DevBuf big_twM, big_tw2, big_ch, big_bh, big_W, big_W2;
  int czt_M = 0;                     // > 0: n_fft is not a power of two -> chirp-z kernels (czt.hpp) of size M
  bool mr_ok = false;                // n_fft even, n_fft / 2 <= 2048 with prime factors <= 13, not a power of two: the float32 and
  MrPlan mr{};                       // float64 STFT / decision / apply kernels of mixed.hpp (run-time radix schedule) instead of chirp-z
  DevBuf mr_pt32, mr_pt64;           // the plan's per-pass twiddle tables (mr_pass_tables)
  DevBuf regtab;                     // k_gate_onepass512 / 256 / 2048: MFMA operands + byte expansion (onepass512.hpp, onepass256.hpp, onepass2048.hpp)
  DevBuf czt_tw64, czt_ch64, czt_bh64, czt_tw32, czt_ch32, czt_bh32;
  bool force_noseam = false;
  bool force_nolean = false;         // SG_OPT_FORCE_NOLEAN: full-size slices + stored frames (2 waves/SIMD)
  bool fast_ok = false;              // default geometry: fused apply kernel available
  const RegGeom* reg = nullptr;      // n_fft = win = 512 / 256 / 2048, hop = n_fft / 4: register-transform kernels (reg_geom)
  bool force_nofast = false;
  bool force_f64_decide = false;     // SG_OPT_FORCE_F64_DECIDE: float64 STFT for every mask decision
  int64_t ktot = 1;                  // (nf+1)^2 (nt+1)^2: integer weight total of the smoothing filter
  bool fused_ok = false;
  double sum_abs_w = 0.0;
  sg::host::LastBatch last;    // sg_debug_fetch / sg_debug_dims / sg_debug_range: what the last batch left (note_batch)
  bool force_unfused = false;  // sg_set_option(SG_OPT_FORCE_UNFUSED): materialised v1 path
  // per-kernel timing with HIP events on the launch stream (sg_profile_*)
  bool roctx_on = false;       // SG_ROCTX=1: a roctx range around every stage's enqueue
  bool prof_on = false;
  uint64_t prof_mask = ~0ull;  // stages that get an event pair (sg_profile_select)
  int prof_override = -1;  // >= 0: book every launch under this stage (noise statistics)
  struct ProfRec { int stage; hipEvent_t a, b; };
  std::vector<ProfRec> prof_live;
  std::vector<hipEvent_t> prof_pool;
  double prof_ms[SG_N_STAGES_ALL] = {0};
  int64_t prof_cnt[SG_N_STAGES_ALL] = {0};
  sg::RgState* rg = nullptr;        // ragged batches (sg_process_clips, ragged.hip): workspace and threshold tap
  sg::RwState* rw = nullptr;        // padded batches of different-length rows (sg_process_rows, rows.hip): workspace
  std::string err;
};

#define HIPCHK(h, call)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (h)->err = sg::host::fmt("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      (void)hipGetLastError(); /* reported here: not once more by the next launch check of any handle */ \
      return SG_E_HIP;                                                                       \
    }                                                                                        \
  } while (0)

#define FAIL(h, code, ...)                \
  do {                                    \
    (h)->err = sg::host::fmt(__VA_ARGS__); \
    return (code);                        \
  } while (0)

namespace sg {
namespace host {

// (create.hip)
int ensure(sg_handle* h, DevBuf& b, size_t bytes);
// ensure() + zero fill when the buffer was (re)allocated: for state that kernels keep clean themselves
int ensure_zeroed(sg_handle* h, DevBuf& b, size_t bytes, hipStream_t st, bool* fresh = nullptr);
int upload(sg_handle* h, DevBuf& b, const void* src, size_t bytes);

// RAII: records an event pair around one kernel launch when profiling is enabled, and a roctx range around its enqueue
// under SG_ROCTX=1 (create.hip)
struct ProfScope {
  sg_handle* h;
  hipStream_t st;
  int idx = -1;
  bool ranged = false;
  ProfScope(sg_handle* h_, int stage, hipStream_t st_);
  ~ProfScope();
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;
};
// the same pair as the hooks an RgCtx passes on to the table-driven units
void* rg_prof_begin(void* ctx, int stage, hipStream_t st);
void rg_prof_end(void* tok);

// (api.hip: they run kernels of its headers, or read what its stages left)
int handoff_verdict(sg_handle* h);
// sg_debug_fetch field 1 after a fused batch that left K counts only: expands them into the float mask field M
int expand_k16_mask(sg_handle* h, size_t cells, hipStream_t st);
// sg_debug_counter 8 of the OP_TRACE development build (api.hip, next to stage_onepass); false: not such a build, nothing done
bool onepass_dev_counter(sg_handle* h, int which, int64_t* value, hipStream_t st, int* rc);

inline int64_t frames_for(const sg_handle* h, int64_t L) {
  // S: zero extension W//2 per side, padded=False (scipy/_spectral_py.py:2052,2185-2189).
  // T: torch.stft(center=True) pads n_fft//2 per side: 1 + (L + 2 (n//2) - n) // hop
  //    (= 1 + L // hop for even n_fft).
  if (h->p.variant == SG_VARIANT_S) return (L + 2 * (int64_t)(h->W / 2) - h->W) / h->H + 1;
  return 1 + (L + 2 * (int64_t)(h->n / 2) - h->n) / h->H;
}
inline int64_t outlen_for(const sg_handle* h, int64_t L) {
  int64_t T = frames_for(h, L);
  if (h->p.variant == SG_VARIANT_S) return (T - 1) * h->H + h->W - 2 * (int64_t)(h->W / 2);
  // torch.istft(center=True) trims n_fft//2 from both ends of the n_fft + (T-1) hop buffer
  return (T - 1) * (int64_t)h->H + (h->n - 2 * (int64_t)(h->n / 2));
}

inline Geom make_geom(const sg_handle* h, int64_t Lp) {
  Geom g;
  g.n = h->n; g.W = h->W; g.H = h->H; g.F = h->F; g.FS = h->FS; g.padL = h->padL;
  g.T = frames_for(h, Lp);
  g.Lout = outlen_for(h, Lp);
  return g;
}

inline bool dtype_ok(int d) { return d >= SG_F32 && d <= SG_I32; }

// Bytes of one float32 / float64 element (the dtypes of the variant-T outputs and gradients).
inline size_t elem_bytes(int dtype) { return dtype == SG_F64 ? 8 : 4; }
// The head of every variant-T entry point: a handle, and one of variant T.
inline int t_entry(sg_handle* h, const char* who) {
  if (!h) return SG_E_INVALID;
  if (h->p.variant != SG_VARIANT_T) FAIL(h, SG_E_INVALID, "%s is a variant-T entry point", who);
  return SG_OK;
}

// The reference's minimum lengths of x and xn, and the rows of xn (torchgate.py:215-220).
inline int t_min_lengths(sg_handle* h, int64_t B, int64_t L, const void* xn_dev, int64_t Bn, int64_t Ln) {
  if (L < 2 * (int64_t)h->W) FAIL(h, SG_E_INVALID, "x must be bigger than %d", 2 * h->W);
  if (xn_dev) {
    if (Ln < 2 * (int64_t)h->W) FAIL(h, SG_E_INVALID, "xn must be bigger than %d", 2 * h->W);
    if (Bn != 1 && Bn != B) FAIL(h, SG_E_INVALID, "xn rows (%lld) must be 1 or the batch size", (long long)Bn);
  }
  return SG_OK;
}

inline FeatBank feat_bank(const sg_handle* h) {
  return {(const float*)h->fb_d.p, (const float*)h->fbT_d.p, (const int2*)h->fb_khull.p, (const int2*)h->fb_mhull.p, h->n_filters};
}

inline bool spectrum_geom_ok(const sg_handle* h) { return spec_native(h->n) && !h->czt_M && !h->big_M && !h->mr_ok; }

inline int features_args_ok(sg_handle* h, const char* who, int power, double eps) {
  if (power != 1 && power != 2) FAIL(h, SG_E_INVALID, "%s: power must be 1 or 2", who);
  if (!(eps == eps)) FAIL(h, SG_E_INVALID, "%s: eps is NaN", who);
  if (!spectrum_geom_ok(h)) FAIL(h, SG_E_UNSUPPORTED, "%s: n_fft=%d (powers of two from 256 to 4096 only)", who, h->n);
  if (!h->n_filters) FAIL(h, SG_E_INVALID, "%s: no filterbank set (sg_set_filterbank)", who);
  return SG_OK;
}

inline sg::RgCtx rg_ctx(sg_handle* h) {
  sg::RgCtx c{};
  c.n = h->n; c.N = h->N; c.W = h->W; c.H = h->H; c.F = h->F; c.FS = h->FS; c.padL = h->padL;
  c.mag_scale = h->mag_scale; c.tw64 = h->tw64.p; c.wfull64 = (const double*)h->wfull64.p;
  c.stationary = h->p.stationary; c.cs = h->p.chunk_size; c.pad = h->p.padding;
  c.nf = h->p.smooth_mask ? h->p.n_grad_freq : 0;
  c.nt = h->p.smooth_mask ? h->p.n_grad_time : 0;
  c.prop = h->p.prop_decrease; c.top_db = h->p.top_db; c.n_std = h->p.n_std_thresh; c.iir_b = h->p.iir_b;
  c.nthresh = h->p.nonstat_thresh; c.slope = h->p.nonstat_slope; c.ddof = h->p.ddof;
  c.hook_ctx = h; c.prof_begin = rg_prof_begin; c.prof_end = rg_prof_end;
  return c;
}

}  // namespace host
}  // namespace sg
