// Which route a gate call takes (api.hip: run_S and its callees, process_batch_impl), decided once per call from plain
// numbers: RouteCaps is what routing reads of a handle (api.hip: route_caps copies it), RouteShape what it reads of the call,
// plan_S / plan_T state every branch the stages take, workspace_S what the planned route allocates.  Host arithmetic only --
// no HIP, no handle -- so tests/route_plan_host.cpp walks the whole table without a GPU.  The conditions of the former
// predicates of api.hip (onepass_ok, onepass_geom_ok, onepass_reg_ok, exact_fused_ok, nonstat2_chain_ok, nonstat2_ok,
// box_mask_ok, bits_path_ok, rowgate_ok, k16_apply_geom, RG_MIN_ROWS) are written here and nowhere else.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/mi355gate.h"

namespace sg {
namespace host {

// geometry constants of a one-pass gate: tiles of NF frames every NH frames
struct OnePassGeom {
  int hop, NF, NH, tile_words, xw, max_nf, max_nt, F;
  size_t lds;      // dynamic LDS (n_fft = 1024: + OP_PROP_LDS when prop_decrease != 1)
  int extra = 0;   // 3 when the tiles abut (NH == NF, abutting_tiles), 0 when they overlap by 3 frames
  int64_t tiles(int64_t nh) const { return (nh + extra + NH - 1) / NH; }
};

}  // namespace host
namespace route {

// Limits of the kernels a route leads to (api.hip asserts each against the header that owns it)
constexpr int NS_TT = 64, NS_MAX_NF = 24, NS_IIR_MAX_NT = 20, NS_BOX_MAX_NT = 12, NS_BOX_KB = 20;
constexpr bool ns_iir_nt_ok(int nt) { return (nt >= 1 && nt <= NS_IIR_MAX_NT) || nt == 25 || nt == 34 || nt == 37; }
constexpr int RG_FRAMES = 64, RG_NFMAX = 30, RG_NTMAX = 16;
// The row gate runs one workgroup per row and one workgroup per CU at a time: a call of fewer rows than ~2/3 of the CUs is
// faster on the four-kernel path, which spreads a row over 5 workgroups (256 x 16000: 0.110 vs 0.146 ms; 128 rows: ~0.105
// vs 0.097; 1024 rows: 0.45 vs 0.52; profiles/r04_rowgate_scale.json).
constexpr int64_t RG_MIN_ROWS = 160;
constexpr int XIIR_TT = 32;   // exact.hpp: tile of the float64 recurrence (exact_unit_bytes)

// How the handle's frame length is transformed.  DEFAULT: n_fft = win = 1024, hop 256 (register transform, fused kernels);
// REG: n_fft = win = 512 / 256 / 2048, hop n_fft / 4 (RegGeom); POW2: another power of two up to 8192 (LDS transform);
// MIXED: 2 N with N a product of 2, 3, 5, 7, 11, 13 (mixed.hpp); CZT: chirp-z; LONG: four-step through HBM (big.hpp).
enum class GeomClass { DEFAULT, REG, POW2, MIXED, CZT, LONG };

struct RouteCaps {
  // gate parameters
  int variant = SG_VARIANT_S;
  bool stationary = true, smooth_mask = true;
  double prop_decrease = 1.0, iir_b = 0.0;
  int nf = 0, nt = 0, n_movemean = 0;   // n_grad_freq, n_grad_time
  int64_t ktot = 1;
  bool fused_ok = false, t_sm2_ok = true;
  // geometry
  GeomClass geom = GeomClass::POW2;
  const host::OnePassGeom *op = nullptr, *op_seam = nullptr;   // DEFAULT: both the 1024 gate's; REG: overlapping / abutting tiles
  bool reg_abut = false;    // REG: the one-pass gate needs abutting tiles (2048)
  int reg_frames = 0;       // REG: frames per abutting apply tile (DEFAULT: 16)
  // resources
  bool ftab3 = false, optab = false, regtab = false, norm64 = false;
  // options
  bool force_unfused = false, force_nofast = false, force_f64_decide = false, force_noseam = false, force_nolean = false,
       force_split = false, fast_integer = false, force_exact = false, exact_materialised = false;
  int rowgate_mode = 0, tile_order = 0;
  int64_t ws_budget = (int64_t)8 << 30;
};

struct RouteShape {
  int F = 0, FS = 0, n = 0;
  int64_t T = 0;
  int64_t nh = 0;             // hops of the geometry's one-pass / apply tiles that hold the output map's samples
  int in_dtype = SG_F32, out_dtype = SG_F32;
  int64_t units = 1;          // units of the call (variant T: rows)
  bool field = false;         // variant T: the sink wants the mask as a float field (spectrum, features)
  int64_t noise_rows = 0;     // variant T: rows of xn (0: none given)
};

enum class Pipe { EXACT_FUSED, EXACT, ONEPASS, ONEPASS_REG, BITS3, FUSED, UNFUSED };
enum class Decide { NONE, FAST, REG, LDS, F64 };           // the decide kernel inside stage_fused_mask
enum class NsMask { NONE, SMOOTHED, CHAIN, RAW, BOX };     // non-stationary mask: two-pass + smoothing, chain only, raw; T: box mask
enum class Apply { NONE, FAST64_K, FAST64_M, X_OLA, FAST_K, FAST_M, REG_K, REG_M, OLA_K, OLA_M, FIELD };
enum class Range { KEEP, ALL, WINDOW, TILES };             // sg_debug_range: as the last route with bits left it, [0, T), what the stage decided
enum class Thresh { NONE, SHARED, PER_ROW, SELF };         // variant T: the shared noise row's, each row's own noise, the rows themselves

// What the debug taps report of a batch of this route (handle.hpp: LastBatch)
struct BatchFacts {
  bool keeps = true;   // false: the route keeps no fields (sg_debug_dims reports 0 units)
  bool has_P = false, has_raw = false, fused = false, fast = false, k16_only = false, rg = false;
  Range range = Range::KEEP;
};

struct SPlan {
  Pipe pipe = Pipe::UNFUSED;
  Decide decide = Decide::NONE;
  NsMask ns = NsMask::NONE;
  bool smooth_stage = false;   // UNFUSED: stage_smooth follows the mask stage
  bool k16_to_mask = false;    // FUSED: the K counts are expanded into the float mask field
  Apply apply = Apply::NONE;   // (the one-pass gates apply themselves)
  bool seam = false;           // ONEPASS_REG: abutting tiles + k_ola_seam
  bool exact_tiled = false;    // EXACT: the tile-parallel recurrence and the LDS-tiled smoothing may be taken
  bool lean = false;           // the workspace holds bit / count fields only
  bool f32_copy = false;       // a float32 copy of a recording of another sample type is made first
  bool fast = false, reg = false;   // the geometry's fused (1024) / register (512, 256, 2048) kernels are in use
  BatchFacts facts;
};

struct TPlan {
  bool rowgate = false, bits_path = false, to_raw = false, row_fused = false;
  Thresh thresh = Thresh::NONE;
  NsMask ns = NsMask::NONE;
  bool smooths = false;
  Apply apply = Apply::NONE;
  bool fast = false, reg = false;
  BatchFacts facts;
};

namespace detail {
inline bool geom_fast(const RouteCaps& c) { return c.geom == GeomClass::DEFAULT && !c.force_nofast; }
inline bool geom_reg(const RouteCaps& c) { return c.geom == GeomClass::REG && !c.force_nofast; }
inline bool fused(const RouteCaps& c) { return c.fused_ok && !c.force_unfused; }
// the general apply kernel that can read the K counts of the fused bit-mask stages directly
inline bool k16_apply_geom(const RouteCaps& c) { return c.geom != GeomClass::LONG && c.geom != GeomClass::CZT; }
inline bool int_out(const RouteShape& s) { return s.out_dtype == SG_I16 || s.out_dtype == SG_I32; }

// One-pass stationary gate, default geometry: at least two abutting tiles (seam mode)
inline bool onepass_ok(const RouteCaps& c, const RouteShape& s) {
  if (!fused(c) || !geom_fast(c) || !c.op) return false;
  if (c.force_split || c.force_f64_decide || c.force_noseam || c.force_nolean) return false;
  if (!c.smooth_mask || c.nf > c.op->max_nf || c.nt > c.op->max_nt || !c.ftab3 || !c.optab) return false;
  return s.F == c.op->F && c.op->tiles(s.nh) >= 2;
}
// ... of a register geometry
inline bool onepass_reg_ok(const RouteCaps& c, const RouteShape& s) {
  if (!geom_reg(c) || !c.op || (c.reg_abut && c.force_noseam)) return false;
  if (c.force_split || c.force_f64_decide || !fused(c)) return false;
  if (c.variant != SG_VARIANT_S || !c.stationary || !c.smooth_mask) return false;
  if (c.nf > c.op->max_nf || c.nt > c.op->max_nt || s.F != c.op->F || !c.regtab) return false;
  return c.tile_order != 1 && s.nh > 0;
}
// The stationary gate in float64 without materialised float64 fields (default geometry, full reduction)
inline bool exact_fused_ok(const RouteCaps& c, const RouteShape& s) {
  return c.stationary && fused(c) && geom_fast(c) && !c.force_f64_decide && s.F == 513 && c.norm64 && !c.exact_materialised;
}
// Variant-S non-stationary mask in two passes over |X| (nonstat.hpp).  chain: the recurrence can run tile-parallel;
// smoothed: ... and k_iir_mask also smooths (nt instantiated, nf <= NS_MAX_NF), the mask in one kernel.  The backward
// sweep regenerates the forward values in reverse: error growth c^-rows must stay small.
inline bool nonstat2_chain_ok(const RouteCaps& c, const RouteShape& s) {
  if (c.variant != SG_VARIANT_S || c.stationary || c.force_unfused) return false;
  if (!(c.iir_b > 0.0 && c.iir_b < 1.0)) return false;
  return std::pow(1.0 - c.iir_b, (double)(NS_TT + 2 * NS_IIR_MAX_NT)) >= 1e-3 && s.T >= 1;
}
inline bool nonstat2_ok(const RouteCaps& c, const RouteShape& s) {
  if (!nonstat2_chain_ok(c, s) || !c.smooth_mask) return false;
  if (c.nt > NS_IIR_MAX_NT && !(std::pow(1.0 - c.iir_b, (double)(NS_TT + 2 * c.nt)) >= 1e-3)) return false;
  return c.nf <= NS_MAX_NF && ns_iir_nt_ok(c.nt);
}
// Variant-T non-stationary mask in one kernel (k_box_mask): the default moving-mean length, k_iir_mask's widths
inline bool box_mask_ok(const RouteCaps& c) {
  if (c.variant != SG_VARIANT_T || c.stationary || c.force_unfused || c.n_movemean != NS_BOX_KB) return false;
  if (!c.smooth_mask) return true;
  return c.nf <= NS_MAX_NF && c.nt >= 1 && c.nt <= NS_BOX_MAX_NT;
}
// Variant T, default geometry, full reduction: decisions as bits -> integer smoothing -> uint16 sums for the fused apply
inline bool bits_path_ok(const RouteCaps& c) {
  return geom_fast(c) && !c.force_unfused && c.prop_decrease == 1.0 && c.ktot <= 65535 &&
         (!c.smooth_mask || (c.nt <= 96 && c.t_sm2_ok));
}
// TorchGate.forward of whole rows in one kernel (rowgate.hpp): rows of at most 64 frames, statistics from the row itself
inline bool rowgate_ok(const RouteCaps& c, const RouteShape& s) {
  if (c.rowgate_mode == 1 || (c.rowgate_mode == 0 && s.units < RG_MIN_ROWS)) return false;
  return geom_fast(c) && !c.force_unfused && c.stationary && c.prop_decrease == 1.0 && c.smooth_mask && c.ktot <= 65535 &&
         s.F == 513 && s.T >= 1 && s.T <= RG_FRAMES && c.nf >= 1 && c.nf <= RG_NFMAX && c.nt >= 1 && c.nt <= RG_NTMAX;
}
}  // namespace detail

// Variant S (run_S): the route of every batch of the call
inline SPlan plan_S(const RouteCaps& c, const RouteShape& s) {
  using namespace detail;
  SPlan p;
  p.fast = geom_fast(c);
  p.reg = geom_reg(c);
  const bool fu = fused(c), full = c.prop_decrease == 1.0;
  // integer outputs are the TRUNCATED float64 result of the reference (base.py:217-226): float64 pipeline
  if (c.force_exact || (int_out(s) && !c.fast_integer)) {
    if (exact_fused_ok(c, s)) {
      p.pipe = Pipe::EXACT_FUSED; p.decide = Decide::FAST; p.apply = Apply::FAST64_K; p.lean = true;
      p.facts.fused = p.facts.fast = true; p.facts.range = Range::WINDOW;
    } else {
      p.pipe = Pipe::EXACT; p.exact_tiled = !c.exact_materialised;
      p.apply = (p.fast && s.F == 513 && c.norm64 && !c.exact_materialised) ? Apply::FAST64_M : Apply::X_OLA;
      p.facts.keeps = false;
    }
    return p;
  }
  const bool ns_ok = nonstat2_ok(c, s), ns_chain = nonstat2_chain_ok(c, s);
  const bool onepass = onepass_ok(c, s), onepass_r = onepass_reg_ok(c, s);
  // one-pass gate (any prop_decrease) or, with prop_decrease == 1, the three-kernel bit-mask path: bit / count fields only
  p.lean = onepass || onepass_r || (fu && p.fast && full);
  // the register-FFT kernels would take the checked per-sample path for every frame of a recording that is not float32
  p.f32_copy = s.in_dtype != SG_F32 && ((p.fast && (onepass || (!c.stationary && ns_ok))) || onepass_r);
  if (onepass || onepass_r) {
    p.pipe = onepass ? Pipe::ONEPASS : Pipe::ONEPASS_REG;
    p.seam = onepass || c.reg_abut || !c.force_noseam;
    p.facts.fused = p.facts.fast = true; p.facts.range = Range::TILES;
    return p;
  }
  if (fu && p.fast && full) {
    p.pipe = Pipe::BITS3; p.decide = c.force_f64_decide ? Decide::F64 : Decide::FAST; p.apply = Apply::FAST_K;
    p.facts.fused = p.facts.fast = true; p.facts.range = c.force_f64_decide ? Range::ALL : Range::WINDOW;
    return p;
  }
  if (fu) {
    p.pipe = Pipe::FUSED;
    p.decide = c.force_f64_decide ? Decide::F64 : (p.reg ? Decide::REG : Decide::LDS);
    const bool k16_only = !p.reg && k16_apply_geom(c) && full;   // k_apply_istft reads the K counts itself
    p.k16_to_mask = !(p.reg && full) && !k16_only;
    p.apply = p.fast ? Apply::FAST_M : (p.reg ? (full ? Apply::REG_K : Apply::REG_M) : (k16_only ? Apply::OLA_K : Apply::OLA_M));
    p.facts.fused = true; p.facts.has_raw = true; p.facts.k16_only = k16_only; p.facts.range = Range::ALL;
    p.facts.fast = p.fast || (p.reg && full);
    return p;
  }
  p.pipe = Pipe::UNFUSED;
  if (!c.stationary) p.ns = ns_ok ? NsMask::SMOOTHED : (ns_chain ? NsMask::CHAIN : NsMask::RAW);
  p.smooth_stage = c.stationary || !(ns_ok || (ns_chain && !c.smooth_mask));
  p.apply = p.fast ? Apply::FAST_M : (p.reg ? Apply::REG_M : Apply::OLA_M);
  p.facts.has_P = c.stationary; p.facts.fast = p.fast;
  p.facts.has_raw = c.stationary || !ns_chain || (!ns_ok && c.smooth_mask);
  return p;
}

// Variant T (process_batch_impl): sg_process_batch, sg_gate_spectrum, sg_gate_features
inline TPlan plan_T(const RouteCaps& c, const RouteShape& s) {
  using namespace detail;
  TPlan p;
  p.fast = geom_fast(c);
  p.reg = geom_reg(c);
  const bool box = box_mask_ok(c);
  p.smooths = c.stationary || !box;   // (the box mask comes smoothed out of its one kernel)
  p.apply = s.field ? Apply::FIELD : (p.fast ? Apply::FAST_M : (p.reg ? Apply::REG_M : Apply::OLA_M));
  p.facts.has_P = c.stationary; p.facts.fast = p.fast; p.facts.has_raw = p.smooths;
  if (!c.stationary) {
    p.ns = box ? NsMask::BOX : NsMask::RAW;
    return p;
  }
  if (!s.field && s.noise_rows == 0 && rowgate_ok(c, s)) {
    p.rowgate = true; p.smooths = false; p.apply = Apply::NONE;
    p.facts = BatchFacts{true, false, false, true, true, false, true, Range::ALL};
    return p;
  }
  p.thresh = s.noise_rows == 1 ? Thresh::SHARED : (s.noise_rows > 0 ? Thresh::PER_ROW : Thresh::SELF);
  p.bits_path = bits_path_ok(c);
  p.to_raw = s.field;
  // short rows: statistics + constants + decisions of a (row, 64 bands) tile in one kernel
  p.row_fused = p.bits_path && (size_t)s.T * 64 * sizeof(double) <= 64 * 1024;
  if (p.bits_path && !s.field) {   // the bits straight through the integer smoothing into the fused apply kernel
    p.smooths = false; p.apply = Apply::FAST_K;
    p.facts = BatchFacts{true, true, false, true, true, false, false, Range::ALL};
  }
  return p;
}

// ------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------
// Per unit.  lean: the bit mask (T*wpr*8 B) and the uint16 weight sums (T*FS*2 B) only.
constexpr size_t unit_bytes(const RouteShape& s, bool lean) {
  const size_t cells = (size_t)s.T * s.FS;
  if (lean) return (size_t)s.T * ((s.F + 63) / 64) * 8 + cells * 2 + (size_t)s.FS * 16 + 64 + (size_t)(s.T / 16 + 2) * 6 * 256 * 4;
  return cells * (8 + 4 + 4 + 2) + (size_t)s.T * s.n * 4 + (size_t)s.FS * 16 +
         (size_t)(s.T / NS_TT + 1) * 2 * s.FS * 8 * 2 +  // + partials and carries of the two-pass non-stationary mask
         (size_t)(s.T / 8 + 1) * 2 * s.FS * 8;           // + the magnitude kernels' per-tile partials (tiles of 8 frames at n_fft = 2048)
}
// float64 pipeline (exact.hpp): P, raw, M, tmp (8 B per cell each) + frames (8 B per sample of every frame) + the statistics
// rows + the non-stationary gate's tile partials and carries (2 x 2 doubles per band and 32-frame tile, one tile more than T / 32)
inline size_t exact_unit_bytes(const RouteShape& s) {
  return (size_t)s.T * s.FS * 32 + (size_t)s.T * s.n * 8 + (size_t)s.FS * 16 + (size_t)(s.T / XIIR_TT + 2) * s.FS * 32;
}
inline int64_t units_per_batch(int64_t budget, size_t unit, int64_t total) {
  return std::min(std::max<int64_t>(1, std::min<int64_t>(budget / (int64_t)unit, 32768)), total);
}

struct Workspace {
  int64_t ub = 0;         // units per batch
  int64_t unit = 0;       // bytes per unit of the route's fields
  int64_t exchange = 0;   // bytes of the route's exchange buffers for ub units: tile bits, partial hops, seam partials, counters
  int64_t total() const { return ub * unit + exchange; }
};
// What a call of `units` units on the planned route allocates (the float32 copy and the long frames' work buffers aside)
inline Workspace workspace_S(const RouteCaps& c, const SPlan& p, const RouteShape& s, int64_t units) {
  Workspace w;
  const bool exact = p.pipe == Pipe::EXACT;
  w.unit = (int64_t)(exact ? exact_unit_bytes(s) : unit_bytes(s, p.lean));
  w.ub = units_per_batch(c.ws_budget, (size_t)w.unit, units);
  const int hop = c.op ? c.op->hop : 0, frames = c.geom == GeomClass::DEFAULT ? 16 : c.reg_frames;
  const int64_t abut = frames ? (s.nh + 3 + frames - 1) / frames : 0;
  if (p.pipe == Pipe::ONEPASS || p.pipe == Pipe::ONEPASS_REG) {
    const host::OnePassGeom& S = p.seam ? *c.op_seam : *c.op;
    const int64_t tiles = S.tiles(s.nh);
    w.exchange += w.ub * (tiles + 2) * S.tile_words * 8;                  // tile bits (two halo tiles more)
    if (p.pipe == Pipe::ONEPASS) w.exchange += w.ub * tiles * 3 * 256 * 8 + 64;   // partial hops, tickets
    else if (p.seam) w.exchange += w.ub * abut * 6 * hop * 4;             // seam partials
  } else if (p.apply == Apply::FAST_K || p.apply == Apply::FAST_M) {
    if (abut >= 2 && !c.force_noseam) w.exchange += w.ub * abut * 3 * 256 * 8 + w.ub * 64 + 64;   // partial hops (in-launch or seam), tickets
  } else if (p.apply == Apply::REG_K || p.apply == Apply::REG_M) {
    if (abut >= 2 && !c.force_noseam) w.exchange += w.ub * abut * 6 * hop * 4;
  }
  return w;
}

}  // namespace route
}  // namespace sg
