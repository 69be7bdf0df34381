// The host arithmetic of a stream bank (stream.hip): plain C++17, no HIP and no StBank, so that a
// stand-alone host program (tests/stream_plan_host.cpp) reaches every line of it.
//   st_counters_at   what a stream has decided, applied and emitted after n samples: THE statement of the counters
//   st_live       ... and which part of its state a later step can still read (the payload of a snapshot)
//   st_layout     the rings' depths and the bytes of every device buffer of a bank
//   st_check_step every check of a step, before any device work
//   st_plan_step  the step's tables (StUnit, StSpec / StFeatUnit, the tiles of the four launches) and the slots afterwards
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mi355gate.h"
#include "tile_tables.hpp"

namespace sg {

// what a spectrum step (sg_stream_push_spectrum) stores on top of a push: spec / mask buffers (mask may be null), the
// element type of both (SG_F32: float2 / float, SG_F64: double2 / double), and the table parallel to the step's records
struct StSpecOut {
  void* spec;
  int dtype;
  void* mask;
  const sg_stream_spec_rec* recs;
};
// what a feature step (sg_stream_push_features) stores on top of a push: feat / mask buffers (mask may be null), the
// element type of both (SG_F32 / SG_F64), the table parallel to the step's records and the switches of the reduction
// (scale == 0: the handle's 1 / sum(window))
struct StFeatOut {
  void* feat;
  int dtype;
  void* mask;
  const sg_stream_feat_rec* recs;
  int32_t power, take_log;
  double eps, scale;
};

// ---- geometry and counters ---------------------------------------------------------------------------------------------
// what the arithmetic needs of a bank -- or of a header alone (sg_stream_head_bytes)
struct StGeo {
  int64_t n, F, FS, W, H, nt, L, RC, wpr, C;   // n_fft, bins, padded bins, window, hop, time half width, lookahead, ring, ...
  bool ns, ad, fixed, exact;
  // a box bank (TorchGate's non-stationary gate: the level is a moving mean over K = Lb + 1 + L frames): a non-stationary
  // bank whose decide step also reads Lb frames BEHIND the one it decides; 0 / false for every other bank
  int64_t Lb;
  bool box;
};
// kind: SG_STREAM_FIXED / _NONSTATIONARY / _ADAPTIVE; the lookahead counts for a non-stationary bank only
inline StGeo st_make_geo(int64_t n_fft, int64_t F, int64_t FS, int64_t W, int64_t H, int64_t nt, int64_t lookahead, int64_t C,
                         int kind, bool exact) {
  StGeo g{};
  g.n = n_fft; g.F = F; g.FS = FS; g.W = W; g.H = H; g.nt = nt; g.C = C;
  g.ns = kind == SG_STREAM_NONSTATIONARY; g.ad = kind == SG_STREAM_ADAPTIVE; g.fixed = kind == SG_STREAM_FIXED;
  g.exact = exact;
  g.L = g.ns ? lookahead : 0;
  g.RC = W + (nt + g.L + 1) * H;
  g.wpr = (F + 63) / 64;
  return g;
}
// the box bank of a moving mean over K frames, frames [t - (K - 1) / 2, t - (K - 1) / 2 + K): look-back Lb = (K - 1) / 2,
// lookahead L = K - 1 - Lb
inline StGeo st_make_geo_box(int64_t n_fft, int64_t F, int64_t FS, int64_t W, int64_t H, int64_t nt, int64_t K, int64_t C,
                             bool exact) {
  const int64_t lo = (K - 1) / 2;
  StGeo g = st_make_geo(n_fft, F, FS, W, H, nt, K - 1 - lo, C, SG_STREAM_NONSTATIONARY, exact);
  g.Lb = lo;
  g.box = true;
  return g;
}
inline StGeo st_geo(const sg_stream_head& hd) {
  const int64_t F = hd.n_fft / 2 + 1;
  return st_make_geo(hd.n_fft, F, (F + 15) / 16 * 16, hd.win_length, hd.hop_length, hd.smooth_mask ? hd.n_grad_time : 0,
                     hd.lookahead_frames, hd.channels, hd.kind, hd.exact != 0);
}

// last frame that lies inside the first n samples (-1: none)
inline int64_t st_tdec(int64_t W, int64_t H, int64_t n) {
  const int64_t a = n + W / 2 - W;
  return a < 0 ? -1 : a / H;
}
// After n samples a stream has decided (transformed) frame td, has raw mask rows up to ts (L frames behind), has applied
// frame ta (nt more behind) and has emitted E samples.  Every other statement of a counter calls this one.
struct StCounters {
  int64_t td, ts, ta, E;
};
inline StCounters st_counters_at(int64_t W, int64_t H, int64_t nt, int64_t L, int64_t n) {
  StCounters v{};
  v.td = st_tdec(W, H, n);
  v.ts = std::max<int64_t>(-1, v.td - L);
  v.ta = std::max<int64_t>(-1, v.ts - nt);
  v.E = std::max<int64_t>(0, (v.ta + 1) * H - W / 2);
  return v;
}
inline StCounters st_counters_at(const StGeo& g, int64_t n) { return st_counters_at(g.W, g.H, g.nt, g.L, n); }
// samples emitted after n received by a stationary stream of the handle's geometry (sg_stream_emitted)
inline int64_t st_emitted(int W, int H, int nt, int64_t n) { return st_counters_at(W, H, nt, 0, n).E; }

// what of a stream that has received n samples a later step can still read (every counter follows from n)
struct StLive {
  int64_t td, ts, ta, E;
  int64_t ring_lo, ring_n;   // samples [ring_lo, n)
  int64_t car_n;             // carry positions [E, E + car_n)
  int64_t row_lo, bit_rows;  // bit rows [row_lo, td] (stationary / adaptive)
  int64_t mk_rows;           // sigmoid rows [row_lo, ts] (non-stationary)
  int64_t fa_rows;           // A / fwd rows (ts, td] (non-stationary); A rows (ts - Lb, td] of a box bank
};
inline StLive st_live(const StGeo& g, int64_t n) {
  const int64_t h = g.W / 2;
  const StCounters k = st_counters_at(g, n);
  StLive v{};
  v.td = k.td; v.ts = k.ts; v.ta = k.ta; v.E = k.E;
  v.ring_lo = std::max<int64_t>(0, n - g.RC);
  v.ring_n = n - v.ring_lo;
  v.car_n = v.ta >= 0 ? std::max<int64_t>(0, v.ta * g.H - h + g.W - v.E) : 0;
  v.row_lo = std::max<int64_t>(0, v.ta + 1 - g.nt);
  v.bit_rows = g.ns ? 0 : v.td - v.row_lo + 1;
  v.mk_rows = g.ns ? v.ts - v.row_lo + 1 : 0;
  v.fa_rows = g.ns ? v.td - std::max<int64_t>(-1, v.ts - g.Lb) : 0;
  return v;
}
// 8-byte words of a float mask row / a double one
inline int64_t mk_words(const StGeo& g) { return g.exact ? g.FS : g.FS / 2; }

// 8-byte words of one slot's snapshot payload after n samples
inline int64_t st_payload_words(const StGeo& g, int64_t n) {
  const StLive v = st_live(g, n);
  int64_t per = v.ring_n + v.car_n;
  if (g.box) per += v.fa_rows * g.FS + v.mk_rows * mk_words(g);   // (no snapshot of a box bank yet: sg_stream_export refuses)
  else if (g.ns) per += g.FS + v.fa_rows * 2 * g.FS + v.mk_rows * mk_words(g);
  else per += g.FS + v.bit_rows * g.wpr;
  if (g.ad) per += 3 * g.FS;
  return (g.fixed ? 2 * g.FS : 0) + g.C * per;
}

// ---- the bank's buffers ------------------------------------------------------------------------------------------------
constexpr int ST_FPT = 2;     // frames per apply tile
constexpr int ST_RPT = 16;    // rows per smoothing tile
constexpr int64_t ST_WS_PREALLOC = (int64_t)256 << 20;

// frames one step can decide or apply for a stream: those of max_block samples plus the zero-extended ones of a flush
inline int64_t st_max_frames(const StGeo& g, int64_t max_block) { return (max_block + g.W / 2) / g.H + 3; }

// Depths of the rings and bytes of every device buffer of a bank; 0: the kind of bank has no such buffer.  RB is the depth
// the arithmetic gives and what state_bytes() reports; a stationary bank indexes with RB_ring, the depth clamped to
// INT32_MAX, and allocates bits_alloc, the bit rows at that depth (st_create refuses a non-stationary bank whose rings are
// deeper than INT32_MAX).
struct StLayout {
  int64_t RC, RB, RF, max_frames, RB_ring;
  // the state that survives between steps (stream.hpp's table), in the order st_create allocates it
  int64_t ring, carry, fst, fa, mk, rmax, bits, nst;
  // not state: a fixed bank's thresholds [slot] and their upload staging, the slot list of sg_stream_set_threshold
  int64_t thr, T2, stage, slot_list;
  // tables and scratch of a typical step, allocated up front (a larger step grows them, which synchronises once)
  int64_t tabs, ws;
  int64_t bits_alloc;
  int64_t state_bytes() const { return ring + carry + fst + fa + mk + rmax + bits + nst; }
};
inline StLayout st_layout(const StGeo& g, int64_t n_slots, int64_t max_block) {
  StLayout y{};
  const int64_t nu = n_slots * g.C, mf = st_max_frames(g, max_block);
  y.max_frames = mf;
  y.RC = g.RC;
  // (a flush decides the L frames a push holds back on top of the block's own: the mask rows are L deeper for it)
  y.RB = 2 * g.nt + 1 + g.L + mf;
  // (the A rows: the L + 1 a decision reads ahead, the Lb it reads behind -- a box bank's alone -- and the step's own)
  y.RF = g.L + g.Lb + 1 + mf;
  y.RB_ring = std::min<int64_t>(INT32_MAX, y.RB);
  y.ring = nu * y.RC * 8;
  y.carry = nu * 2 * g.W * 8;
  if (g.ns) {
    // (a box bank carries no forward pass: no fst, and its fa rows hold A alone)
    y.fst = g.box ? 0 : nu * g.FS * 8;
    y.fa = nu * y.RF * (g.box ? 1 : 2) * g.FS * 8;
    y.mk = nu * y.RB * g.FS * (g.exact ? 8 : 4);
  } else {
    y.rmax = nu * g.FS * 8;
    y.bits = nu * y.RB * g.wpr * 8;
    y.bits_alloc = nu * y.RB_ring * g.wpr * 8;
    if (g.ad) {
      y.nst = nu * 3 * g.FS * 8;
    } else {
      y.thr = y.T2 = n_slots * g.FS * 8;
      y.stage = g.FS * 8;
    }
  }
  y.slot_list = n_slots * 4;
  y.tabs = (int64_t)(align256(nu * sizeof(StUnit)) + align256(nu * 16 * sizeof(Tile)) + align256(nu * sizeof(StSpec)));
  const int64_t per_unit = (int64_t)(align256((size_t)((mf + 2 * g.nt) * g.FS * (g.exact && g.ns ? 8 : 4))) +
                                     align256((size_t)(mf * g.n * (g.exact ? 8 : 4))));
  y.ws = std::min<int64_t>(ST_WS_PREALLOC, nu * per_unit);
  return y;
}

// ---- one step ----------------------------------------------------------------------------------------------------------
// what the bank remembers of a slot: the counters are st_counters_at(n)
struct StSlot {
  int64_t n = 0;
  int par = 0;   // carry buffer the next step reads
  bool has_thr = false;
};

// The counters of a stream before and after a block of n_samples (flush: its last one).  The check and the plan of a step
// both read the frames a record reports (ta1 - v0.ta) here.
struct StAdvance {
  StCounters v0;
  int64_t n1, td1, ts1, ta1, E1;
  int64_t Tend, Lout;   // flush: frames of the whole stream, valid samples of the inverse transform; else "unbounded"
};
inline StAdvance st_advance(const StGeo& g, int64_t n0, int64_t n_samples, bool flush) {
  const int64_t UNBOUNDED = (int64_t)1 << 60, h = g.W / 2;
  StAdvance a{};
  a.v0 = st_counters_at(g, n0);
  a.n1 = n0 + n_samples;
  if (flush) {
    const int64_t T = (a.n1 + 2 * h - g.W) / g.H + 1;
    a.Tend = T;
    // (a box bank has no zero tail: its last N mod H samples are the overlap-add over the window envelope continued)
    a.Lout = g.box ? a.n1 : (T - 1) * g.H + g.W - 2 * h;
    a.td1 = a.ts1 = a.ta1 = T - 1;
    a.E1 = a.n1;
  } else {
    const StCounters v1 = st_counters_at(g, a.n1);
    a.Tend = a.Lout = UNBOUNDED;
    a.td1 = v1.td; a.ts1 = v1.ts; a.ta1 = v1.ta; a.E1 = v1.E;
  }
  return a;
}

inline const char* st_step_name(const StSpecOut* so, const StFeatOut* fo) {
  return fo ? "sg_stream_push_features" : so ? "sg_stream_push_spectrum" : "sg_stream_push";
}

// Every check of a step (sg_stream_push / _push_spectrum / _push_features), before any device work or state change.
// M: filters of the bank's filterbank (0: none set).
inline int st_check_step(const StGeo& g, int64_t max_block, int M, const std::vector<StSlot>& slots, int in_dtype, int out_dtype,
                         const sg_stream_rec* recs, int32_t n_recs, const StSpecOut* so, const StFeatOut* fo, std::string* err) {
  const char* who = st_step_name(so, fo);
  const int n_slots = (int)slots.size();
  char msg[200];
  auto dtype_ok = [&](int d) { return d == SG_F32 || d == SG_F64 || (g.exact && (d == SG_I16 || d == SG_I32)); };
  if (!dtype_ok(in_dtype) || !dtype_ok(out_dtype)) {
    *err = std::string(who) + ": bad argument (float32 / float64 buffers)";
    return SG_E_INVALID;
  }
  if (so && ((so->dtype != SG_F32 && so->dtype != SG_F64) || (n_recs > 0 && (!so->spec || !so->recs)))) {
    *err = std::string(who) + ": bad argument (spec_dev and spec_recs are needed; spec_dtype is SG_F32 or SG_F64)";
    return SG_E_INVALID;
  }
  if (fo) {
    if (so) { *err = std::string(who) + ": bad argument (a step stores the spectrum or the features)"; return SG_E_INVALID; }
    if ((fo->dtype != SG_F32 && fo->dtype != SG_F64) || (n_recs > 0 && (!fo->feat || !fo->recs))) {
      *err = std::string(who) + ": bad argument (feat_dev and feat_recs are needed; feat_dtype is SG_F32 or SG_F64)";
      return SG_E_INVALID;
    }
    if (fo->power != 1 && fo->power != 2) { *err = std::string(who) + ": power must be 1 or 2"; return SG_E_INVALID; }
    if (!(fo->eps == fo->eps)) { *err = std::string(who) + ": eps is NaN"; return SG_E_INVALID; }
    if (!(fo->scale >= 0.0 && fo->scale <= 1.79769313486231570e308)) {
      *err = std::string(who) + ": scale must be finite and not negative (0: the bank's 1 / sum(window))";
      return SG_E_INVALID;
    }
    if (!M) { *err = std::string(who) + ": no filterbank set (sg_stream_set_filterbank)"; return SG_E_INVALID; }
  }
  std::vector<char> seen(n_slots, 0);
  for (int32_t i = 0; i < n_recs; ++i) {
    const sg_stream_rec& r = recs[i];
    if (r.slot < 0 || r.slot >= n_slots) {
      snprintf(msg, sizeof msg, "%s: record %d: unknown slot %d (the bank has %d)", who, i, r.slot, n_slots);
      *err = msg;
      return SG_E_INVALID;
    }
    if (seen[r.slot]) {
      snprintf(msg, sizeof msg, "%s: slot %d appears twice in one step", who, r.slot);
      *err = msg;
      return SG_E_INVALID;
    }
    seen[r.slot] = 1;
    if (r.n_samples < 0 || r.n_samples > max_block) {
      snprintf(msg, sizeof msg, "%s: slot %d: block of %lld samples (max_block is %lld)", who, r.slot,
               (long long)r.n_samples, (long long)max_block);
      *err = msg;
      return SG_E_INVALID;
    }
    if (r.in_offset < 0 || r.out_offset < 0 || (g.C > 1 && (r.in_stride < r.n_samples || r.out_stride < 0))) {
      snprintf(msg, sizeof msg, "%s: slot %d: bad offsets / strides", who, r.slot);
      *err = msg;
      return SG_E_INVALID;
    }
    const StSlot& S = slots[r.slot];
    if (!S.has_thr) {
      snprintf(msg, sizeof msg, "%s: slot %d has no noise threshold yet", who, r.slot);
      *err = msg;
      return SG_E_STATE;
    }
    if (r.flush && S.n + r.n_samples < g.W) {
      snprintf(msg, sizeof msg, "%s: slot %d: a stream of %lld samples is shorter than win_length=%d", who, r.slot,
               (long long)(S.n + r.n_samples), (int)g.W);
      *err = msg;
      return SG_E_INVALID;
    }
    if (so || fo) {
      // (the frames the record reports: those the plan applies)
      const StAdvance a = st_advance(g, S.n, r.n_samples, r.flush != 0);
      const int64_t frames = a.ta1 - a.v0.ta;
      if (so) {
        const sg_stream_spec_rec& q = so->recs[i];
        if (q.spec_offset < 0 || (so->mask && q.mask_offset < 0) || (g.C > 1 && q.stride < frames * g.F)) {
          snprintf(msg, sizeof msg, "%s: slot %d: bad spectrum offsets / stride", who, r.slot);
          *err = msg;
          return SG_E_INVALID;
        }
      } else {
        const sg_stream_feat_rec& q = fo->recs[i];
        if (q.feat_offset < 0 || (fo->mask && q.mask_offset < 0) ||
            (g.C > 1 && (q.feat_stride < frames * M || (fo->mask && q.mask_stride < frames * g.F)))) {
          snprintf(msg, sizeof msg, "%s: slot %d: bad feature offsets / strides", who, r.slot);
          *err = msg;
          return SG_E_INVALID;
        }
      }
    }
  }
  return SG_OK;
}

// The tables of a checked step.  Stage s of the four launches reads tiles [t_s, t_s + n_s) of tl.
struct StStep {
  std::vector<StUnit> units;        // [record][channel]
  std::vector<StSpec> specs;        // parallel to units in a spectrum step, else empty
  std::vector<StFeatUnit> feats;    // parallel to units in a feature step, else empty
  TileList tl;
  int64_t t_dec, n_dec, t_fs, n_fs, t_ap, n_ap, t_fin, n_fin;
  int64_t mrows, sframes;           // rows of the smoothed-row / segment scratch
  std::vector<StSlot> after;        // [record]: the slot's state once the step is enqueued
};
inline StStep st_plan_step(const StGeo& g, const std::vector<StSlot>& slots, const sg_stream_rec* recs, int32_t n_recs,
                           const StSpecOut* so, const StFeatOut* fo) {
  const int64_t h = g.W / 2;
  StStep P{};
  P.after.resize(n_recs);
  for (int32_t i = 0; i < n_recs; ++i) {
    const sg_stream_rec& r = recs[i];
    const StSlot& S = slots[r.slot];
    const StAdvance a = st_advance(g, S.n, r.n_samples, r.flush != 0);
    StUnit U{};
    U.n0 = S.n; U.n1 = a.n1;
    U.td0 = a.v0.td; U.td1 = a.td1;
    U.ts0 = a.v0.ts; U.ts1 = a.ts1;
    U.ta0 = a.v0.ta; U.ta1 = a.ta1;
    U.E0 = a.v0.E; U.E1 = a.E1;
    U.Tend = a.Tend; U.Lout = a.Lout;
    U.flush = r.flush ? 1 : 0;
    U.cov0 = U.ta0 >= 0 ? U.ta0 * g.H - h + g.W : 0;
    if (U.ta1 > U.ta0) {
      U.r0 = std::max<int64_t>(0, U.ta0 + 1 - g.nt);
      U.r1 = std::min<int64_t>(U.Tend, U.ta1 + g.nt + 1);
    }
    U.slot = r.slot;
    U.par = S.par;
    for (int ch = 0; ch < g.C; ++ch) {
      StUnit V = U;
      V.state = r.slot * (int32_t)g.C + ch;
      V.in_off = r.in_offset + (int64_t)ch * r.in_stride;
      V.out_off = r.out_offset + (int64_t)ch * r.out_stride;
      V.mrow = P.mrows; P.mrows += V.r1 - V.r0;
      V.srow = P.sframes; P.sframes += V.ta1 - V.ta0;
      P.units.push_back(V);
      if (so) P.specs.push_back(StSpec{so->recs[i].spec_offset + ch * so->recs[i].stride, so->recs[i].mask_offset + ch * so->recs[i].stride});
      if (fo) P.feats.push_back(StFeatUnit{fo->recs[i].feat_offset + ch * fo->recs[i].feat_stride, fo->recs[i].mask_offset + ch * fo->recs[i].mask_stride});
    }
    StSlot& N = P.after[i];   // (a flushed slot is empty: n = 0, par = 0)
    N.has_thr = true;
    if (!r.flush) {
      N.n = U.n1;
      N.par = U.ta1 > U.ta0 ? (S.par ^ 1) : S.par;
    }
  }
  const std::vector<StUnit>& units = P.units;
  TileList& tl = P.tl;
  P.t_dec = tl.begin_stage();
  for (size_t u = 0; u < units.size(); ++u)
    if (units[u].td1 > units[u].td0 || units[u].ts1 > units[u].ts0) tl.push(u, units[u].td0 + 1, units[u].td1 + 1);
  P.n_dec = tl.count_since(P.t_dec);
  P.t_fs = tl.begin_stage();
  for (size_t u = 0; u < units.size(); ++u) tl.push_ranges(u, units[u].r0, units[u].r1, ST_RPT);
  P.n_fs = tl.count_since(P.t_fs);
  P.t_ap = tl.begin_stage();
  for (size_t u = 0; u < units.size(); ++u) tl.push_ranges(u, units[u].ta0 + 1, units[u].ta1 + 1, ST_FPT);
  P.n_ap = tl.count_since(P.t_ap);
  P.t_fin = tl.begin_stage();
  for (size_t u = 0; u < units.size(); ++u) {
    const StUnit& U = units[u];
    // newly final samples [E0, E1) and the open ones up to the last applied frame's end (a flush closes every sample,
    // also when its last frame was applied before)
    if (U.ta1 > U.ta0 || U.flush)
      tl.push_ranges(u, U.E0, U.flush ? U.E1 : std::max(U.E1, U.ta1 * g.H - h + g.W), 256, true, ST_OLA);
    if (!U.flush) tl.push_ranges(u, std::max(U.n0, U.n1 - g.RC), U.n1, 256, true, ST_APPEND);
    else if (!g.ns) tl.push(u, 0, 0, ST_CLEAR);
  }
  P.n_fin = tl.count_since(P.t_fin);
  return P;
}

}  // namespace sg
