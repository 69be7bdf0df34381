// The launch plan of the n_fft = 1024 one-pass gate (k_gate_onepass): everything about a tile's coordinates that does not
// depend on the tile, worked out once on the host (stage_onepass) and read by the kernel as one 128-byte block.
//
// A ticket names (unit, tile): u = ticket / ntt, jt = ticket % ntt - 1; the unit names (row, chunk).  The kernel used to
// derive both with 32-bit division expansions and to walk the clause chains of `blk_vec` (the tile's span is five aligned
// 16-byte loads per thread) and `tile_fast` (the straight-line epilogue) field by field, at every place that needs a tile's
// coordinates.  Nearly all of that is the same for every tile of a launch:
//   * the quotients become a multiply-high and shifts (round-up method: exact for EVERY 32-bit dividend);
//   * a unit is INTERIOR when the readable range of its row (lo / hi) and the kept range of the output (g_lo / g_hi) cannot
//     bind for any of its tiles -- every chunk of a row but the first and the last readable ones -- and when the
//     launch-invariant halves of both flags hold (float32 in and out, normalised, 16-byte aligned bases and strides);
//   * for an interior unit `blk_vec` and `tile_fast` are functions of jt alone: closed ranges [bv0, bv1] and [tf0, tf1];
//   * source and output pointers are a folded base + row * stride + chunk * step + jt * 4096.
// A unit that is not interior, and a tile outside the ranges, takes the kernel's field-by-field evaluation unchanged.
//
// Host and device run the SAME functions (tests/test_onepass_plan_host.py builds them into a stand-alone program and holds
// them to divisions and the clause chains restated in Python).  No HIP header is needed to read this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OP_PLAN_HD __host__ __device__ __forceinline__
#else
#define OP_PLAN_HD inline
#endif

namespace sg {
namespace fast {

constexpr int OP_PLAN_NF = 16;                               // frames (= hops) per tile
constexpr int OP_PLAN_HOP = 256;
constexpr int OP_PLAN_SPAN = (OP_PLAN_NF - 1) * 256 + 1024;  // samples a tile stages
constexpr int OP_PLAN_TILE = OP_PLAN_NF * OP_PLAN_HOP;       // samples a tile advances by
constexpr int OP_PLAN_SCAN_MAX = 5 * 256;                    // longest floor-test slice that rides in registers

// n / d for every 32-bit n: t = mulhi(m, n); q = (t + ((n - t) >> s1)) >> s2 (Granlund & Montgomery, round-up multiplier)
struct OpMagic {
  uint32_t m, s;   // s = s1 | s2 << 8
};
inline OpMagic op_magic(uint32_t d) {
  uint32_t l = 0;
  while (l < 32 && ((uint64_t)1 << l) < d) ++l;   // ceil(log2 d)
  OpMagic g;
  g.m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / d + 1);
  g.s = (l < 1 ? l : 1u) | ((l > 0 ? l - 1 : 0u) << 8);
  return g;
}
OP_PLAN_HD uint32_t op_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
OP_PLAN_HD uint32_t op_magic_div(uint32_t n, uint32_t m, uint32_t s) {
  const uint32_t t = op_mulhi(m, n);
  return (t + ((n - t) >> (s & 31u))) >> (s >> 8);
}

// The launch as plain numbers (stage_onepass fills it from View, Geom, OutMap and the hop range)
struct OpPlanIn {
  uint64_t x, out;                   // addresses of the source and output buffers
  int32_t in_dtype, out_dtype, normalize;
  int64_t stride, lo, hi, cs, pad, Lp, c0, unit0;
  int32_t n_chunks;
  int64_t ostride, p0, p1, g_step, g0, g_lo, g_hi;
  int32_t padL;
  int64_t T, Lout, h_begin, h_end;
  int32_t n_tiles, scan_q;
};

struct alignas(64) OpPlan {
  // ---- first 64 bytes: quotients, ranges, source ----
  uint32_t m_ntt, s_ntt, ntt;        // ticket / ntt
  uint32_t m_nch, s_nch, nch;        // (unit0 + u) / n_chunks
  uint32_t unit0;
  uint32_t k0, k1;                   // interior units: chunk - c0 in [k0, k1] (empty: 1, 0)
  int32_t bv0, bv1;                  // ... whose tile jt is blk_vec: jt in [bv0, bv1]
  int32_t tf0, tf1;                  // ... and tile_fast: jt in [tf0, tf1]
  int32_t s0b0;                      // first staged sample of tile 0, unit-local: (h_begin - 3) * 256 - padL
  uint64_t src;                      // address of that sample in row 0, chunk 0
  // ---- second 64 bytes: strides, output, floor-test slices ----
  int64_t sstride, cs;               // source: + row * sstride + chunk * cs + jt * 4096 (samples)
  uint64_t dst;                      // address of tile 0's first output sample in row 0, chunk 0
  int64_t dstride, g_step;           // output: + row * dstride + chunk * g_step + jt * 4096
  int64_t c0;
  int32_t scan_q, sc_lenA, sc_total, sc_last;   // floor-test slices of an interior unit (see tile_src in the kernel)
};
static_assert(sizeof(OpPlan) == 128, "two 64-byte scalar loads");

// A ticket against the plan
struct OpTile {
  uint32_t u;        // unit of the launch
  int32_t jt;        // tile of the unit, -1 and n_tiles: halo tiles
  uint32_t row, k;   // row; chunk - c0
  bool interior;
};
OP_PLAN_HD OpTile op_plan_tile(const OpPlan& P, uint32_t ticket) {
  OpTile t;
  t.u = op_magic_div(ticket, P.m_ntt, P.s_ntt);
  t.jt = (int32_t)(ticket - t.u * P.ntt) - 1;
  const uint32_t gu = P.unit0 + t.u;
  t.row = op_magic_div(gu, P.m_nch, P.s_nch);
  t.k = gu - t.row * P.nch;
  t.interior = (t.k - P.k0) <= (P.k1 - P.k0) && P.k0 <= P.k1;
  return t;
}
OP_PLAN_HD bool op_plan_blk_vec(const OpPlan& P, const OpTile& t) {
  return t.interior & ((uint32_t)(t.jt - P.bv0) <= (uint32_t)(P.bv1 - P.bv0)) & (P.bv0 <= P.bv1);
}
OP_PLAN_HD bool op_plan_tile_fast(const OpPlan& P, const OpTile& t) {
  return t.interior & ((uint32_t)(t.jt - P.tf0) <= (uint32_t)(P.tf1 - P.tf0)) & (P.tf0 <= P.tf1);
}
// sample offsets from P.src / P.dst (valid where the flag holds)
OP_PLAN_HD int64_t op_plan_src_off(const OpPlan& P, const OpTile& t) {
  return (int64_t)t.row * P.sstride + (P.c0 + t.k) * P.cs + (int64_t)t.jt * OP_PLAN_TILE;
}
OP_PLAN_HD int64_t op_plan_dst_off(const OpPlan& P, const OpTile& t) {
  return (int64_t)t.row * P.dstride + (P.c0 + t.k) * P.g_step + (int64_t)t.jt * OP_PLAN_TILE;
}
// granule offsets: published bits (64-bit words) and trailing partial hops
OP_PLAN_HD uint64_t op_plan_xbits_off(const OpPlan& P, const OpTile& t, uint32_t tile_words) {
  return ((uint64_t)t.u * P.ntt + (uint32_t)(t.jt + 1)) * tile_words;
}
OP_PLAN_HD int64_t op_plan_part2_off(const OpPlan& P, const OpTile& t) {
  return ((int64_t)t.u * (P.ntt - 2u) + t.jt) * 3 * 256;
}
// the floor-test slice of an interior unit's tile: [c0, c1) of A ++ B, and where it starts relative to P.src when it rides
// in registers (has == true)
struct OpScan {
  int64_t c0, c1, off;
  bool has;
};
OP_PLAN_HD OpScan op_plan_scan(const OpPlan& P, const OpTile& t) {
  OpScan s;
  s.c0 = (int64_t)(t.jt + 1) * P.scan_q;
  const int64_t e = s.c0 + P.scan_q;
  s.c1 = e < P.sc_total ? e : (int64_t)P.sc_total;
  s.has = s.c1 > s.c0 && s.c1 - s.c0 <= OP_PLAN_SCAN_MAX && (s.c1 <= P.sc_lenA || s.c0 >= P.sc_lenA);
  s.off = (int64_t)t.row * P.sstride + (P.c0 + t.k) * P.cs - P.s0b0 + (s.c1 <= P.sc_lenA ? s.c0 : P.sc_last + (s.c0 - P.sc_lenA));
  return s;
}

// ---- host: the plan of a launch ----
inline OpPlan op_plan_build(const OpPlanIn& I) {
  OpPlan P{};
  // (a launch has at least one chunk and no negative tile count: a divisor of 0 has no multiplier.  Such arguments get divisors
  // of 1 and no interior unit)
  const bool sane = I.n_chunks >= 1 && I.n_tiles >= 0;
  const OpMagic a = op_magic(sane ? (uint32_t)(I.n_tiles + 2) : 1u), b = op_magic(sane ? (uint32_t)I.n_chunks : 1u);
  P.m_ntt = a.m; P.s_ntt = a.s; P.ntt = sane ? (uint32_t)(I.n_tiles + 2) : 1u;
  P.m_nch = b.m; P.s_nch = b.s; P.nch = sane ? (uint32_t)I.n_chunks : 1u;
  P.unit0 = (uint32_t)I.unit0;
  P.k0 = 1; P.k1 = 0; P.bv0 = 1; P.bv1 = 0; P.tf0 = 1; P.tf1 = 0;
  P.c0 = I.c0;
  P.sstride = I.stride; P.cs = I.cs; P.dstride = I.ostride; P.g_step = I.g_step;
  P.scan_q = I.scan_q;
  const int64_t tf00 = I.h_begin - 3, s0b0 = tf00 * 256 - I.padL;   // tile 0's first frame and first staged sample
  // what must fit the plan's 32-bit fields; a launch outside them has no interior unit (the kernel's own evaluation serves it)
  if (I.Lp <= 0 || I.Lp >= (1ll << 30) || s0b0 <= -(1ll << 30) || s0b0 >= (1ll << 30) || I.n_tiles < 1 || !sane) return P;
  P.s0b0 = (int32_t)s0b0;
  P.src = I.x + (uint64_t)((s0b0 - I.pad) * 4);
  P.dst = I.out + (uint64_t)((s0b0 - I.p0 - I.g0) * 4);
  // launch-invariant halves: sample types, normalisation, and alignment of every term of both addresses
  const bool inv = I.in_dtype == 0 && I.out_dtype == 0 && I.normalize != 0 && (P.src & 15) == 0 && (P.dst & 15) == 0 &&
                   (I.stride & 3) == 0 && (I.cs & 3) == 0 && (I.ostride & 3) == 0 && (I.g_step & 3) == 0 && I.cs >= 0 &&
                   I.g_step >= 0;
  if (!inv) return P;
  // the clauses that depend on jt alone: each side monotone in jt, so the tiles that pass form one closed range
  int bv0 = 1, bv1 = 0, tf0 = 1, tf1 = 0;
  for (int jt = -1; jt <= I.n_tiles; ++jt) {
    const int64_t tf = tf00 + (int64_t)jt * OP_PLAN_NF, s0b = tf * 256 - I.padL;
    const bool bv = tf >= 0 && tf + OP_PLAN_NF <= I.T && s0b >= 0 && s0b + OP_PLAN_SPAN <= I.Lp;
    const bool fast = tf >= 3 && tf + OP_PLAN_NF + 2 < I.T && tf >= I.h_begin && tf + OP_PLAN_NF + 2 < I.h_end && s0b >= I.p0 &&
                      s0b + OP_PLAN_TILE <= I.p1 && s0b + OP_PLAN_TILE <= I.Lout;
    if (bv) { if (bv0 > bv1) bv0 = jt; bv1 = jt; }
    if (fast) { if (tf0 > tf1) tf0 = jt; tf1 = jt; }
  }
  if (bv0 > bv1) return P;
  const bool has_tf = tf0 <= tf1;   // (units of two tiles have no tile_fast tile: the flag is false for every tile, as the clauses say)
  // interior units: the row's readable range and the output's kept range bind for none of those tiles, nor for the
  // floor test's window.  Each clause is monotone in the chunk index: the chunks that pass form one closed range.
  auto chunk_ok = [&](int64_t chunk) -> bool {
    const int64_t g0c = chunk * I.cs - I.pad, o0 = chunk * I.g_step - I.p0;
    return g0c >= I.lo && I.hi - g0c >= I.Lp &&
           g0c + s0b0 + (int64_t)bv0 * OP_PLAN_TILE >= I.lo && g0c + s0b0 + (int64_t)bv1 * OP_PLAN_TILE + OP_PLAN_SPAN <= I.hi &&
           (!has_tf || (o0 + s0b0 + (int64_t)tf0 * OP_PLAN_TILE >= I.g_lo && o0 + s0b0 + (int64_t)(tf1 + 1) * OP_PLAN_TILE <= I.g_hi));
  };
  int64_t k0 = 0, k1 = (int64_t)I.n_chunks - 1;
  while (k0 <= k1 && !chunk_ok(I.c0 + k0)) ++k0;
  while (k1 >= k0 && !chunk_ok(I.c0 + k1)) --k1;
  if (k0 > k1) return P;
  // the floor test's window of an interior unit: A = [0, first span), B = [last span's end, Lp)
  const int64_t sp0 = (tf00 - OP_PLAN_NF) * 256 - I.padL, sp1 = (tf00 + (int64_t)I.n_tiles * OP_PLAN_NF) * 256 - I.padL + OP_PLAN_SPAN;
  const int64_t first = sp0 < 0 ? 0 : (sp0 > I.Lp ? I.Lp : sp0), last = sp1 < 0 ? 0 : (sp1 > I.Lp ? I.Lp : sp1);
  P.sc_lenA = (int32_t)first;
  P.sc_last = (int32_t)last;
  P.sc_total = (int32_t)(first + (I.Lp - last));
  P.k0 = (uint32_t)k0; P.k1 = (uint32_t)k1; P.bv0 = bv0; P.bv1 = bv1; P.tf0 = tf0; P.tf1 = tf1;
  return P;
}

// ---- host: the tickets of the one-launch floor fix-up (k_floor_fix, onepass.hpp) ----
// Tickets [0, n_max) are the frame blocks of the float64 band maxima, unit-major (ticket = unit * blocks + block), tickets
// [n_max, n_max + tiles) the REDO tiles in the first launch's order; one workgroup per ticket.  ok == false: the counts do not
// fit 32 bits (the caller keeps the two launches).
constexpr int OP_PLAN_FIX_FRAMES = 16;   // frames per maxima block (k_stft_bits<512, 4, 4>: 4 waves x 4 frames)
struct FloorFixPlan {
  uint32_t blocks;   // maxima blocks per unit: ceil(T / 16)
  uint32_t n_max;    // units * blocks: the first tile ticket
  uint32_t grid;     // n_max + tiles
  bool ok;
};
inline FloorFixPlan floor_fix_plan(int64_t units, int64_t T, int64_t tiles /* units * (n_tiles + 2) */) {
  FloorFixPlan p{};
  if (units < 1 || T < 1 || tiles < 1) return p;
  const int64_t blocks = (T + OP_PLAN_FIX_FRAMES - 1) / OP_PLAN_FIX_FRAMES;
  if (blocks > 0x7fffffff / units || tiles > 0x7fffffff - units * blocks) return p;
  p.blocks = (uint32_t)blocks;
  p.n_max = (uint32_t)(units * blocks);
  p.grid = (uint32_t)(units * blocks + tiles);
  p.ok = true;
  return p;
}

}  // namespace fast
}  // namespace sg
