// One-pass stationary gate for the default geometry (n_fft = win = 1024, hop = 256, float32 transforms):
// every frame's forward transform is computed ONCE.
//
//   k_decide_fast + k_smooth_bits2 + k_apply_fast          (3 transforms per frame, K round trip in HBM)
//     ->  k_gate_onepass                                    (2 transforms per frame, no mask field in HBM)
//
// A workgroup owns one TILE of 16 consecutive frames of one unit (4 wavefronts x 4 frames, the register
// FFT of fastpath.hpp).  After the forward transform it decides its 16 x 513 cells (float32 + exact
// float64 refinement, bit-identical to k_decide_fast), and keeps the spectra IN REGISTERS while
//   1. the mask bits of the tile (16 x 9 words = 1152 B) are PUBLISHED to the neighbouring tiles through
//      a tile-blocked exchange buffer in HBM (write-through stores, drained, then an epoch-valued flag);
//   2. it waits for the flags of tiles j-1 and j+1 and reads their nt adjacent rows (nt <= 16: the time
//      half-width of the smoothing filter, base.py:115) -- 2*nt*72 B;
//   3. the (16 + 2 nt) x 513 bit tile is smoothed in LDS with the exact integer separable triangle
//      filter (the arithmetic of k_smooth_bits2: table lookups along f, weighted sums along t) into the
//      uint16 weight sums K of its own 16 frames;
// then x mask -> inverse transform -> window -> overlap-add -> store exactly as k_apply_fast<LEAN>.
// The smoothing buffers live in the exchange slices, which are idle between the two transforms: the
// kernel needs no more LDS than k_apply_fast plus its own small tables (3 workgroups per CU).
//
// Inter-workgroup protocol (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup
// visibility"): payload and flag are 8/4-byte agent-scope relaxed atomics on both sides (sc1 stores and
// loads: write-through, L1-bypassing -- per-XCD L2s are not coherent), the payload stores are drained
// (s_waitcnt vmcnt(0) + workgroup barrier) before the flag is stored; every tile's payload is 1152 B =
// 9 x 128 B, 128-byte aligned: no cache line is shared between producers.
// Deadlock freedom does not rely on dispatch order: a workgroup takes a TICKET (atomic counter) when it
// starts and works on tile number `ticket`; it publishes before it waits for anything, so the only
// workgroup that can wait for a tile nobody has started yet is the one with the highest ticket, and
// every other resident workgroup finishes and frees its slot.
#pragma once
#include "fastpath.hpp"
#include "fused.hpp"   // stft_bits_block (k_floor_fix)
#include "limits.hpp"
#include "onepass_plan.hpp"

namespace sg {
namespace fast {

// Build-time switches of this kernel (tools/README.md lists every switch of csrc/ with what builds with it)
#ifndef OP_TRACE
#define OP_TRACE 0   // (development) 1: per-phase shader-clock stamps, see OP_STAMP below
#endif
#ifndef OP_NO_LOOPTOP_WAIT
#define OP_NO_LOOPTOP_WAIT 0   // (diagnosis) 1: without the explicit LDS wait before the persistent loop's top barrier (the state that lost hand-offs)
#endif
// between two tries of a bounded poll: 64 cycles
__device__ __forceinline__ void op_poll_sleep() { __builtin_amdgcn_s_sleep(1); }
struct OnePassArgs {
  ApplyArgs A;              // view, geometry, output map, tables, seam buffer (A.K / A.Mf unused)
  // the caller's samples in their own dtype (A.view may be a float32 copy): exact refinement.  Only these three fields
  // differ from A.view (96 bytes of kernel arguments fewer than a second View)
  const void* x_exact;
  int64_t stride_exact;
  int dtype_exact;
  const char* tab;          // the constant tables (OP_TAB_*): float32 window, window^2, 1/envelope, w_512^(k1 c), w_1024^j,
                            // float64 window and w_1024^j (exact refinement), MFMA operands, byte -> 8 bytes expansion
  ThreshConsts tc;
  double mag_scale, top_db;
  unsigned long long* xbits;  // [units][n_tiles + 2][16][OP_XW][2] published mask bits: granules {32 bits, epoch}
  unsigned* ticket;           // work counter: never reset, a launch takes exactly units * (n_tiles + 2) tickets
  unsigned ticket_base;       // its value before this launch
  unsigned epoch;
  unsigned* err;              // host-mapped word: bit 0 / 1 = a bit / partial-hop hand-off timed out
  int nf, nt;
  float prop, inv_ktot;       // PROP instantiation: prop_decrease and 1 / ktot (A.kscale = 1/512 then)
  unsigned long long* part2;  // [units][n_tiles][3][256] trailing partial hops of every tile: granules {float, epoch}
  // In-kernel floor test (see "floor test" in the kernel): alim = bit pattern of the largest max|x| for which no band's
  // -top_db floor can be live (alim[2 .. 2 + OP_ALIM_BLOCKS), see fastpath.hpp), null when the flags in tc.need_floor were computed up front
  // (k_unit_absmax + k_prep_thresh).  The REDO instantiation is the second launch of such a call: only the units whose
  // test fired run.
  // alim[1]: tc.need_tag of the last call in which some unit reported: the second launch returns at once -- before tables
  // and ticket -- when it is another call's (7152 workgroups that only took their ticket and left cost 83 us:
  // tools/ubench/ticket_atomic.hip)
  unsigned* alim;
  int scan_q;                 // in-kernel floor test: samples of the unit window's unstaged part that each tile scans
  unsigned total_tiles;       // units * (n_tiles + 2): PERSIST workgroups draw tickets until they get one >= this
  OpPlan plan;                // what a tile's coordinates need that does not depend on the tile (onepass_plan.hpp; stage_onepass fills it)
#if OP_TRACE
  unsigned* trace;                   // [workgroups][4 waves][16] shader cycles per phase (slot 15 = 1: tile completed): development builds
#endif
};

// LATE ARGUMENTS.  Whatever the kernel needs of its arguments after the entry block it reads again from the kernel-argument
// segment, where it needs it: scalar loads through an OPAQUE pointer (the compiler cannot merge them with the entry block's
// loads or hoist them above the place where the pointer is made), instead of values that stay live in scalar registers
// across the phases in between.  op_late_ptr() makes such a pointer -- every site makes its own, at its own place in the
// text --, OP_LATE reads a member of OnePassArgs through it, OP_LATE_PTR a member that is a pointer (rebuilt from its
// 64 bits: a generic pointer to the compiler, see "GLOBAL accesses" below).  OnePassArgs lies at the start of the segment
// in both kernels (k_floor_fix: FloorFixArgs::P).
typedef const __attribute__((address_space(4))) char* op_late_t;
__device__ __forceinline__ op_late_t op_late_ptr() {
  op_late_t kp = (op_late_t)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  return kp;
}
#define OP_LATE(kp, type, member) (*(const __attribute__((address_space(4))) type*)((kp) + __builtin_offsetof(OnePassArgs, member)))
#define OP_LATE_PTR(kp, type, member) ((type)(uintptr_t)OP_LATE(kp, unsigned long long, member))

// exact float64 |X[f]|^2 of frame t (see k_decide_fast).  A rare path (about one wave in fifty): its arguments -- a dozen
// 64-bit values of the view -- are late arguments, read HERE instead of staying live in scalar registers from the entry
// block to the decision stage.
__device__ __forceinline__ double op_exact_power(const OnePassArgs& P, int64_t row, int64_t chunk, int64_t t, int f,
                                                 int lane) {
  const op_late_t kp4 = op_late_ptr();
  const int64_t s0 = t * OP_LATE(kp4, int32_t, A.g.H) - OP_LATE(kp4, int32_t, A.g.padL);
  const int64_t v_cs = OP_LATE(kp4, int64_t, A.view.cs), v_pad = OP_LATE(kp4, int64_t, A.view.pad), v_Lp = OP_LATE(kp4, int64_t, A.view.Lp),
                v_lo = OP_LATE(kp4, int64_t, A.view.lo), v_hi = OP_LATE(kp4, int64_t, A.view.hi), x_stride = OP_LATE(kp4, int64_t, stride_exact);
  const void* const x_exact = OP_LATE_PTR(kp4, const void*, x_exact);
  const int x_dtype = OP_LATE(kp4, int, dtype_exact);
  const char* const tab = OP_LATE_PTR(kp4, const char*, tab);
  // the ORIGINAL samples: view_sample on A.view's geometry with the caller's pointer / dtype / stride
  const int64_t e = chunk * v_cs - v_pad + s0;   // the frame's first sample in its row
  int a, b;
  exact1024_terms(s0, e, v_Lp, v_lo, v_hi, a, b);
  return exact1024_power(x_exact, x_dtype, row * x_stride + e, a, b, reinterpret_cast<const double*>(tab + OP_TAB_WIN64),
                         reinterpret_cast<const cx<double>*>(tab + OP_TAB_TW64), f, lane);
}

// the quiet NaN of a lost hand-off, made where it is needed (cold): as a plain constant it is hoisted out of the persistent
// tile loop into a register of its own, which then lives in scratch
__device__ __forceinline__ unsigned op_nan_bits() {
  unsigned v = 0x7fc00000u;
  asm volatile("" : "+v"(v));
  return v;
}

// GLOBAL accesses where the pointer was rebuilt from a 64-bit kernel argument (late arguments): such a pointer is a generic one to
// the compiler, its accesses are FLAT, and while a FLAT access is pending every wait the compiler emits is vmcnt(0) / lgkmcnt(0)
// -- never a partial vmcnt(N) -- which also waits for whatever the wave issued AFTER the value it needs (the next tile's
// prefetched samples, the open seam's loads) and for the write-through acknowledgements of the inline-asm sc1 stores.
// So the epilogue's 1 / envelope load and output stores, the mid-tile ticket draw and the error word go through
// address_space(1) pointers, and the smoothing stage's MFMA operands come from LDS (s_mc): profiles/onepass_chain.txt, D.
typedef float op_v4f __attribute__((ext_vector_type(4)));
#define OP_G4 __attribute__((address_space(1)))
__device__ __forceinline__ float4 op_ldg4(const float* p) {
  const op_v4f v = *(const OP_G4 op_v4f*)p;
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void op_stg4(float* p, float4 a) {
  const op_v4f v = {a.x, a.y, a.z, a.w};
  *(OP_G4 op_v4f*)p = v;
}
// The mid-tile ticket draw (and a halo tile's, which consumes it at once): a GLOBAL returning atomic whose result the compiler waits for where it is consumed.  The address
// passes through a vector register the compiler cannot see into: to a wave-uniform address the atomic optimizer applies its
// wave reduction (v_mbcnt / s_bcnt1 / v_readfirstlane), and the readfirstlane waits for the atomic three instructions later.
__device__ __forceinline__ unsigned op_draw_ticket_late(unsigned long long p64) {
  asm volatile("" : "+v"(p64));
  return __hip_atomic_fetch_add((__attribute__((address_space(1))) unsigned*)p64, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a lost hand-off's bit in the host-mapped error word (atomicOr_system on a GLOBAL pointer: cold, but its block lies inside
// the smoothing stage and the epilogue, and a FLAT access there is one the compiler must assume pending at the next join)
// (the word is host memory: the statement attribute of atomicOr_system keeps the compare-and-swap expansion -- an OR is not
// among the atomics the bus carries)
__device__ __forceinline__ void op_err_or(unsigned* p, unsigned bits) {
  __HIP_ATOMIC_BACKWARD_COMPAT_MEMORY {
    __hip_atomic_fetch_or((__attribute__((address_space(1))) unsigned*)p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// lane ^ M (M < 32) by ds_swizzle: the pattern is an immediate.  __shfl_xor's ds_bpermute takes its lane index from a register,
// and the indices of a wave's xor steps -- loop-invariant -- were hoisted out of the persistent tile loop: three registers
// live through every phase of a kernel that sits at its 168, one of them in scratch in the PROP instantiation.
template <int M>
__device__ __forceinline__ int op_xor_lanes(int v) {
  static_assert(M > 0 && M < 32, "within a half-wave");
  return __builtin_amdgcn_ds_swizzle(v, (M << 10) | 0x1f);
}

// OP_ABLATE (development only, default 0; results are wrong): 1 no decision stage, 2 no wait for the
// neighbours' flags, 8 no exact refinement, 16 no wait for the previous tile's trailing hops
#ifndef OP_ABLATE
#define OP_ABLATE 0
#endif
// LAUNCH PLAN: three places of the PERSIST instantiations evaluate a ticket against the launch plan (onepass_plan.hpp) instead
// of deriving the tile's coordinates field by field: the loop top (u, jt, row, chunk by multiply-high), prefetch_next and the
// epilogue.  The publish stage and seam_issue measured below 1 % of a step as ceilings and are left alone; the loop top keeps
// its own tile_src: from the plan it cost 30 scalar registers and time (profiles/onepass_tile_plan.txt; the builds that
// measured both: tools/experiments/onepass_plan_ablate.patch).
// OP_TRACE (development only): per-phase shader-clock stamps of every non-halo wave, summed into P.trace (tools/
// trace_onepass.py): where a tile's lifetime goes
#if OP_TRACE
#define OP_STAMP(i)                                                                                   \
  do {                                                                                                \
    const long long t_now_ = clock64();                                                               \
    if (lane == 0 && t_slot_) t_slot_[i] = (unsigned)(t_now_ - t_prev_);                              \
    t_prev_ = t_now_;                                                                                 \
  } while (0)
#else
#define OP_STAMP(i) do { } while (0)
#endif

// PROP: prop_decrease < 1 (stationary.py:108-114 applies it BEFORE the smoothing: mask = p K / ktot + (1 - p) edge,
// edge = the smoothing filter's weight inside the spectrogram -- 1 except near its borders)
// LOSE (tests only, SG_OPT_INJECT_HANDOFF_FAULT bits 3..4): an instantiation whose polls give up at once -- the timeout
// branch of every hand-off (error word, NaN-poisoned hops) runs without a second of spinning and without a test
// argument in the product kernel, whose register allocation sits at the 168-VGPR edge.
// REDO: the second launch of a call with the in-kernel floor test (its own instantiation: its launches are their own row in
// a profile -- when no chunk reported they return at once, and would halve the gate's average duration -- and the first
// launch carries no test for it).
// PERSIST (round 6): a workgroup LOOPS over tickets instead of handling one tile.  What that buys -- a tile's first two phases
// (ticket atomic + constant tables: one memory round trip; span loads + compare constants: a second one) were 11.4 k of the
// 58.7 k cycles a wave lives (profiles/r03_onepass_phase_trace.txt), pure memory latency that the other two workgroups of the
// CU only partly cover (the kernel runs tiles x lifetime / 768 slots almost exactly):
//   * twiddles, window, byte-expansion table, compare constants (a lazy first launch has need == 0 in every unit: they do not
//     depend on the tile) and the floor test's bound are staged ONCE per workgroup;
//   * the NEXT ticket is drawn by thread 0 right after the neighbours' bits have arrived (never earlier: a workgroup that
//     held ticket j + 1 while waiting for tile j + 1's bits would wait for itself) and travels through LDS under the
//     smoothing stage's closing barrier;
//   * the next tile's span (five 16-byte loads per thread) and its slice of the floor test are issued after the inverse
//     transform, when the 64 spectrum registers are about to die, and land under the overlap-add and the epilogue;
//     the loop top only moves them from registers to LDS.
// Round 4's attempt at this died of loop-carried kernel arguments (160 spilled SGPRs).  Here NOTHING of the argument struct
// is loop-carried: every iteration reads `P` through late_args() -- an opaque pointer to the kernel-argument segment made
// inside the loop body, so no load from it can be hoisted -- and thread / lane indices come from an opaque copy of
// threadIdx.x.  Loop-carried: the parity of the ticket slot, the "prefetched" flag, one VGPR of floor-test bound and the 25
// VGPRs of prefetched samples.
// Deadlock freedom as before (tickets; publish before wait); a launch needs two resident workgroups, and draws
// total_tiles + gridDim.x tickets (every workgroup ends on one ticket >= total_tiles).
// Not for REDO / LOSE / a-priori floor flags (compare constants depend on the unit there) / SG_OPT_TILE_ORDER 1.
// DEFERRED SEAM (PERSIST only; profiles/onepass_chain.txt, B).  An interior (tile_fast) tile j used to end by polling for tile j - 1's three
// trailing partial hops.  Tile j - 1 runs in near lockstep and publishes them in its own last phase, so tile j always paid a
// write-through plus a read round trip with nothing left to hide it behind (phase 13 of the trace).  Now tile j publishes its
// trailing partials as before but leaves its three LEADING hops open: waves 0 - 2 write their un-normalised partial sums where
// the finished samples will go (one float4 per lane; the same lane reads them back -- four loop-carried registers were 19
// spilled ones in a kernel that sits at its 168) and thread 0 notes the tile's ticket and poison bit in s_misc[0].  One tile
// later the workgroup loads them and tile j - 1's granules before the overlap-add's closing barrier -- published a whole
// tile ago -- and finishes the hops in that iteration's epilogue: previous trailing + own leading, poison, normalise, store, the same sums
// in the same order.  A tag that is still not current falls back to the bounded poll (OP_SPIN_MAX, NaN, error word).  An
// open seam is closed on the spot before the workgroup leaves, in a halo tile's early exit, and in the epilogue of a tile
// that is not tile_fast (those keep the immediate protocol for their own hops).  Deadlock freedom: a seam waits for a tile
// with a LOWER ticket than any this workgroup has held since, and publishing never waits.
#ifndef OP_OCC
#define OP_OCC 3   // workgroups per CU the register budget is set for (development builds: 2 shows the unconstrained pressure)
#endif
#define OP_DONE { if (PERSIST) continue; return; }
constexpr unsigned OP_SEAM_NONE = 0xffffffffu;   // s_misc[0] (PERSIST): ticket | poison << 31 of the tile whose leading hops are open
// MERGED (REDO only): the tile runs inside k_floor_fix (below), the one launch that follows the first launch of a lazy call.
// Its ticket was drawn by the wrapper (`pre_ticket`), it waits for the float64 band maxima of its unit (FloorWait) before it
// reads them, and it reads them past the caches that are not coherent between XCDs.
struct FloorWait {
  const unsigned long long* arrive;   // [units] {count, epoch}: maxima workgroups of the unit that have finished, in this launch
  unsigned blocks;                    // maxima workgroups per unit
  unsigned lose;                      // tests (SG_OPT_INJECT_HANDOFF_FAULT): the wait gives up at once
};
template <int WAVES, bool PROP, bool LOSE = false, bool REDO = false, bool PERSIST = false>
__global__ __launch_bounds__(WAVES * 64, OP_OCC) void k_gate_onepass(OnePassArgs Pk) {
  constexpr bool MERGED = false;
  [[maybe_unused]] constexpr unsigned pre_ticket = 0u;
  [[maybe_unused]] constexpr FloorWait fw{};
#include "onepass_tile.hpp"
}
// k_floor_fix's tile role: the REDO tile of ticket `pre_ticket`, behind the wait for its unit's band maxima
template <int WAVES, bool PROP>
__device__ __forceinline__ void floor_fix_tile(const OnePassArgs& Pk, unsigned pre_ticket, FloorWait fw) {
  constexpr bool LOSE = false, REDO = true, PERSIST = false, MERGED = true;
#include "onepass_tile.hpp"
}

// The floor fix-up of a lazy call as ONE launch behind the first gate launch (before: k_stft_bits<MODE 0> + the REDO
// instantiation, two launches that both return on alim[1] != need_tag in the common case -- each a launch boundary of ~4.7 us).
//   * Every workgroup reads that word first and leaves when no unit reported: before tables, ticket and LDS.
//   * Otherwise it draws a ticket from the launch's own counter (zeroed by the first launch's ticket-0 workgroup) and takes
//     one role: tickets [0, n_max) are the frame blocks of the float64 band maxima (ticket = unit * blocks + block; the body
//     of k_stft_bits<MODE 0>, fused.hpp), tickets [n_max, n_max + total_tiles) the REDO tiles (floor_fix_tile).
//   * A maxima workgroup of a reported unit, once every one of its atomics on pmax has returned, adds one to the unit's
//     arrival word {count, epoch}: an atomicMax with {0, epoch} opens the word for this launch (epochs only grow: nothing is
//     cleared per call), an atomicAdd counts.  No fence: the atomics are agent-scope, carried out past the per-XCD L2s, and
//     the tiles read count and maxima with sc1 loads (a device-scope release would write back the XCD's L2: DESIGN 8).
//   * A tile of a reported unit waits for `blocks` arrivals (onepass_tile.hpp, MERGED: bounded, with the progress argument).
// OnePassArgs comes FIRST in the argument struct: the tile reads its arguments from the start of the kernel-argument segment.
struct FloorFixArgs {
  OnePassArgs P;                // the REDO launch's arguments: ticket = the launch's own counter, epoch = this launch's
  View vx;                      // the caller's samples in their own dtype (the maxima are exact)
  const cx<double>* tw64;
  const double* wfull64;
  unsigned long long* arrive;   // [units]
  unsigned n_max, blocks;       // floor_fix_plan (onepass_plan.hpp)
  unsigned lose;
};
static_assert(__builtin_offsetof(FloorFixArgs, P) == 0, "late arguments");
constexpr int FFX_N = 512, FFX_WAVES = 4, FFX_FPW = 4;   // k_stft_bits<512, 4, 4, 0, 64>: OP_PLAN_FIX_FRAMES frames per block
static_assert(FFX_WAVES * FFX_FPW == OP_PLAN_FIX_FRAMES, "onepass_plan.hpp");
template <int WAVES, bool PROP>
__global__ __launch_bounds__(WAVES * 64, 2) void k_floor_fix(FloorFixArgs F) {   // (two per CU: the tile role without the scratch that the gate's budget of 168 registers costs it next to the float64 role)
  static_assert(WAVES == FFX_WAVES, "one workgroup shape for both roles");
  if (F.P.alim[1] != F.P.tc.need_tag) return;   // no unit of this call reported (the common case)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* s_tk = reinterpret_cast<unsigned*>(smem);
  if (threadIdx.x == 0) s_tk[0] = atomicAdd(F.P.ticket, 1u);
  __syncthreads();
  const unsigned tk = (unsigned)__builtin_amdgcn_readfirstlane((int)s_tk[0]);
  __syncthreads();   // (the word belongs to the role's own LDS layout from here on)
  if (tk < F.n_max) {
    const unsigned u = tk / F.blocks, bx = tk - u * F.blocks;
    const bool live = stft_bits_block<FFX_N, FFX_WAVES, FFX_FPW, 0, 64, true>(
        F.vx, F.P.A.g, F.tw64, F.wfull64, F.P.tc, F.P.mag_scale, F.P.top_db,
        reinterpret_cast<unsigned long long*>(const_cast<double*>(F.P.tc.pmax)), nullptr, 0, bx, (int64_t)u);
    if (!live) return;   // the unit did not report (workgroup-uniform)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();     // every wave's atomics have returned
    if (threadIdx.x == 0) {
      unsigned long long* aw = F.arrive + u;
      const unsigned long long opened = atomicMax(aw, (unsigned long long)F.P.epoch << 32);
      asm volatile("" : : "v"(opened) : "memory");   // (returned: the word carries this launch's epoch before the count moves)
      atomicAdd(aw, 1ull);
    }
    return;
  }
  const unsigned tile = tk - F.n_max;
  if (tile >= F.P.total_tiles) return;   // (a grid rounded up past the last ticket)
  floor_fix_tile<WAVES, PROP>(F.P, tile, FloorWait{F.arrive, F.blocks, F.lose});
}

}  // namespace fast
}  // namespace sg
