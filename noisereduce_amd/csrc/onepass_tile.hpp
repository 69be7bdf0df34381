// The tile of a workgroup of the n_fft = 1024 one-pass gate: the function body of k_gate_onepass (every instantiation) and of
// floor_fix_tile, k_floor_fix's tile role (onepass.hpp includes this file once inside each).  Two copies of the TEXT, not one
// shared __device__ function: as a function inlined into a wrapper kernel the persistent instantiations came out with another
// schedule and register assignment, and their listing is held to the one that was measured.  In scope where this is included:
// WAVES, PROP, LOSE, REDO, PERSIST, MERGED (compile-time), Pk (the arguments), pre_ticket and fw (MERGED only).
// (No include guard: the file is meant to be included twice.)
  static_assert(WAVES == 4, "tile = 16 frames");
  static_assert(!PERSIST || (!LOSE && !REDO), "the persistent loop is the lazy first launch only");
  static_assert(!MERGED || (REDO && !LOSE), "k_floor_fix runs the REDO tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf* tw512 = reinterpret_cast<cf*>(smem);
  cf* regions = tw512 + FN;
  float* swin = reinterpret_cast<float*>(regions + WAVES * WAVE_CX_H);
  float* s_t2 = swin + 1024;
  unsigned long long* s_exp = reinterpret_cast<unsigned long long*>(s_t2 + T2_FLOATS);
  double* s_t2d = reinterpret_cast<double*>(s_exp + 256);   // exact compare constants (refinement), same order
  // the smoothing stage's three MFMA operands (OP_TAB_MCONST, 192 x 8 B): from LDS their wait is an lgkmcnt one -- as loads from
  // the table behind the bits' publish store the first MFMA waited for that store's write-through acknowledgement
  unsigned long long* s_mc = reinterpret_cast<unsigned long long*>(s_t2d + 514);
  unsigned* s_misc = reinterpret_cast<unsigned*>(s_mc + 192);   // [0] ticket, [1] lost hand-off, [4], [5]: PERSIST ticket slots
  unsigned char* s_ef = reinterpret_cast<unsigned char*>(s_misc + 8);  // PROP: integer weight (<= 81) of the valid taps along f, per bin
  constexpr int NF = 4 * WAVES;
  constexpr int SPAN = (NF - 1) * 256 + 1024, XPITCH = 288;
  static_assert((SPAN / 256) * XPITCH <= WAVES * WAVE_CX_H * 2, "span must fit the exchange slices");
  // span loads: one dword per thread and 256-sample row (lane-contiguous, 19 per thread).  16-byte loads (five per thread)
  // need aligned register QUADS; held across the second half of a tile (PERSIST) the allocator could not place them next to
  // the 64 spectrum registers and spilled all of them -- a scratch store that waits for the load it was meant to hide
  constexpr int NQ = SPAN / 256;
  static_assert(SPAN % 256 == 0 && WAVES * 64 == 256, "one sample per thread and row");
  constexpr int SCAN_REG = 5;                     // floor-test slices up to 5 x 256 samples ride in registers

  if (REDO && Pk.alim[1] != Pk.tc.need_tag) return;   // second launch of a call none of whose units reported (the common case)
  double t2pre[3];   // compare constants of entries tid, tid + 256 and 512 (they do not depend on the ticket)
  unsigned alim_v = 0u;
  {
    const int tid = threadIdx.x, lane = tid & 63;
    // table loads first, the ticket's atomic behind them in the same queue: one memory round trip, not two
    static_assert(FN == 2 * WAVES * 64 && WAVES * 64 == 256, "one pass of the prologue loads per thread");
    const cf tw_a = reinterpret_cast<const cf*>(Pk.tab + OP_TAB_TW512)[(tid >> 4) * (tid & 15)];
    const cf tw_b = reinterpret_cast<const cf*>(Pk.tab + OP_TAB_TW512)[((tid + 256) >> 4) * (tid & 15)];
    const float4 w4 = reinterpret_cast<const float4*>(Pk.tab + OP_TAB_WIN)[tid];
    const unsigned long long e8 = reinterpret_cast<const unsigned long long*>(Pk.tab + OP_TAB_EXP8)[tid];
    const unsigned long long mc8 = reinterpret_cast<const unsigned long long*>(Pk.tab + OP_TAB_MCONST)[min(tid, 191)];
    t2pre[0] = Pk.tc.T2[perm_inv(tid)];
    t2pre[1] = Pk.tc.T2[perm_inv(tid + 256)];
    t2pre[2] = Pk.tc.T2[perm_inv(512)];
    if (!REDO && Pk.alim != nullptr) {
      // the floor test's compare constant: a VECTOR load behind the table loads (as a scalar load the compiler places it
      // at its use, after the span has landed: one more exposed round trip per tile, 5 us of the kernel)
      int z = 2 + min(lane & 15, OP_ALIM_BLOCKS - 1);   // one bound per band block of the noise statistics: minimum below
      asm volatile("" : "+v"(z));
      alim_v = Pk.alim[z];
    }
    if (tid == 0) {
      // (ticket_base == 0xffffffff: SG_OPT_TILE_ORDER 1, the block index instead of a ticket)
      if constexpr (MERGED) s_misc[0] = pre_ticket;   // (drawn by k_floor_fix before anything else)
      else s_misc[PERSIST ? 4 : 0] = Pk.ticket_base == 0xffffffffu ? blockIdx.x : atomicAdd(Pk.ticket, 1u) - Pk.ticket_base;
      s_misc[1] = 0u;   // set when a hand-off of this tile is lost: its output hops are POISONED (NaN), never plausible garbage
      if (PERSIST) s_misc[0] = OP_SEAM_NONE;
    }
    tw512[tid] = tw_a;
    tw512[tid + 256] = tw_b;
    reinterpret_cast<float4*>(swin)[tid] = w4;
    s_exp[tid] = e8;
    if (tid < 192) s_mc[tid] = mc8;
    if constexpr (PROP) {
      for (int f = tid; f <= 512; f += WAVES * 64) {
        const int lo = max(-Pk.nf, -f), hi = min(Pk.nf, 512 - f);
        int sum = 0;
        for (int a = lo; a <= hi; ++a) sum += Pk.nf + 1 - (a < 0 ? -a : a);
        s_ef[f] = (unsigned char)sum;
      }
    }
    if constexpr (PERSIST) {
      // need == 0 in every unit of a lazy first launch: one set of compare constants for all of the workgroup's tiles
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int i = tid + k * WAVES * 64;
        if (i > 512) break;
        s_t2[t2_pos(i)] = t2_to_f32(t2pre[k], 4.0);
        s_t2d[i] = t2pre[k];
      }
      for (int off = 1; off < 16; off <<= 1) alim_v = min(alim_v, (unsigned)__shfl_xor((int)alim_v, off));
      if (tid == 0) s_misc[2] = alim_v;   // (not a loop-carried register: it would live in scratch)
    }
  }
  __syncthreads();

  // what one tile reads from the recording: its span, and its slice of the floor test's scan (see "floor test" below).
  // A function of the ticket alone: the loop top evaluates it for the tile at hand, the prefetch for the next one.
  struct TileSrc {
    const float* sp;        // first sample of the span
    bool blk_vec;           // interior tile of float32 input: five aligned 16-byte loads per thread
    const float* sc_base;   // floor-test slice that rides in registers (null: none, or the slow loop)
    int sc_n1;              // its length - 1
    int64_t s0b, sc_lo, sc_last, sc_lenA, sc_c0, sc_c1;
  };
  auto tile_src = [](const OnePassArgs& P, int64_t row, int64_t chunk, int jt, bool test) -> TileSrc {
    const ApplyArgs& A = P.A;
    TileSrc S;
    const int64_t tf_tile = A.h_begin - 3 + (int64_t)jt * NF;
    S.s0b = tf_tile * 256 - A.g.padL;
    const int64_t gb = chunk * A.view.cs - A.view.pad + S.s0b;
    S.sp = (const float*)A.view.x + row * A.view.stride + gb;
    S.blk_vec = A.view.dtype == 0 && tf_tile >= 0 && tf_tile + NF <= A.g.T && S.s0b >= 0 && S.s0b + SPAN <= A.view.Lp &&
                gb >= A.view.lo && gb + SPAN <= A.view.hi && (reinterpret_cast<uintptr_t>(S.sp) & 15) == 0;
    S.sc_base = nullptr;
    S.sc_n1 = 0;
    S.sc_lo = S.sc_last = S.sc_lenA = S.sc_c0 = S.sc_c1 = 0;
    if (test) {
      const int64_t g0 = chunk * A.view.cs - A.view.pad;
      const int64_t s_lo = max<int64_t>(0, A.view.lo - g0), s_hi = min<int64_t>(A.view.Lp, A.view.hi - g0);
      const int64_t sp0 = (A.h_begin - 3 - NF) * 256 - A.g.padL;                                   // tile -1's span begins
      const int64_t sp1 = (A.h_begin - 3 + (int64_t)A.n_tiles * NF) * 256 - A.g.padL + SPAN;       // tile n_tiles' span ends
      const int64_t first = min(s_hi, max(s_lo, sp0));
      S.sc_lo = s_lo;
      S.sc_last = max(s_lo, min(s_hi, sp1));
      S.sc_lenA = first - s_lo;
      S.sc_c0 = (int64_t)(jt + 1) * P.scan_q;
      S.sc_c1 = min(S.sc_c0 + P.scan_q, S.sc_lenA + (s_hi - S.sc_last));
      if (A.view.dtype == 0 && S.sc_c1 > S.sc_c0 && S.sc_c1 - S.sc_c0 <= SCAN_REG * WAVES * 64 &&
          (S.sc_c1 <= S.sc_lenA || S.sc_c0 >= S.sc_lenA)) {
        S.sc_base = (const float*)A.view.x + row * A.view.stride + g0 +
                    (S.sc_c1 <= S.sc_lenA ? s_lo + S.sc_c0 : S.sc_last + (S.sc_c0 - S.sc_lenA));
        S.sc_n1 = (int)(S.sc_c1 - S.sc_c0) - 1;
      }
    }
    return S;
  };
  // the same for a tile the launch plan knows as blk_vec (an interior unit's: nothing of the view is read)
  static_assert(NF == OP_PLAN_NF && SPAN == OP_PLAN_SPAN && SCAN_REG * WAVES * 64 == OP_PLAN_SCAN_MAX, "onepass_plan.hpp");
  auto tile_src_plan = [](const OpPlan& L, const OpTile& tl) -> TileSrc {
    TileSrc S;
    const float* base = (const float*)(const __attribute__((address_space(1))) float*)(uintptr_t)L.src;
    S.sp = base + op_plan_src_off(L, tl);
    S.blk_vec = true;
    S.s0b = (int64_t)L.s0b0 + (int64_t)tl.jt * OP_PLAN_TILE;
    const OpScan sc = op_plan_scan(L, tl);
    S.sc_lo = 0;
    S.sc_last = L.sc_last;
    S.sc_lenA = L.sc_lenA;
    S.sc_c0 = sc.c0;
    S.sc_c1 = sc.c1;
    S.sc_base = sc.has ? base + sc.off : nullptr;
    S.sc_n1 = sc.has ? (int)(sc.c1 - sc.c0) - 1 : 0;
    return S;
  };
  // loop-carried (PERSIST): the samples of the tile at hand, issued by the previous iteration
  float q[NQ];
  float sc[SCAN_REG];
  bool pf = false;
  constexpr bool DEFER = PERSIST;   // the deferred seam (onepass.hpp)
  // where the open seam of tile `pend` lives: the previous tile's trailing granules of hop `wv`, the output samples
  auto seam_where = [](unsigned pend, const unsigned long long*& src, float*& dst) {
    const op_late_t kq = op_late_ptr();
    const unsigned tk = pend & 0x7fffffffu;
    const unsigned ntl = (unsigned)OP_LATE(kq, int, A.n_tiles), nttq = ntl + 2u;
    const unsigned uq = tk / nttq;
    const int jq = (int)(tk % nttq) - 1;
    const unsigned guq = (unsigned)(OP_LATE(kq, int64_t, A.view.unit0) + uq), nchq = (unsigned)OP_LATE(kq, int32_t, A.view.n_chunks);
    const int64_t rowq = guq / nchq, chunkq = OP_LATE(kq, int64_t, A.view.c0) + guq % nchq;
    const int64_t tfq = OP_LATE(kq, int64_t, A.h_begin) - 3 + (int64_t)jq * NF;
    const int64_t pb0 = tfq * 256 - OP_LATE(kq, int32_t, A.g.padL);
    const int64_t gi00 = chunkq * OP_LATE(kq, int64_t, A.om.g_step) + (pb0 - OP_LATE(kq, int64_t, A.om.p0));
    // (the tile's part is wave-uniform: two scalar registers each, the lane's offset is added where it is used)
    auto uni = [](const void* p_) -> char* {
      const unsigned long long v_ = (unsigned long long)(uintptr_t)p_;
      return (char*)(uintptr_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v_ >> 32)) << 32) |
                                (unsigned)__builtin_amdgcn_readfirstlane((int)v_));
    };
    dst = (float*)uni(OP_LATE_PTR(kq, float*, A.om.out) +
                      (rowq * OP_LATE(kq, int64_t, A.om.stride) + gi00 - OP_LATE(kq, int64_t, A.om.g0)));
    src = (const unsigned long long*)uni(OP_LATE_PTR(kq, const unsigned long long*, part2) +
                                         ((size_t)uq * ntl + jq - 1) * 3 * 256);
  };
  auto seam_off = [](int wv, int s4_) -> int { return wv * 256 + s4_; };   // a lane's four samples of hop `wv`
  // previous trailing + own leading, poison, normalise, store: the tail of the tile_fast epilogue.  g4 = the four granules
  // as loaded (a tag that is not current yet: the bounded poll)
  auto seam_finish = [&](unsigned pend, int wv, int s4_, unsigned long long g0_, unsigned long long g1_, unsigned long long g2_,
                        unsigned long long g3_, float* dst, float4 ld, float4 nrm) {
    op_v4u ga = {(unsigned)g0_, (unsigned)(g0_ >> 32), (unsigned)g1_, (unsigned)(g1_ >> 32)};
    op_v4u gb = {(unsigned)g2_, (unsigned)(g2_ >> 32), (unsigned)g3_, (unsigned)(g3_ >> 32)};
    const op_late_t kq = op_late_ptr();
    const unsigned e = OP_LATE(kq, unsigned, epoch);
    if (!(ga[1] == e && ga[3] == e && gb[1] == e && gb[3] == e)) {   // (cold)
      const unsigned long long* src;
      float* d2_;
      seam_where(pend, src, d2_);
      src += seam_off(wv, s4_);
      for (int spin = 0;; ++spin) {
        asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(ga), "=&v"(gb) : "v"(src) : "memory");
        if (ga[1] == e && ga[3] == e && gb[1] == e && gb[3] == e) break;
        if (spin >= OP_SPIN_MAX) {
          op_err_or(OP_LATE_PTR(kq, unsigned*, err), 2u);
          ga[0] = ga[2] = gb[0] = gb[2] = op_nan_bits();   // the previous tile's share is unknown: NaN, not a partial sum
          break;
        }
        op_poll_sleep();
      }
    }
    const float psn = __uint_as_float((pend >> 31) * 0x7fc00000u);   // NaN or 0 (scalar arithmetic: as a select the constant was hoisted out of the tile loop and spilled)
    float4 a;
    a.x = __uint_as_float(ga[0]) + ld.x;
    a.y = __uint_as_float(ga[2]) + ld.y;
    a.z = __uint_as_float(gb[0]) + ld.z;
    a.w = __uint_as_float(gb[2]) + ld.w;
    a.x = (a.x + psn) * nrm.x; a.y = (a.y + psn) * nrm.y; a.z = (a.z + psn) * nrm.z; a.w = (a.w + psn) * nrm.w;
    op_stg4(dst + seam_off(wv, s4_), a);
  };
  // an open seam closed on the spot (cold: the workgroup leaves, a halo tile): waves 0 - 2
  auto seam_close = [&](unsigned pend, int tid_) {
    const int wv = tid_ >> 6, s4_ = (tid_ & 63) * 4;
    if (pend == OP_SEAM_NONE || wv >= 3) return;
    const op_late_t kq = op_late_ptr();
    const float4 nrm = op_ldg4(&reinterpret_cast<const float*>(OP_LATE_PTR(kq, const char*, tab) + OP_TAB_INVN)[s4_]);
    const unsigned long long* src;
    float* dst;
    seam_where(pend, src, dst);
    const float4 ld = op_ldg4(dst + seam_off(wv, s4_));   // the leading partial this lane left there
    seam_finish(pend, wv, s4_, 0ull, 0ull, 0ull, 0ull, dst, ld, nrm);   // (tag 0 is never current: the epoch starts at 1 -- straight to the poll)
  };

  for (unsigned iter = 0; iter == 0u || PERSIST; ++iter) {
  // ---- PERSIST: nothing of the arguments or the thread's indices survives an iteration (see above) ----
  const OnePassArgs& P = *late_args<OnePassArgs>();   // (every instantiation: 0 spilled SGPRs; by value, outside PERSIST, they spilled)
  int tid = threadIdx.x;
#if OP_TRACE
  long long t_prev_ = clock64();   // (PERSIST: phase 0 = the wait at the loop-top barrier)
  unsigned* t_slot_ = nullptr;   // known once the ticket is
#endif
  if constexpr (PERSIST) {
    asm volatile("" : "+v"(tid));
    // (round 6, found with the builds listed in DESIGN 3: on the halo tiles' path to this barrier -- s_misc[next slot] = ticket;
    // continue -- the compiler emits NO s_waitcnt lgkmcnt(0) between the ds_write and the s_barrier (gfx950 has no automatic
    // wait before a barrier; the normal path's barrier has one).  Alone on the GPU the LDS write always landed before the other
    // waves' read of the slot; next to a kernel that keeps the LDS queues busy a wave could read the slot's PREVIOUS content --
    // the ticket of two tiles ago -- and the workgroup ran a tile with two different tickets: mis-gated tiles, lost hand-offs,
    // wild addresses.  The wait is explicit now.)
    if (iter != 0u) {
#if !OP_NO_LOOPTOP_WAIT
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
      __syncthreads();   // the previous tile's epilogue has read every hop accumulator: the slices are free
    }
  }
  const ApplyArgs& A = P.A;
  const Geom& G = A.g;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const unsigned tk_slot = PERSIST ? 4u + (iter & 1u) : 0u;
  const unsigned ticket = PERSIST ? (unsigned)__builtin_amdgcn_readfirstlane((int)s_misc[tk_slot]) : s_misc[0];
  if (PERSIST && ticket >= P.total_tiles) {   // (workgroup-uniform)
    if constexpr (DEFER) seam_close((unsigned)__builtin_amdgcn_readfirstlane((int)s_misc[0]), tid);
    return;
  }
  if (PERSIST && tid == 0) s_misc[1] = 0u;
#if OP_TRACE
  t_slot_ = P.trace + ((size_t)ticket * 4 + wave) * 16;
  if (lane == 0) t_slot_[14] = (blockIdx.x + 1u) | (iter << 16);   // who took the ticket up (sg_debug_counter 8 reads it after a lost hand-off)
#endif
  OP_STAMP(0);   // tables + ticket
  [[maybe_unused]] int ntt;   // tiles per unit incl. one decide-only halo tile per side
  int64_t u, row, chunk;
  int jt;                     // -1 and n_tiles: halo tiles
  bool halo_tile;
  if constexpr (PERSIST) {
    // the launch plan: both quotients by multiply-high and shifts
    const OpTile tl = op_plan_tile(P.plan, ticket);
    ntt = (int)P.plan.ntt;
    u = tl.u;
    jt = tl.jt;
    halo_tile = jt < 0 || jt >= ntt - 2;
    row = tl.row;
    chunk = P.plan.c0 + tl.k;
  } else {
    ntt = A.n_tiles + 2;
    u = ticket / (unsigned)ntt;
    jt = (int)(ticket % (unsigned)ntt) - 1;
    halo_tile = jt < 0 || jt >= A.n_tiles;
    // (32-bit division: unit indices fit, and a 64-bit divide is ~150 instructions of every workgroup's prologue)
    const unsigned gu = (unsigned)(A.view.unit0 + u), nch = (unsigned)A.view.n_chunks;
    row = gu / nch;
    chunk = A.view.c0 + gu % nch;
  }
  // Floor flags of the unit.  lazy (P.alim set): the first launch assumes "not live" and runs the floor test on the
  // samples it stages (below); the second launch (REDO) serves exactly the units whose test fired.
  const bool lazy = PERSIST || P.alim != nullptr;
  const int need = (lazy && !REDO) ? 0 : need_of(P.tc, u);
  if (REDO && need == 0) return;   // whole workgroup
  // (first launch: the second launch's work counter -- it only counts when a unit reported -- starts from zero)
  if (!REDO && lazy && ticket == 0u && tid == 0) P.ticket[8] = 0u;
  const bool floor_live = need == 1;
  if constexpr (MERGED) {
    // The unit's band maxima are made in THIS launch (k_floor_fix): wait until every maxima workgroup of the unit has
    // arrived.  Progress: every maxima ticket is lower than every tile ticket, a workgroup draws its ticket before anything
    // else, and maxima work waits for nothing -- so whenever a tile waits here, every block it waits for is held by a
    // workgroup that is already running and finishes on its own.  The wait comes before the tile publishes: a tile that
    // waits for a neighbour's bits waits for a workgroup that is past this point or, by the same argument, gets past it.
    // Bounded like every poll (OP_SPIN_MAX): a wait that gives up sets bit 3 of the error word (the call returns
    // SG_E_HANDOFF) and poisons the tile's hops.  Only a unit with need == 1 has maxima work (need == 2: no cell passes).
    if (floor_live) {
      const unsigned long long* aw = fw.arrive + u;
      const unsigned e = P.epoch;
      for (int spin = 0;; ++spin) {
        const unsigned long long w = op_ld8_sc1(aw);
        if (!fw.lose && (unsigned)(w >> 32) == e && (unsigned)w >= fw.blocks) break;
        if (fw.lose || spin >= OP_SPIN_MAX) {
          op_err_or(P.err, 8u);
          s_misc[1] = 1u;   // the unit's maxima are unknown: every hop the tile finalises or hands on becomes NaN
          break;
        }
        op_poll_sleep();
      }
    }
  }

  // compare constants (x4: the split works on 2X), permuted like the lanes' entries -- see k_decide_fast
  auto t2eff = [&](int f, double v) -> double {
    if (floor_live) {
      // (MERGED: the maxima were raised by workgroups of this launch, maybe on another XCD -- a load past the L1 and the
      // non-coherent L2 lines, like the granule loads)
      const double pm = MERGED ? __longlong_as_double((long long)op_ld8_sc1(&P.tc.pmax[u * G.FS + f])) : P.tc.pmax[u * G.FS + f];
      double fl = cell_db(pm, P.mag_scale) - P.top_db;
      if (fl > P.tc.thresh[f]) v = -1.0;
    }
    if (need & 2) v = T2_NEVER;   // non-finite sample in the unit (wins over 1: lazy tiles OR their verdicts together)
    return v;
  };
  const int64_t tf_tile = A.h_begin - 3 + (int64_t)jt * NF;  // first frame of the tile (abutting tiles)
  const int64_t tq = tf_tile + 4 * wave;
  const int64_t t = tq + g;                                  // this lane group's frame
  const bool fvalid = t >= 0 && t < G.T;
  cf* fb = regions + wave * WAVE_CX_H + frame_base_h(g);

  // ---- stage the tile's contiguous sample span: interior tiles of float32 input with 16-byte loads, the others
  // (unit edges, halo tiles) sample by sample through view_sample -- zero outside the readable range ------------
  bool blk_vec;
  {
    // ---- floor test (lazy, first launch).  k_unit_absmax + k_prep_thresh read the whole recording before the gate to
    // decide, per unit, whether _amp_to_db's floor max(dB, band max - top_db) (spectralgate/utils.py:16) can lift a band
    // over its threshold: max|x| sum|w| bounds every |X|.  The tiles of a unit stage nearly all of its window anyway:
    // each compares the largest sample it staged with the same bound (alim).  The rest of the window -- the chunk's
    // padding, which no tile of THIS unit transforms: A = [s_lo, first span) and B = [last span's end, s_hi) -- is dealt
    // to the unit's tiles in slices of P.scan_q samples of A ++ B (~1200 at the default chunking: five loads per thread,
    // in flight with the span's).  A tile whose test fires reports its unit: need_floor[u] |= 1 (2: a non-finite
    // sample), the unit's band maxima cleared for the float64 pre-pass that follows.  This launch's result for a reported
    // unit is overwritten by the second (REDO).
    const bool test = !REDO && lazy;
    const TileSrc S = tile_src(P, row, chunk, jt, test);
    blk_vec = S.blk_vec;
    const int64_t s0b = S.s0b;
    auto fill_t2 = [&]() {
      if constexpr (!PERSIST) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int i = tid + k * WAVES * 64;
          if (i > 512) break;
          const double v = t2eff(perm_inv(i), t2pre[k]);
          s_t2[t2_pos(i)] = t2_to_f32(v, 4.0);
          s_t2d[i] = v;   // the rare exact re-evaluation compares against this (no log10 in the hot kernel body)
        }
      }
    };
    float* xs = reinterpret_cast<float*>(regions);
    unsigned mi = 0u;   // max |x| seen by this thread, as a bit pattern (sign cleared: NaN / Inf order above every finite value)
    auto ab = [](float x) -> unsigned { return __float_as_uint(x) & 0x7fffffffu; };
    // issued BEHIND the span's loads (every later phase waits for the span), consumed after them.  One scalar base + a
    // clamped lane offset: the slice's tail re-reads its last sample (a predicated load is a branch and a copy)
    if (!pf) {
      if (S.blk_vec) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) q[k] = S.sp[tid + k * 256];
      }
      if (S.sc_base != nullptr) {
#pragma unroll
        for (int k = 0; k < SCAN_REG; ++k) sc[k] = S.sc_base[min(tid + k * WAVES * 64, S.sc_n1)];
      }
    }
    fill_t2();   // (span loads in flight while the compare constants are built)
    if (blk_vec) {
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        xs[k * XPITCH + tid] = q[k];
        mi = max(mi, ab(q[k]));
      }
    } else {
      for (int i = tid; i < SPAN; i += WAVES * 64) {
        const float xv = (float)view_sample(A.view, row, chunk, s0b + i);
        xs[(i >> 8) * XPITCH + (i & 255)] = xv;
        mi = max(mi, ab(xv));
      }
    }
    if (test) {
      if (S.sc_base != nullptr) {
#pragma unroll
        for (int k = 0; k < SCAN_REG; ++k) mi = max(mi, ab(sc[k]));
      } else {
        // the slice that straddles A | B, long slices (padding much longer than the kept part), other sample types: a
        // loop after the span
        for (int64_t i = S.sc_c0 + tid; i < S.sc_c1; i += WAVES * 64)
          mi = max(mi, ab((float)view_sample(A.view, row, chunk, i < S.sc_lenA ? S.sc_lo + i : S.sc_last + (i - S.sc_lenA))));
      }
      unsigned alim_t = PERSIST ? s_misc[2] : alim_v;
      if constexpr (!PERSIST)
        for (int off = 1; off < 16; off <<= 1) alim_t = min(alim_t, (unsigned)__shfl_xor((int)alim_t, off));
      const bool hit = mi >= alim_t;
      if (__any(hit)) {   // wave-uniform, rare
        const bool nonfinite = __any(mi >= 0x7f800000u);
        double* pm = const_cast<double*>(P.tc.pmax) + u * G.FS;
        for (int f = lane; f < G.FS; f += 64) pm[f] = 0.0;
        if (lane == 0) {
          atomicMax(reinterpret_cast<unsigned*>(const_cast<int*>(P.tc.need_floor)) + u, (P.tc.need_tag << 2) | (nonfinite ? 2u : 1u));
          P.alim[1] = P.tc.need_tag;
          P.err[1] = P.epoch;   // host-mapped: "a unit of launch `epoch` reported" (the host picks the a-priori test next time)
        }
      }
    }
  }
  __syncthreads();  // tables, compare constants and span staged
  OP_STAMP(1);   // span + compare constants

  // ---- gather: v[r] = (x[2c + 32r], x[2c + 32r + 1]) * window ---------------------------------------
  cf v[32];
  float nrm2 = 0.f;
  {
    const float* xs = reinterpret_cast<const float*>(regions) + (4 * wave + g) * XPITCH + 2 * c;
    const float2* wl = reinterpret_cast<const float2*>(swin + 2 * c);
    if (blk_vec) {
#pragma unroll
      for (int r = 0; r < 32; ++r) {
        const float2 x2 = *reinterpret_cast<const float2*>(xs + (r >> 3) * XPITCH + 32 * (r & 7));
        const float2 w2 = wl[16 * r];
        v[r] = {x2.x * w2.x, x2.y * w2.y};
      }
    } else {
#pragma unroll
      for (int r = 0; r < 32; ++r) {
        float2 x2 = *reinterpret_cast<const float2*>(xs + (r >> 3) * XPITCH + 32 * (r & 7));
        if (!fvalid) x2 = make_float2(0.f, 0.f);   // frames before / past the unit: zeros
        const float2 w2 = wl[16 * r];
        v[r] = {x2.x * w2.x, x2.y * w2.y};
      }
    }
  }
  __syncthreads();  // every lane has its samples: the span may be overwritten by the exchanges
  OP_STAMP(2);   // gather
  {
#pragma unroll
    for (int r = 0; r < 32; ++r) nrm2 += v[r].x * v[r].x + v[r].y * v[r].y;
    nrm2 += __int_as_float(op_xor_lanes<1>(__float_as_int(nrm2)));
    nrm2 += __int_as_float(op_xor_lanes<2>(__float_as_int(nrm2)));
    nrm2 += __int_as_float(op_xor_lanes<4>(__float_as_int(nrm2)));
    nrm2 += __int_as_float(op_xor_lanes<8>(__float_as_int(nrm2)));
  }
  {
    // an opaque ZERO OFFSET (not an opaque pointer: that would lose the LDS address space and turn every
    // access into a FLAT instruction) keeps the loop-invariant twiddle reads from being hoisted and pinned
    int z0 = 0;
    asm volatile("" : "+v"(z0));
    fft512_fwd_half(v, fb, tw512 + z0, c);
  }
  OP_STAMP(3);   // forward transform

  // ---- decide (k_decide_fast): mask bits of this lane's 32 entries -----------------------------------
  // ---- real-FFT split, ONCE: conjugate pair (a, b) = (Zc[k], Zc[N-k]) -> X2[k] = E + w O, conj-pair value
  // X2n = E - w O (both 2x the spectrum; E = a + conj b, O = (a - conj b)/i).  Slot order (see k_apply_fast):
  // lanes >= 1 pair registers (sl, 31 - sl); lane 0 pairs its self-conjugate rows differently, handled by
  // selects on the way in HERE only -- the decision stage and the mask stage both read pa/pb in slot order.
  cf pa[16], pb[16];
  const cf raw0 = v[0], raw8 = v[8];   // lane 0: bins 0 / 512 and bin 256 are not part of a pair
  const bool l0 = c == 0;
  cf wlo = reinterpret_cast<const cf*>(P.tab + OP_TAB_TW1024)[c];
  asm volatile("" : "+v"(wlo.x), "+v"(wlo.y));
  cf whi = wlo;
  {
    const cf w16 = reinterpret_cast<const cf*>(P.tab + OP_TAB_TW1024)[16];
    if (l0) whi = {-w16.y, w16.x};  // i * w_1024^16
  }
  {
    auto sel = [&](cf a0, cf a1) -> cf { return {l0 ? a0.x : a1.x, l0 ? a0.y : a1.y}; };
    auto split = [&](cf a, cf b2, cf w, cf& xa, cf& xb) { split_pair(a, b2, w, xa, xb); };
    split(v[0], v[31], wlo, pa[0], pb[0]);
#pragma unroll
    for (int sl = 1; sl < 16; ++sl) {
      const cf a = sl < 8 ? v[sl] : sel(v[8 + sl], v[sl]);
      const cf b2 = sl < 8 ? sel(v[16 - sl], v[31 - sl]) : sel(v[39 - sl], v[31 - sl]);
      const cf w = mul_tw<false>(sl < 8 ? wlo : whi, twc<32>(sl), tws<32>(sl));
      split(a, b2, w, pa[sl], pb[sl]);
    }
  }

#define OP_PA(sl) pa[sl]
#define OP_PB(sl) pb[sl]
  OP_STAMP(4);   // split
  // ---- decide (k_decide_fast): mask bits of this lane's 32 entries -----------------------------------
  unsigned long long myword;  // lane c < 9 of group g: word c of frame tq + g
  {
    // compare constants are read from LDS where they are used (the spectra stay live through this phase:
    // 32 more registers for a preloaded table would spill)
    int zt = 0;
    asm volatile("" : "+v"(zt));
    const float* t2 = s_t2 + c * T2_PITCH + zt;
    const float t2_512 = s_t2[T2_POS512];
    const float d2 = nrm2 > 0.f ? 8.0f * 2.3283064e-10f * nrm2 : -1.0f;
    // Decisions as SIGN BITS shifted into accumulators (v_alignbit: acc = acc << 1 | sign), no compares or selects:
    //   passes    <=>  T - P < 0                      (sign of nd)
    //   ambiguous <=>  d2 (P + T) - (T - P)^2 >= 0    (sign of e CLEAR)
    // Slot sl decides entry sl (accumulators A, in slot order: bit 15 - sl) and entry 31 - sl (accumulators B: bit
    // 15 - sl = entry 16 + that bit, already in place); A is bit-reversed at the end.
    unsigned pA = 0, pB = 0, nA = 0, nB = 0;
    auto decideA = [&](float Pw, float T) {
      const float nd = T - Pw;
      const float e = fmaf(-nd, nd, d2 * (Pw + T));
      pA = __builtin_amdgcn_alignbit(pA, __float_as_uint(nd), 31);
      nA = __builtin_amdgcn_alignbit(nA, __float_as_uint(e), 31);
    };
    auto decideB = [&](float Pw, float T) {
      const float nd = T - Pw;
      const float e = fmaf(-nd, nd, d2 * (Pw + T));
      pB = __builtin_amdgcn_alignbit(pB, __float_as_uint(nd), 31);
      nB = __builtin_amdgcn_alignbit(nB, __float_as_uint(e), 31);
    };
    bool pred512 = false, amb512 = false;
    {
      const float Pk = OP_PA(0).x * OP_PA(0).x + OP_PA(0).y * OP_PA(0).y;
      const float Pn = OP_PB(0).x * OP_PB(0).x + OP_PB(0).y * OP_PB(0).y;
      const float x0 = 2.f * (raw0.x + raw0.y), xN = 2.f * (raw0.x - raw0.y);
      const float P256 = 4.f * (raw8.x * raw8.x + raw8.y * raw8.y);
      decideA(l0 ? x0 * x0 : Pk, t2[0]);
      decideB(l0 ? P256 : Pn, t2[31]);
      const float P5 = xN * xN, d5 = P5 - t2_512;
      pred512 = l0 && d5 > 0.f;
      amb512 = l0 && d5 * d5 <= d2 * (P5 + t2_512);
    }
#pragma unroll
    for (int sl = 1; sl < 16; ++sl) {
      if ((sl & 3) == 0) __builtin_amdgcn_sched_barrier(0);  // keep the constant loads next to their use
      decideA(OP_PA(sl).x * OP_PA(sl).x + OP_PA(sl).y * OP_PA(sl).y, t2[sl]);
      decideB(OP_PB(sl).x * OP_PB(sl).x + OP_PB(sl).y * OP_PB(sl).y, t2[31 - sl]);
    }
    __builtin_amdgcn_sched_barrier(0);
    unsigned pred = (__brev(pA) >> 16) | (pB << 16);
    unsigned amb = ~((__brev(nA) >> 16) | (nB << 16));
    // a unit with non-finite samples (compare constants = T2_NEVER): NaN powers have no meaningful sign
    if (need == 2) { pred = 0; amb = 0; pred512 = false; amb512 = false; }
    if (!fvalid) { amb = 0; amb512 = false; pred = 0; pred512 = false; }
    // exact re-evaluation, one cell at a time, whole wave cooperating.  Rare (about one wave in fifty has an
    // ambiguous cell), but its float64 temporaries do not fit next to the 64 registers of the split spectra:
    // the wave parks half of them (pb: 8 KB) in its idle exchange slice for the duration.
    if ((OP_ABLATE & 8) == 0 && __ballot(amb != 0 || amb512) != 0ull) {
      float* park = reinterpret_cast<float*>(regions + wave * WAVE_CX_H) + lane;
      static_assert(64 * 32 * 4 <= WAVE_CX_H * 8, "parked registers must fit the wave's slice");
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        park[(2 * i) * 64] = OP_PB(i).x;
        park[(2 * i + 1) * 64] = OP_PB(i).y;
      }
      while (true) {
        const unsigned long long pending = __ballot(amb != 0 || amb512);
        if (pending == 0) break;
        const int src = __ffsll((long long)pending) - 1;
        const unsigned amb_s = (unsigned)__shfl((int)amb, src);
        const int q = amb_s ? (__ffs((int)amb_s) - 1) : 32;
        const int cs = src & 15, gs = src >> 4;
        const int f = q < 32 ? bin_of_entry(cs, q) : 512;
        const double Pe = op_exact_power(P, row, chunk, tq + gs, f, lane);
        const bool pass = Pe > s_t2d[q < 32 ? cs * 32 + q : 512];
        if (lane == src) {
          if (q < 32) {
            pred = (pred & ~(1u << q)) | ((pass ? 1u : 0u) << q);
            amb &= ~(1u << q);
          } else {
            pred512 = pass;
            amb512 = false;
          }
        }
      }
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        OP_PB(i).x = park[(2 * i) * 64];
        OP_PB(i).y = park[(2 * i + 1) * 64];
      }
      wave_lds_sync();
    }
    if (l0)  // entry -> register: e 0..7 -> 0..7, 8..23 -> 16..31, 24..30 -> 9..15, 31 -> 8
      pred = (pred & 0xffu) | ((pred & 0x00ffff00u) << 8) | ((pred >> 15) & 0xfe00u) | ((pred >> 23) & 0x100u);
    // Lane (g, c) holds the 32 decisions of frame g in ENTRY order; word m of the frame's bit row needs entry 2m (and
    // 16 + 2m, 2m + 1, 17 + 2m) of all 16 lanes.  A 16 x 16 bit transpose of both 16-bit halves at once -- four
    // xor-shuffle steps, each swapping the off-diagonal s x s blocks -- leaves in lane k: low half = entry k of lanes
    // 0..15, high half = entry 16 + k.  (32 wave ballots + per-lane selects did the same in ~200 instructions.)
    unsigned tr = pred;
    // (`up` = lanes whose column index has bit `sft` set: a compile-time lane mask -> SGPR-pair selects, sel_s of fastpath.hpp)
    auto tstep = [&](unsigned y, int sft, unsigned msk, unsigned long long up) {   // y = tr of lane ^ sft
      const unsigned ysh = sel_s(up, y >> sft, y << sft);
      const unsigned mk = sel_s(up, msk, ~msk);
      tr = (tr & ~mk) | (ysh & mk);
    };
    tstep((unsigned)op_xor_lanes<8>((int)tr), 8, 0x00ff00ffu, 0xff00ff00ff00ff00ull);
    tstep((unsigned)op_xor_lanes<4>((int)tr), 4, 0x0f0f0f0fu, 0xf0f0f0f0f0f0f0f0ull);
    tstep((unsigned)op_xor_lanes<2>((int)tr), 2, 0x33333333u, 0xccccccccccccccccull);
    tstep((unsigned)op_xor_lanes<1>((int)tr), 1, 0x55555555u, 0xaaaaaaaaaaaaaaaaull);
    const unsigned long long b8 = __ballot(pred512);
    {
      const int sh = 16 * g;
      const int srcl = (lane & 48) | ((2 * c) & 15);
      const unsigned wa = (unsigned)__shfl((int)tr, srcl), wb2 = (unsigned)__shfl((int)tr, srcl + 1);
      const unsigned f0 = wa & 0xffffu, f1 = wa >> 16, f2 = wb2 & 0xffffu, f3 = wb2 >> 16;
      const unsigned r1 = (((__brev(f1) >> 16) << 1) | (f1 & 1u)) & 0xffffu;
      const unsigned r3 = (((__brev(f3) >> 16) << 1) | (f3 & 1u)) & 0xffffu;
      myword = (unsigned long long)(f0 | (r1 << 16)) | ((unsigned long long)(f2 | (r3 << 16)) << 32);
      if (c == 8) myword = (b8 >> sh) & 1ull;
    }
  }

  OP_STAMP(5);   // decide (+ refinement) + transpose
  // ---- publish this tile's bits; the spectra stay in v[] ---------------------------------------------
  // (LATE ARGUMENTS, see the epilogue: what the middle of the kernel needs -- exchange buffer, epoch, error word, tables,
  // mask scale, smoothing width -- is read from the kernel-argument segment here, after the prologue's peak of live scalars)
  const op_late_t kpm = op_late_ptr();
  const unsigned m_ticket = (unsigned)__builtin_amdgcn_readfirstlane((int)s_misc[tk_slot]);
  const unsigned m_ntt = (unsigned)(OP_LATE(kpm, int, A.n_tiles) + 2);
  const int64_t m_u = m_ticket / m_ntt;
  const int m_jt = (int)(m_ticket % m_ntt) - 1;
  unsigned long long* const m_xbits = OP_LATE_PTR(kpm, unsigned long long*, xbits);
  const unsigned m_epoch = OP_LATE(kpm, unsigned, epoch);
  unsigned* const m_err = OP_LATE_PTR(kpm, unsigned*, err);
  const char* const m_tab = OP_LATE_PTR(kpm, const char*, tab);
  const float m_kscale = OP_LATE(kpm, float, A.kscale);
  const int m_nt = OP_LATE(kpm, int, nt);
  [[maybe_unused]] const float m_inv_ktot = OP_LATE(kpm, float, inv_ktot), m_prop = OP_LATE(kpm, float, prop);
  unsigned long long* xb_mine = m_xbits + ((size_t)m_u * m_ntt + (m_jt + 1)) * OP_TILE_WORDS;
  // data-tagged granules: every 8-byte store carries 32 mask bits and the launch epoch.  A consumer polls the
  // granules it needs until their tags are current: no separate flag, no drain of the stores, one write-through
  // and one read on the critical path instead of two of each.
  if (c < OP_XW) {
    const op_v4u gr = {(unsigned)myword, m_epoch, (unsigned)(myword >> 32), m_epoch};
    op_st16_sc1(&xb_mine[((4 * wave + g) * OP_XW + c) * 2], gr);
  }
  [[maybe_unused]] unsigned pend_halo = OP_SEAM_NONE;
  if constexpr (DEFER) {
    if (halo_tile) pend_halo = (unsigned)__builtin_amdgcn_readfirstlane((int)s_misc[0]);   // (read before, cleared after the barrier)
  }
  __syncthreads();   // every wave is past its forward exchange: the slices are idle from here
  if (halo_tile) {
    if constexpr (DEFER) {
      seam_close(pend_halo, tid);
      if (tid == 0) s_misc[0] = OP_SEAM_NONE;
    }
    if constexpr (PERSIST) {
      // a halo tile ends here: its next ticket is drawn on the spot (two tiles in 149 at the default chunking)
      if (tid == 0) s_misc[tk_slot ^ 1u] = op_draw_ticket_late(OP_LATE(kpm, unsigned long long, ticket)) - OP_LATE(kpm, unsigned, ticket_base);
      pf = false;
      // (defined on this path too: left alone, the registers of the samples staged at the loop top would stay live up to here)
#pragma unroll
      for (int k = 0; k < NQ; ++k) q[k] = 0.f;
#pragma unroll
      for (int k = 0; k < SCAN_REG; ++k) sc[k] = 0.f;
    }
    OP_DONE;
  }
  OP_STAMP(6);   // publish + barrier

  // ---- smoothing on the matrix cores (exact integer arithmetic, v_mfma_i32_16x16x32_i8) ----------------
  // The separable triangle filter is two small dense contractions per 16-bin block:
  //   H[row][bin]  = sum_k  bit[row][16 b - 8 + k] * vf[k - 8 - j]        (A = 16 rows x 32 bins of 0/1 bytes,
  //                                                                          B = 32 x 16 band matrix, constant)
  //   K[frame][bin] = sum_row vt[row - frame - m_nt] * H[row][bin]           (A = 16 frames x 32 row slots, constant,
  //                                                                          B = H as bytes: H <= (nf+1)^2 <= 81)
  // The first product's result layout (lane = bin column, 4 consecutive rows per lane group) IS the second
  // product's B layout once its k slots are numbered accordingly, so H never leaves the registers.  Row block 0
  // = the tile's OWN 16 rows: its H is computed before the neighbours' flags are polled (the hand-off latency
  // hides behind it); row blocks 1, 2 = the 2 m_nt neighbour rows.
  constexpr int WP = OP_XW + 2;        // one zero word on each side of every bit row
  constexpr int WPB = WP * 8;          // bytes per row
  constexpr int SLICE_B = WAVE_CX_H * 8;
  char* rbytes = reinterpret_cast<char*>(regions);
  unsigned long long* wb = reinterpret_cast<unsigned long long*>(rbytes + 4 * OP_KP * 2);  // tail of slice 0: 48 rows
  static_assert(4 * OP_KP * 2 + 48 * WPB <= SLICE_B, "bit rows must fit behind wave 0's K rows");
  const unsigned char* wbb = reinterpret_cast<const unsigned char*>(wb);
  if (c < OP_XW) wb[(m_nt + 4 * wave + g) * WP + 1 + c] = myword;
  for (int r = tid; r < 48; r += WAVES * 64) {
    wb[r * WP] = 0ull;
    wb[r * WP + WP - 1] = 0ull;
  }
  const int q4 = lane >> 4, j16 = lane & 15;
  const long Bf = (long)s_mc[lane], At1 = (long)s_mc[64 + lane], At2 = (long)s_mc[128 + lane];
  const bool three = 2 * m_nt > 16;      // a third row block (wave-uniform)
  // neighbour-list index m -> tile row: m < m_nt: row m (previous tile), else row m_nt + 16 + (m - m_nt) (next tile)
  const int m1 = j16, m2 = 16 + j16;
  const int r1 = m1 < 2 * m_nt ? (m1 < m_nt ? m1 : 16 + m1) : 0;
  const int r2 = m2 < 2 * m_nt ? (m2 < m_nt ? m2 : 16 + m2) : 0;
  __syncthreads();
  typedef int op_v4i __attribute__((ext_vector_type(4)));
  const op_v4i zero4 = {0, 0, 0, 0};
  unsigned hown[9];   // H of the own rows, 4 bytes per 16-bin block
  {
    const unsigned char* rp = wbb + (m_nt + j16) * WPB + 7 + q4;
#pragma unroll
    for (int nb = 0; nb < 9; ++nb) {
      const int b = wave + 4 * nb;
      hown[nb] = 0u;
      if (b < 33) {
        const long a = (long)s_exp[rp[2 * b]];
        const op_v4i h = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, Bf, zero4, 0, 0, 0);
        hown[nb] = (unsigned)h[0] | ((unsigned)h[1] << 8) | ((unsigned)h[2] << 16) | ((unsigned)h[3] << 24);
      }
    }
  }
  OP_STAMP(7);   // zero fill + barrier + own rows on the matrix cores
  // neighbour rows: one 16-byte load per 64-bit word (2 m_nt x 9 words <= 288: at most two per thread), polled
  // until both tags are current
  for (int i = tid; i < 2 * m_nt * OP_XW; i += WAVES * 64) {
    const int side = i >= m_nt * OP_XW;
    const int rem = i - side * m_nt * OP_XW;
    const int rr = rem / OP_XW, w = rem - rr * OP_XW;
    const unsigned long long* src = side ? xb_mine + OP_TILE_WORDS + (rr * OP_XW + w) * 2
                                         : xb_mine - OP_TILE_WORDS + ((NF - m_nt + rr) * OP_XW + w) * 2;
    op_v4u gr = op_ld16_sc1(src);
    for (int spin = 0; !(OP_ABLATE & 2) && (LOSE || gr[1] != m_epoch || gr[3] != m_epoch); ++spin) {
      if (LOSE || spin >= OP_SPIN_MAX) {   // every spin is bounded: report instead of hanging the device
        op_err_or(m_err, 1u);
        s_misc[1] = 1u;            // the tile's mask is unknown: every hop it finalises or hands on becomes NaN
        break;
      }
      op_poll_sleep();
      gr = op_ld16_sc1(src);
    }
    wb[(side ? m_nt + NF + rr : rr) * WP + 1 + w] = (unsigned long long)gr[0] | ((unsigned long long)gr[2] << 32);
  }
  __syncthreads();
  OP_STAMP(8);   // neighbours' bits (poll) + barrier
  // PERSIST: the next ticket.  Drawn only now -- this tile no longer waits for a tile with a HIGHER ticket -- and consumed at
  // the end of the smoothing stage: the atomic's round trip (~1.5 us) runs under the matrix-core work (a GLOBAL atomic and no
  // FLAT access pending: as flat_atomic_add wave 0's first MFMA of this stage waited vmcnt(0) for it -- op_draw_ticket_late)
  [[maybe_unused]] unsigned nx_raw = 0u;
  if constexpr (PERSIST) {
    if (tid == 0) nx_raw = op_draw_ticket_late(OP_LATE(kpm, unsigned long long, ticket));
  }
  {
    const unsigned char* rp1 = wbb + r1 * WPB + 7 + q4;
    const unsigned char* rp2 = wbb + r2 * WPB + 7 + q4;
#pragma unroll
    for (int nb = 0; nb < 9; ++nb) {
      const int b = wave + 4 * nb;
      if (b < 33) {
        const long a1 = (long)s_exp[rp1[2 * b]];
        const op_v4i h1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, Bf, zero4, 0, 0, 0);
        const unsigned p1 = (unsigned)h1[0] | ((unsigned)h1[1] << 8) | ((unsigned)h1[2] << 16) | ((unsigned)h1[3] << 24);
        const long bt1 = (long)(((unsigned long long)p1 << 32) | (unsigned long long)hown[nb]);
        op_v4i d = __builtin_amdgcn_mfma_i32_16x16x32_i8(At1, bt1, zero4, 0, 0, 0);
        if (three) {
          const long a2 = (long)s_exp[rp2[2 * b]];
          const op_v4i h2 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a2, Bf, zero4, 0, 0, 0);
          const unsigned p2 = (unsigned)h2[0] | ((unsigned)h2[1] << 8) | ((unsigned)h2[2] << 16) | ((unsigned)h2[3] << 24);
          d = __builtin_amdgcn_mfma_i32_16x16x32_i8(At2, (long)(unsigned long long)p2, d, 0, 0, 0);
        }
        // lane group q4 holds output frames 4 q4 .. 4 q4 + 3 = wave q4's frames: K rows live in THAT wave's slice
        unsigned short* kd = reinterpret_cast<unsigned short*>(rbytes + q4 * (SLICE_B + 64)) + 16 * b + j16;  // +64 B per slice: the four lane groups hit disjoint banks
        kd[0] = (unsigned short)d[0];
        kd[OP_KP] = (unsigned short)d[1];
        kd[2 * OP_KP] = (unsigned short)d[2];
        kd[3 * OP_KP] = (unsigned short)d[3];
      }
    }
  }
  if constexpr (PERSIST) {
    if (tid == 0) s_misc[tk_slot ^ 1u] = nx_raw - OP_LATE(kpm, unsigned, ticket_base);
  }
  __syncthreads();  // K of all 16 frames complete; from here every wave touches only its own slice
  OP_STAMP(9);   // smoothing on the matrix cores + barrier

  const unsigned short* kt = reinterpret_cast<const unsigned short*>(rbytes + wave * (SLICE_B + 64));
  // entry e of this lane = bin c + 32 e (e < 16) or (32 - c) + 32 (e - 16); lane 0 pairs its bins
  // differently (bin_of_entry): read where used, two 16-bit LDS loads per conjugate pair
  const unsigned short* krow = kt + g * OP_KP;
  const unsigned short* k_lo = krow + (c == 0 ? 0 : c);        // entries e < 16 of lanes c >= 1
  const unsigned short* k_hi = krow + (c == 0 ? 0 : 32 - c);   // entries e >= 16
  // PROP: weight of the valid taps along t for this lane group's frame (closed form of the triangle's tails)
  float tt = 0.f;
  if constexpr (PROP) {
    const int64_t tl_ = t < m_nt ? m_nt - t : 0, tr_ = (G.T - 1 - t) < m_nt ? m_nt - (G.T - 1 - t) : 0;
    tt = (float)((int64_t)(m_nt + 1) * (m_nt + 1) - tl_ * (tl_ + 1) / 2 - tr_ * (tr_ + 1) / 2);
  }
  const unsigned char* e_lo = s_ef + (c == 0 ? 0 : c);
  const unsigned char* e_hi = s_ef + (c == 0 ? 0 : 32 - c);
  // the float mask exactly as k_k16_to_mask writes it: p * (K / ktot) + (1 - p) * edge, edge = tf * tt / ktot
  auto mfull = [&](unsigned short kv, float tf) -> float {
    const float edge = tf * tt * m_inv_ktot;
    return m_prop * ((float)kv * m_inv_ktot) + (1.0f - m_prop) * edge;
  };
  const float k512 = PROP ? mfull(krow[512], (float)s_ef[512]) * m_kscale : (float)krow[512] * m_kscale;
  auto mval = [&](int q, float scale) -> float {
    const int b0 = bin_of_entry(0, q);                         // lane 0 (compile-time)
    const unsigned short* pl = q < 16 ? k_lo : k_hi;
    const int off = q < 16 ? 32 * q : 32 * (q - 16);
    const unsigned short kv = c == 0 ? krow[b0] : pl[off];
    if constexpr (PROP) {
      const float tf = (float)(c == 0 ? s_ef[b0] : (q < 16 ? e_lo : e_hi)[off]);
      return mfull(kv, tf) * scale;
    }
    return (float)kv * scale;
  };
  {
    // mask -> merge (the second half of pair_mask): Yk = X2[k] mk, Yn = conj-pair value x mn, then back to the
    // half-size complex spectrum.  The four 1/2 factors of split and merge ride in the mask scale.
    const float ks = m_kscale * 0.25f;
    auto sel = [&](cf a0, cf a1) -> cf { return {l0 ? a0.x : a1.x, l0 ? a0.y : a1.y}; };
    auto merge = [&](cf& xa, cf& xb, cf w, float mk, float mn) { merge_pair(xa, xb, w, mk, mn); };
    merge(pa[0], pb[0], wlo, mval(0, ks), mval(31, ks));
    cf z0, z8;
    {
      const float y0 = (raw0.x + raw0.y) * mval(0, m_kscale);
      const float yN = (raw0.x - raw0.y) * k512;
      z0 = {0.5f * (y0 + yN), 0.5f * (y0 - yN)};
      const float m8 = mval(31, m_kscale);  // entry 31 of lane 0 = bin 256
      z8 = {raw8.x * m8, raw8.y * m8};
    }
#pragma unroll
    for (int sl = 1; sl < 16; ++sl) {
      const cf w = mul_tw<false>(sl < 8 ? wlo : whi, twc<32>(sl), tws<32>(sl));
      merge(pa[sl], pb[sl], w, mval(sl, ks), mval(31 - sl, ks));
    }
    // scatter back: register i receives, for lanes >= 1, entry i; for lane 0, the entry that lives in register i
    v[0] = sel(z0, pa[0]);
#pragma unroll
    for (int i = 1; i < 8; ++i) v[i] = pa[i];
    v[8] = sel(z8, pa[8]);
#pragma unroll
    for (int i = 9; i < 16; ++i) v[i] = sel(pb[16 - i], pa[i]);
#pragma unroll
    for (int i = 16; i < 24; ++i) v[i] = sel(pa[i - 8], pb[31 - i]);
#pragma unroll
    for (int i = 24; i < 31; ++i) v[i] = sel(pb[39 - i], pb[31 - i]);
    v[31] = sel(pb[8], pb[0]);
  }
  wave_lds_sync();  // K tile consumed: the slice is reused by the inverse transform
  OP_STAMP(10);  // mask + merge

  // ---- inverse transform, synthesis window, wave-private overlap-add (k_apply_fast<LEAN>) -------------
  {
    // fresh address arithmetic for the inverse exchange: shared with the forward transform (CSE) the 16 row
    // addresses would stay live -- and be spilled -- across the whole smoothing phase
    int zi = 0, ci = c;
    asm volatile("" : "+v"(zi), "+v"(ci));
    fft512_inv_half(v, fb + zi, tw512 + zi, ci);
  }
  OP_STAMP(11);  // inverse transform
  float4 n4;   // 1 / window envelope of the lane's four samples of a hop
  auto load_n4 = [&]() { n4 = op_ldg4(&reinterpret_cast<const float*>(m_tab + OP_TAB_INVN)[(tid & 63) * 4]); };   // (a GLOBAL load: its wait is a partial vmcnt)
  if constexpr (PERSIST) load_n4();   // ahead of the prefetch: the epilogue's wait for it must not include the next tile's samples
  auto prefetch_next = [&]() {
    // ---- the NEXT tile's samples: loads issued here, consumed at the loop top (see PERSIST above) ----
    const OnePassArgs& Pn = *late_args<OnePassArgs>();
    const unsigned nx = (unsigned)__builtin_amdgcn_readfirstlane((int)s_misc[tk_slot ^ 1u]);
    pf = true;
    // (every path DEFINES q / sc: a conditional assignment would keep the previous tile's values alive -- 24 registers --
    // through a whole iteration)
    // q / sc are DEFINED on every path, each by one if / else (a conditional assignment -- or a flag the optimiser cannot
    // thread -- keeps the previous tile's values alive through a whole iteration, and the allocator then parks all 24
    // in scratch: a store that waits for the very load it was meant to hide)
    const bool n_live = nx < Pn.total_tiles;
    const unsigned n_tk = n_live ? nx : 0u;
    TileSrc N;
    {
      // the launch plan: an interior unit's tile is base + strides and two range compares, nothing of the view is read
      const OpTile nl = op_plan_tile(Pn.plan, n_tk);
      if (op_plan_blk_vec(Pn.plan, nl)) N = tile_src_plan(Pn.plan, nl);
      else N = tile_src(Pn, (int64_t)nl.row, Pn.plan.c0 + nl.k, nl.jt, true);
    }
    // NO BRANCH around the loads: at the join with a path that issued none the compiler has to assume the least number of loads
    // behind n4, and the epilogue's wait for n4 is vmcnt(0) again -- for the whole span.  A next tile that stages sample by
    // sample (a unit's edge, a halo tile: two in 149) or no tile at all never reads q / sc: its loads go to the constant
    // tables (19 x 256 floats from their start: inside OP_TAB_BYTES).
    static_assert(NQ * 256 * 4 <= OP_TAB_BYTES, "the stand-in loads stay inside the tables");
    const bool n_vec = n_live && N.blk_vec, n_scan = n_live && N.sc_base != nullptr;
    const float* const n_sp = n_vec ? N.sp : reinterpret_cast<const float*>(Pn.tab);
    const float* const n_sc = n_scan ? N.sc_base : n_sp;
    const int n_sc1 = n_scan ? N.sc_n1 : 0;
#pragma unroll
    for (int k = 0; k < NQ; ++k) q[k] = n_sp[tid + k * 256];
#pragma unroll
    for (int k = 0; k < SCAN_REG; ++k) sc[k] = n_sc[min(tid + k * WAVES * 64, n_sc1)];
  };
  // DEFERRED SEAM: the open seam's granules (the tile before it published them a whole tile ago) are loaded during the
  // overlap-add (behind all four quarters of it) and used at the end of the epilogue
  [[maybe_unused]] unsigned sm_pend = OP_SEAM_NONE;
  [[maybe_unused]] unsigned long long sm_g0 = 0ull, sm_g1 = 0ull, sm_g2 = 0ull, sm_g3 = 0ull;
  [[maybe_unused]] float* sm_dst = nullptr;
  [[maybe_unused]] float4 sm_lead = make_float4(0.f, 0.f, 0.f, 0.f);
  auto seam_issue = [&]() {
    sm_pend = (unsigned)__builtin_amdgcn_readfirstlane((int)s_misc[0]);   // (every wave reads it before the barrier; thread 0 rewrites it after)
    if (sm_pend != OP_SEAM_NONE && wave < 3) {
      const unsigned long long* sm_src;
      seam_where(sm_pend, sm_src, sm_dst);
      sm_src += seam_off(wave, (tid & 63) * 4);
      sm_g0 = __hip_atomic_load((const __attribute__((address_space(1))) unsigned long long*)(sm_src), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sm_g1 = __hip_atomic_load((const __attribute__((address_space(1))) unsigned long long*)(sm_src + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sm_g2 = __hip_atomic_load((const __attribute__((address_space(1))) unsigned long long*)(sm_src + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sm_g3 = __hip_atomic_load((const __attribute__((address_space(1))) unsigned long long*)(sm_src + 3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      sm_lead = op_ldg4(sm_dst + seam_off(wave, (tid & 63) * 4));
    }
  };
  float* acc = reinterpret_cast<float*>(regions + wave * WAVE_CX_H);
  {
    const float2* wsrc2 = reinterpret_cast<const float2*>(swin + 2 * c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // (first contribution to hop g + j -- j == 0, or frame g == 3 -- is a plain store; sel_s: fastpath.hpp)
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int r = 8 * j + rr;
        float2* dst = reinterpret_cast<float2*>(acc + (g + j) * HPITCH + 2 * c + 32 * rr);
        const float2 ws = wsrc2[16 * r];
        float2 nw = {v[r].x * ws.x, v[r].y * ws.y};
        if (j != 0) {
          const float2 old = *dst;
          nw.x = sel_s(OLA_KEEP, nw.x + old.x, nw.x);
          nw.y = sel_s(OLA_KEEP, nw.y + old.y, nw.y);
        }
        *dst = nw;
      }
      wave_lds_sync();
      // the prefetch after two quarters of the overlap-add, the open seam's loads behind all four (profiles/onepass_chain.txt)
      if constexpr (PERSIST) { if (j + 1 == 2) prefetch_next(); }
      if constexpr (DEFER) { if (j + 1 == 4) seam_issue(); }
    }
  }
  if constexpr (!PERSIST) load_n4();
  __syncthreads();
  OP_STAMP(12);  // window + wave-private overlap-add + barrier
#if OP_TRACE
  if (lane == 0) t_slot_[15] = 1u;
#endif

  // ---- cross-wave combine, normalise, store (seam mode: abutting tiles) -------------------------------
  // LATE ARGUMENTS (round 5).  The output map, hop range, seam buffer and the tile's coordinates are only needed from here
  // on, but as ordinary kernel arguments they are loaded in the entry block and stay live through every phase: the
  // kernel ran out of scalar registers and parked them in VGPR lanes (v_writelane / 329 v_readlane -- each a 4-cycle slot
  // of the vector pipe, the kernel's binding resource: profiles/r05_valu_classes.txt).  Here they are read again from the
  // kernel-argument segment through an OPAQUE pointer (scalar loads, off the vector pipe; not mergeable with the entry
  // block's loads), and the tile's coordinates are recomputed from the ticket, which is still in LDS.
  const op_late_t kp4 = op_late_ptr();
  const int64_t e_gstep = OP_LATE(kp4, int64_t, A.om.g_step), e_p0 = OP_LATE(kp4, int64_t, A.om.p0), e_p1 = OP_LATE(kp4, int64_t, A.om.p1);
  void* const e_out = OP_LATE_PTR(kp4, void*, A.om.out);
  const int64_t e_ostride = OP_LATE(kp4, int64_t, A.om.stride), e_g0 = OP_LATE(kp4, int64_t, A.om.g0), e_glo = OP_LATE(kp4, int64_t, A.om.g_lo),
                e_ghi = OP_LATE(kp4, int64_t, A.om.g_hi);
  const int e_odtype = OP_LATE(kp4, int, A.om.dtype), e_normalize = OP_LATE(kp4, int, A.normalize), e_ntiles = OP_LATE(kp4, int, A.n_tiles);
  const int64_t e_hbegin = OP_LATE(kp4, int64_t, A.h_begin), e_hend = OP_LATE(kp4, int64_t, A.h_end);
  unsigned long long* const e_part2 = OP_LATE_PTR(kp4, unsigned long long*, part2);
  const unsigned e_epoch = OP_LATE(kp4, unsigned, epoch);
  unsigned* const e_err = OP_LATE_PTR(kp4, unsigned*, err);
  const char* const e_tab = OP_LATE_PTR(kp4, const char*, tab);
  const int e_padL = OP_LATE(kp4, int32_t, A.g.padL);
  const int64_t e_T = OP_LATE(kp4, int64_t, A.g.T), e_Lout = OP_LATE(kp4, int64_t, A.g.Lout);
  const unsigned e_ticket = (unsigned)__builtin_amdgcn_readfirstlane((int)s_misc[tk_slot]);
  constexpr bool PLAN16 = PERSIST;   // the epilogue takes its coordinates from the launch plan
  [[maybe_unused]] const OpPlan& e_plan = *reinterpret_cast<const OpPlan*>((const char*)kp4 + __builtin_offsetof(OnePassArgs, plan));
  [[maybe_unused]] OpTile el{};
  int64_t e_u, e_row, e_chunk;
  int e_jt;
  if constexpr (PLAN16) {
    el = op_plan_tile(e_plan, e_ticket);
    e_u = el.u;
    e_jt = el.jt;
    e_row = el.row;
    e_chunk = e_plan.c0 + el.k;
  } else {
    const unsigned e_ntt = (unsigned)(e_ntiles + 2);
    e_u = e_ticket / e_ntt;
    e_jt = (int)(e_ticket % e_ntt) - 1;
    const unsigned e_gu = (unsigned)(OP_LATE(kp4, int64_t, A.view.unit0) + e_u), e_nch = (unsigned)OP_LATE(kp4, int32_t, A.view.n_chunks);
    e_row = e_gu / e_nch;
    e_chunk = OP_LATE(kp4, int64_t, A.view.c0) + e_gu % e_nch;
  }
  const int64_t e_tf = e_hbegin - 3 + (int64_t)e_jt * NF;
  const float* fr = reinterpret_cast<const float*>(regions);
  const int s4 = (tid & 63) * 4;
  // A lost hand-off must not look like audio: a tile whose neighbour bits never arrived writes NaN to every hop it
  // finalises and publishes NaN partials (the next tile's straddling hops inherit them); a tile whose predecessor's
  // partial hops never arrived writes NaN to those three hops.  The error word still reports it (sg_check_errors).
  // (a scalar select: as a vector one its NaN constant is hoisted out of the tile loop into a register of its own)
  unsigned poison_u = __builtin_amdgcn_readfirstlane((int)s_misc[1]) != 0 ? 0x7fc00000u : 0u;
  asm volatile("" : "+s"(poison_u));
  const float poison = __uint_as_float(poison_u);
  // Hops that straddle two tiles: tile j publishes its three TRAILING partial hops (un-normalised sums) the
  // same way as the mask bits (write-through stores, drained, epoch flag per hop); tile j+1 adds its LEADING
  // partials and finalises them.  Per wave: trailing hop first (published early), interior hops, leading hop
  // last (tile j, one ticket earlier, has usually published by then).  Publishing never waits: no cycles.
  // Interior tiles (every hop inside the output range, all four frames of each hop present, float32 output,
  // aligned rows): straight-line version of the loop below, same sums in the same order.
  {
    const int64_t pb0 = e_tf * 256 - e_padL;
    const int64_t gi00 = e_chunk * e_gstep + (pb0 - e_p0);
    float* dbase;
    bool tile_fast = false;
    if constexpr (PLAN16) {
      // an interior unit's tile inside the plan's range: the flag is one compare, the address base + strides -- none of the
      // output map's fields is waited for (they serve the tiles below: a unit's edge, another sample type, unaligned rows)
      tile_fast = op_plan_tile_fast(e_plan, el);
    }
    if (tile_fast) {
      dbase = (float*)(__attribute__((address_space(1))) float*)(uintptr_t)e_plan.dst + op_plan_dst_off(e_plan, el);
    } else {
      dbase = (float*)e_out + (e_row * e_ostride + gi00 - e_g0);
      tile_fast = e_odtype == 0 && e_normalize && e_tf >= 3 && e_tf + NF + 2 < e_T &&
                  e_tf >= e_hbegin && e_tf + NF + 2 < e_hend && pb0 >= e_p0 &&
                  pb0 + NF * 256 <= e_p1 && pb0 + NF * 256 <= e_Lout && gi00 >= e_glo &&
                  gi00 + NF * 256 <= e_ghi && (reinterpret_cast<uintptr_t>(dbase) & 15) == 0 && WAVES == 4;
    }
    float* dst0 = dbase + s4;
    if (tile_fast) {
      constexpr int R = WAVE_CX_H * 2;
      auto ld4 = [&](int off) { return *reinterpret_cast<const float4*>(&fr[off + s4]); };
      auto fin = [&](float4 a, int jj) {
        a.x = (a.x + poison) * n4.x; a.y = (a.y + poison) * n4.y; a.z = (a.z + poison) * n4.z; a.w = (a.w + poison) * n4.w;
        op_stg4(dst0 + jj * 256, a);
      };
      if (wave == 3) {
#pragma unroll
        for (int it = 0; it < 4; ++it) fin(ld4(it * R + 3 * HPITCH), 3 + 4 * it);
        OP_STAMP(13);
        OP_DONE;
      }
      {
        const float4 a4 = ld4((WAVES - 1) * R + (wave + 4) * HPITCH);
        unsigned long long* dst = e_part2 + (((size_t)e_u * e_ntiles + e_jt) * 3 + wave) * 256 + s4;
        const op_v4u ga = {__float_as_uint(a4.x + poison), e_epoch, __float_as_uint(a4.y + poison), e_epoch};
        const op_v4u gb = {__float_as_uint(a4.z + poison), e_epoch, __float_as_uint(a4.w + poison), e_epoch};
        op_st16_sc1(dst, ga);
        op_st16_sc1(dst + 2, gb);
      }
#pragma unroll
      for (int it = 1; it < 4; ++it) {
        float4 a4 = ld4((it - 1) * R + (wave + 4) * HPITCH);
        const float4 f4 = ld4(it * R + wave * HPITCH);
        a4.x += f4.x; a4.y += f4.y; a4.z += f4.z; a4.w += f4.w;
        fin(a4, wave + 4 * it);
      }
      if constexpr (DEFER) {
        // the seam left open one tile ago is finished, this tile's stays open
        if (sm_pend != OP_SEAM_NONE) seam_finish(sm_pend, wave, s4, sm_g0, sm_g1, sm_g2, sm_g3, sm_dst, sm_lead, n4);
        op_stg4(dst0 + wave * 256, ld4(wave * HPITCH));
        if (tid == 0) s_misc[0] = e_ticket | (s_misc[1] != 0u ? 0x80000000u : 0u);
      } else {
        float4 a4 = ld4(wave * HPITCH);
        const unsigned long long* src = e_part2 + (((size_t)e_u * e_ntiles + e_jt - 1) * 3 + wave) * 256 + s4;
        op_v4u ga, gb;
        for (int spin = 0;; ++spin) {
          asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                       : "=&v"(ga), "=&v"(gb) : "v"(src) : "memory");
          const unsigned e = e_epoch;
          if ((OP_ABLATE & 16) || (!LOSE && ga[1] == e && ga[3] == e && gb[1] == e && gb[3] == e)) break;
          if (LOSE || spin >= OP_SPIN_MAX) {
            op_err_or(e_err, 2u);
            ga[0] = ga[2] = gb[0] = gb[2] = op_nan_bits();   // the previous tile's share is unknown: NaN, not a partial sum
            break;
          }
          op_poll_sleep();
        }
        a4.x = __uint_as_float(ga[0]) + a4.x;
        a4.y = __uint_as_float(ga[2]) + a4.y;
        a4.z = __uint_as_float(gb[0]) + a4.z;
        a4.w = __uint_as_float(gb[2]) + a4.w;
        fin(a4, wave);
      }
      OP_STAMP(13);  // cross-wave combine, hand-off of the straddling hops, stores
      OP_DONE;
    }
  }
  if constexpr (DEFER) {
    // not a tile_fast tile (a unit's edge, an unaligned row): it keeps the immediate protocol, an open seam is closed first
    if (sm_pend != OP_SEAM_NONE && wave < 3) seam_finish(sm_pend, wave, s4, sm_g0, sm_g1, sm_g2, sm_g3, sm_dst, sm_lead, n4);
    if (tid == 0) s_misc[0] = OP_SEAM_NONE;
  }
  for (int it = 0; it < 5; ++it) {
    const int jj = wave < 3 ? (it == 0 ? NF + wave : (it == 4 ? wave : wave + 4 * it)) : (it < 4 ? 3 + 4 * it : -1);
    if (jj < 0) break;
    const int64_t h = e_tf + jj;
    if (h >= e_hend || h < e_hbegin) continue;
    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
    bool all_valid = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t ti = e_tf + jj - q;
      if (ti < 0 || ti >= e_T) all_valid = false;
    }
    {
      const int wh = jj >> 2, lh = jj & 3;
      if (wh >= 1 && wh - 1 < WAVES && lh <= 2) {
        a4 = *reinterpret_cast<const float4*>(&fr[(wh - 1) * WAVE_CX_H * 2 + (lh + 4) * HPITCH + s4]);
      }
      if (wh < WAVES) {
        const float4 f4 = *reinterpret_cast<const float4*>(&fr[wh * WAVE_CX_H * 2 + lh * HPITCH + s4]);
        a4.x += f4.x; a4.y += f4.y; a4.z += f4.z; a4.w += f4.w;
      }
    }
    if (jj >= NF) {
      // trailing partial hop -> tagged granules {float, epoch}
      const int k = jj - NF;
      unsigned long long* dst = e_part2 + (((size_t)e_u * e_ntiles + e_jt) * 3 + k) * 256 + s4;
      const op_v4u ga = {__float_as_uint(a4.x + poison), e_epoch, __float_as_uint(a4.y + poison), e_epoch};
      const op_v4u gb = {__float_as_uint(a4.z + poison), e_epoch, __float_as_uint(a4.w + poison), e_epoch};
      op_st16_sc1(dst, ga);
      op_st16_sc1(dst + 2, gb);
      continue;
    }
    if (jj < 3) {
      // h >= h_begin implies e_jt >= 1: the previous tile exists
      const unsigned long long* src = e_part2 + (((size_t)e_u * e_ntiles + e_jt - 1) * 3 + jj) * 256 + s4;
      op_v4u ga, gb;
      for (int spin = 0;; ++spin) {
        asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %2, off offset:16 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(ga), "=&v"(gb) : "v"(src) : "memory");
        const unsigned e = e_epoch;
        if ((OP_ABLATE & 16) || (!LOSE && ga[1] == e && ga[3] == e && gb[1] == e && gb[3] == e)) break;
        if (LOSE || spin >= OP_SPIN_MAX) {
          op_err_or(e_err, 2u);
          ga[0] = ga[2] = gb[0] = gb[2] = op_nan_bits();
          break;
        }
        op_poll_sleep();
      }
      // trailing partial of the previous tile + leading partial of this one (the order k_ola_seam adds them in)
      a4.x = __uint_as_float(ga[0]) + a4.x;
      a4.y = __uint_as_float(ga[2]) + a4.y;
      a4.z = __uint_as_float(gb[0]) + a4.z;
      a4.w = __uint_as_float(gb[2]) + a4.w;
    }
    a4.x += poison; a4.y += poison; a4.z += poison; a4.w += poison;
    if (!e_normalize) {
    } else if (all_valid) {
      a4.x *= n4.x; a4.y *= n4.y; a4.z *= n4.z; a4.w *= n4.w;
    } else {
      float4 nrm = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t ti = h - q;
        if (ti >= 0 && ti < e_T) {
          const float4 w4 = *reinterpret_cast<const float4*>(&reinterpret_cast<const float*>(e_tab + OP_TAB_WSQ)[256 * q + s4]);
          nrm.x += w4.x; nrm.y += w4.y; nrm.z += w4.z; nrm.w += w4.w;
        }
      }
      a4.x /= (nrm.x > 1e-10f ? nrm.x : 1.f);
      a4.y /= (nrm.y > 1e-10f ? nrm.y : 1.f);
      a4.z /= (nrm.z > 1e-10f ? nrm.z : 1.f);
      a4.w /= (nrm.w > 1e-10f ? nrm.w : 1.f);
    }
    {
      const int64_t pb = h * 256 - e_padL;
      const int64_t gi0 = e_chunk * e_gstep + (pb - e_p0);
      if (e_odtype == 0 && pb >= e_p0 && pb + 256 <= e_p1 && pb + 256 <= e_Lout && gi0 >= e_glo &&
          gi0 + 256 <= e_ghi) {
        float* dst = (float*)e_out + (e_row * e_ostride + gi0 - e_g0 + s4);
        if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
          *reinterpret_cast<float4*>(dst) = a4;
          continue;
        }
      }
    }
    const float vals[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t p = h * 256 + s4 + e - e_padL;
      if (p < e_p0 || p >= e_p1) continue;
      const int64_t gi = e_chunk * e_gstep + (p - e_p0);
      if (gi < e_glo || gi >= e_ghi) continue;
      store_sample(e_out, e_odtype, e_row * e_ostride + gi - e_g0, p < e_Lout ? vals[e] : 0.f);
    }
  }
  }   // tile loop (one iteration unless PERSIST)
