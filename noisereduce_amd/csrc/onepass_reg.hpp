// The tile scaffold shared by the one-pass stationary gates of the register-transform geometries: k_gate_onepass512
// (onepass512.hpp), k_gate_onepass256 (onepass256.hpp) and k_gate_onepass2048 (onepass2048.hpp).
//
// A workgroup takes a TICKET and owns one tile of NF consecutive frames of one unit.  After the forward transform it decides
// its NF x F cells, keeps the spectra in registers and
//   1. publishes the tile's bits (NF rows x XW words) to its neighbours as data-tagged granules {32 bits, launch epoch};
//   2. polls the nt adjacent rows of tiles j - 1 and j + 1 (nt: the time half-width of the smoothing filter);
//   3. smooths the (NF + 2 nt) x F bit tile with the exact integer separable triangle filter on the matrix cores; bits and the
//      K tile (uint16) live in the exchange slices, which are idle between the two transforms;
// then x mask -> inverse transform -> window -> overlap-add -> store (finish_hop, fastpath.hpp).  The bits are the only exchange
// INSIDE the launch.  Inter-workgroup protocol, deadlock freedom (tickets; publish before wait), bounded polls and the
// NaN-poisoned output of a tile that lost a hand-off: onepass.hpp.  The -top_db floor test runs on the staged samples
// (thresh.hpp: FloorLazy); REDO = the second launch for the units whose test fired.
//
// Here: what is the same text at every geometry -- the tile's identity, the floor test over the padding no tile stages, the bit
// rows' margins and the neighbours' rows, the K rows of an MFMA result.  Decide and pack differ from geometry to geometry but not
// between a geometry's two-pass and one-pass kernels: fN_decide_pack in fast512.hpp / fast256.hpp / fast2048.hpp, one text for both
// (here with PARK: half of the spectra wait in the wave's slice during the exact re-evaluation, fastpath.hpp).  The MFMA shapes, the
// merge and the wave-private overlap-add are in the kernels.
#pragma once
#include "fastpath.hpp"

namespace sg {
namespace fast {

typedef int reg_v4i __attribute__((ext_vector_type(4)));

// The ticket of this workgroup into s_misc[0] (read it after the next barrier); s_misc[1]: "lost a hand-off", cleared.
__device__ __forceinline__ void reg_draw_ticket(const OnePassRegArgs& P, unsigned* s_misc, int tid) {
  if (tid == 0) {
    s_misc[0] = atomicAdd(P.ticket, 1u) - P.ticket_base;
    s_misc[1] = 0u;
  }
}

// Which tile a ticket is: n_tiles + 2 tickets per unit, one decide-only halo tile on each side of the unit's own.
// reg_tile_of ALSO STORES: the workgroup that drew ticket 0 of a first launch zeroes P.ticket[8], the counter the REDO launch
// draws from (thread 0, global memory).
struct RegTile : RegUnit {   // + row, chunk, lazy, need, floor_live (fastpath.hpp: reg_unit_of)
  int ntt;           // tiles per unit incl. the two halo tiles
  int64_t u;         // unit of this launch
  int jt;            // tile of the unit, -1 and n_tiles: the halo tiles
  bool halo_tile;
};
template <bool REDO>
__device__ __forceinline__ RegTile reg_tile_of(const OnePassRegArgs& P, unsigned ticket, int tid) {
  const unsigned ntt = (unsigned)(P.n_tiles + 2);
  RegTile W{reg_unit_of<REDO>(P.A, ticket / ntt)};
  W.ntt = (int)ntt;
  W.u = ticket / ntt;
  W.jt = (int)(ticket % ntt) - 1;
  W.halo_tile = W.jt < 0 || W.jt >= P.n_tiles;
  if (!REDO && W.lazy && ticket == 0u && tid == 0) P.ticket[8] = 0u;   // (the second launch's counter starts from zero)
  return W;
}

// Floor test, the part no tile stages.  The tiles of a unit stage the frames its kept hops need (+- nt), not the whole window:
// the rest -- the chunk's padding beyond them, A = [s_lo, first span) and B = [last span's end, s_hi) -- is dealt to the unit's
// tiles in slices of scan_q samples of A ++ B (onepass.hpp "floor test"; a few hundred samples per tile at the default chunking).
// step: frames from one tile to the next.
template <int THREADS, int H, int NF>
__device__ __forceinline__ void floor_scan_padding(const RegArgs& A, const OnePassRegArgs& P, int64_t row, int64_t chunk, int jt,
                                                   int step, int tid, unsigned& fl_mx) {
  constexpr int SPAN = (NF - 1 + 4) * H;
  const int64_t g0 = chunk * A.view.cs - A.view.pad;
  const int64_t s_lo = max<int64_t>(0, A.view.lo - g0), s_hi = min<int64_t>(A.view.Lp, A.view.hi - g0);
  const int64_t sp0 = (A.h_begin - 3 - step) * H - A.g.padL;
  const int64_t sp1 = (A.h_begin - 3 + (int64_t)P.n_tiles * step) * H - A.g.padL + SPAN;
  const int64_t first = min(s_hi, max(s_lo, sp0)), last = max(s_lo, min(s_hi, sp1));
  const int64_t lenA = first - s_lo;
  const int64_t c0 = (int64_t)(jt + 1) * P.scan_q, c1 = min(c0 + P.scan_q, lenA + (s_hi - last));
  for (int64_t i = c0 + tid; i < c1; i += THREADS)
    fl_mx = max(fl_mx, __float_as_uint((float)view_sample(A.view, row, chunk, i < lenA ? s_lo + i : last + (i - lenA))) & 0x7fffffffu);
}

// Bit rows in LDS, brow[ROWS][XW + 2]: one zero word on each side of a row, and zero rows past the neighbours' (the last
// k-block of the time product reads them).
template <int NF, int XW, int ROWS, int THREADS>
__device__ __forceinline__ void zero_bit_row_margins(unsigned long long* brow, int nt, int tid) {
  constexpr int BW = XW + 2;
  for (int r = tid; r < ROWS; r += THREADS) {
    brow[r * BW] = 0ull;
    brow[r * BW + BW - 1] = 0ull;
    if (r >= NF + 2 * nt) {
#pragma unroll
      for (int w = 1; w <= XW; ++w) brow[r * BW + w] = 0ull;
    }
  }
}

// Neighbour rows into brow: one 16-byte load per 64-bit word (2 nt x XW words), polled until both tags are current.  Tile j - 1
// holds frames tf0 - step ..: frame tf0 - nt + rr is its row step - nt + rr; tile j + 1: frame tf0 + NF + rr is its row
// NF - step + rr.  xb_mine: this tile's published rows.
template <int NF, int XW, int BW, int THREADS>
__device__ __forceinline__ void poll_neighbour_rows(const unsigned long long* xb_mine, int step, int nt, const OnePassRegArgs& P,
                                                    unsigned* s_misc, unsigned long long* brow, int tid) {
  constexpr int TILE_WORDS = NF * XW * 2;
  for (int i = tid; i < 2 * nt * XW; i += THREADS) {
    const int side = i >= nt * XW;
    const int rem = i - side * nt * XW;
    const int rr = rem / XW, w = rem - rr * XW;
    const unsigned long long* src = side ? xb_mine + TILE_WORDS + ((NF - step + rr) * XW + w) * 2
                                         : xb_mine - TILE_WORDS + ((step - nt + rr) * XW + w) * 2;
    op_v4u gr = op_ld16_sc1(src);
    for (int spin = 0; gr[1] != P.poll_epoch || gr[3] != P.poll_epoch; ++spin) {
      if (spin >= P.spin_max) {   // bounded: report instead of hanging the device
        atomicOr_system(P.err, 1u);
        s_misc[1] = 1u;            // the tile's mask is unknown: every hop it touches becomes NaN
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      gr = op_ld16_sc1(src);
    }
    brow[(side ? nt + NF + rr : rr) * BW + 1 + w] = (unsigned long long)gr[0] | ((unsigned long long)gr[2] << 32);
  }
}

// The four K rows of an MFMA result (a lane group holds 4 consecutive output frames of one bin column)
__device__ __forceinline__ void store_k4(unsigned short* kd, int KP, reg_v4i d) {
  kd[0] = (unsigned short)d[0];
  kd[KP] = (unsigned short)d[1];
  kd[2 * KP] = (unsigned short)d[2];
  kd[3 * KP] = (unsigned short)d[3];
}

}  // namespace fast
}  // namespace sg
