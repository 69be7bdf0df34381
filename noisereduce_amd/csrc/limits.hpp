// Tile sizes, table offsets and LDS-size rules that both a kernel header and a host-only unit read (create.hip sizes
// tables by them, debug.hip reads fields laid out by them).  Holds no kernels; the kernel header that owns each block
// includes this file.
#pragma once
#include <hip/hip_runtime.h>

namespace sg {

// ---- fused.hpp: k_smooth_bits2 ----
constexpr int SM2_TT = 64;
constexpr int SM2_THREADS = 576;
// (round 5) tallest tile tried for a row of F bins: short rows take tall tiles (fewer halo rows per output -- the time
// half-width of n_fft = 256 at 48 kHz is 37 frames: 64-frame tiles ran phase 1 over 2.2 x the rows) and split them into
// segments for phase 2
__host__ __device__ inline int smooth2_tt_max(int F) { return F <= 160 ? 256 : (F <= 320 ? 128 : SM2_TT); }
__host__ __device__ inline int smooth2_pitch(int F) { return ((F + 3) & ~3) + 4 * ((F + 31) / 32) + 4; }
__host__ __device__ inline size_t smooth2_cf_bytes(int rows, int F, int ct_size) {
  size_t b = (size_t)rows * smooth2_pitch(F) * ct_size;
  return (b + 15) & ~(size_t)15;
}

namespace fast {

// ---- onepass.hpp: the n_fft = 1024 one-pass gate ----
constexpr int OP_XW = 9;                 // 64-bit words per frame row (513 bins)
constexpr int OP_TILE_WORDS = 16 * OP_XW * 2;  // payload of one tile: 288 tagged granules = 2304 B (18 x 128 B)
constexpr int OP_MAX_NT = 16;            // neighbours hold 16 frames each
constexpr int OP_KP = 528;               // K row pitch (uint16 entries) of a wave's private K tile
// The kernel's nine constant tables live in ONE device buffer at fixed offsets (OnePassArgs::tab): one base pointer in the
// kernel arguments instead of nine -- 16 scalar registers fewer in a kernel that spilled 44 of them.
constexpr int OP_TAB_WIN = 0, OP_TAB_WSQ = 4096, OP_TAB_INVN = 8192, OP_TAB_TW512 = 9216, OP_TAB_TW1024 = 13312,
              OP_TAB_WIN64 = 17408, OP_TAB_TW64 = 25600, OP_TAB_MCONST = 33792, OP_TAB_EXP8 = 35328, OP_TAB_BYTES = 37376;

// ---- rowgate.hpp: the row gate's tile ----
constexpr int RG_PP = 528;               // float pitch of the power tile: rows 4w+g of a wave land on disjoint bank quarters

}  // namespace fast
}  // namespace sg
