// One-pass stationary gate for n_fft = win = 2048, hop = 512 (round 6).
//
//   k_decide_fast2048 + k_smooth_bits2 + k_apply_fast2048<K> + k_ola_seam<512, 8>   ->   k_gate_onepass2048 + k_ola_seam<512, 8>
//
// The tile scaffold is onepass_reg.hpp / fastpath.hpp (store_partial_hop, finish_hop), shared with onepass512.hpp and
// onepass256.hpp.  This file's own:
//   * the tile: 8 frames (4 wavefronts x 2), one real frame per 32 lanes on the transforms of fast2048.hpp, 1025 bins = 17 bit
//     words per frame; decisions in the partner-lane form of k_decide_fast2048, packed with ballots.  Tiles always ABUT, as
//     k_apply_fast2048's (overlapping by 3 frames would redo 3 of every 8 transforms): the 3 hops that straddle two tiles leave
//     as partial sums and k_ola_seam (fastpath.hpp) combines them -- there is no overlapping form, the tile step is NF;
//   * the integer smoothing on the matrix cores, with two differences from the 512 / 256 kernels:
//       - the frequency half-width is 10 bins at 48 kHz, 23 at 22.05 kHz (base.py:100: 500 Hz / (sr / 1024)): a 16-bin output
//         block reads 16 + 2 nf <= 64 bins = TWO 32-bin k-blocks (band matrices Bf_lo: bins 16 b - 24 .., Bf_hi: bins 16 b + 8 ..),
//         nf <= 24;
//       - H = bits x band reaches (nf + 1)^2 = 576 > 127 (the int8 range of the second product's operand): it enters the time
//         product as two base-128 digits, K = At x (H & 127) + 128 At x (H >> 7)   (exact: integers).
//     8 + 2 nt <= 32 bit rows (nt <= 8) = two 16-row blocks = ONE k-block of the time product.  Six MFMAs per bin block, 65 blocks.
//   * the K tile (8 x 1025 uint16) and the bits live in the exchange slices, idle between the transforms; the pair stage reads its
//     mask entries straight from there (k_apply_fast2048<K> reads them from HBM), one barrier before the inverse exchange; the
//     overlap-add runs over the whole workgroup's hop buffer in four ordered rounds.
#pragma once
#include "fast2048.hpp"
#include "onepass_reg.hpp"

namespace sg {
namespace fast {

constexpr int O20_NF = 8;                             // frames per tile = tile step
constexpr int O20_XW = 17;                            // 64-bit words per bit row (1025 bins)
constexpr int O20_TILE_WORDS = O20_NF * O20_XW * 2;   // payload of one tile: 272 tagged 8-byte halves = 2176 B
constexpr int O20_BW = O20_XW + 2;                    // bit row pitch in LDS: one zero word on each side
constexpr int O20_ROWS = 32;                          // bit rows in LDS: two 16-row blocks (8 + 2 nt <= 24)
constexpr int O20_KP = 1048;                          // K row pitch (entries): 65 blocks of 16 bins + 8 (rows 4 apart: 16 banks apart)
constexpr int O20_MAX_NT = 8;
constexpr int O20_MAX_NF = 24;
// constant operands (device table `tab`, 64-bit entries): [0, 64) Bf_lo, [64, 128) Bf_hi, [128, 192) At, [192, 448) byte ->
// eight 0 / 1 bytes

#ifndef O20_OCC
#define O20_OCC 3
#endif
template <int WAVES, bool REDO = false>
__global__ __launch_bounds__(WAVES * 64, O20_OCC) void k_gate_onepass2048(OnePassRegArgs P) {
  static_assert(WAVES == 4, "tile = 8 frames");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf* tw = reinterpret_cast<cf*>(smem);                 // [32][32] w_1024^(k1 c)
  cf* regions = tw + 1024;
  float* s_t2 = reinterpret_cast<float*>(regions + WAVES * WAVE_CX_H);   // [1025] compare constants x4
  unsigned* s_misc = reinterpret_cast<unsigned*>(s_t2 + 1028);           // [0] ticket, [1] lost hand-off
  unsigned long long* s_exp = reinterpret_cast<unsigned long long*>(s_misc + 4);   // [256] byte -> eight 0 / 1 bytes
  const RegArgs& A = P.A;
  if (REDO && A.fl.alim[1] != A.tc.need_tag) return;   // no unit of this call reported (the common case)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5, c = lane & 31;
  const Geom& G = A.g;
  reg_draw_ticket(P, s_misc, tid);
  s_exp[tid] = P.tab[192 + tid];
  const unsigned fl_bound = REDO ? 0xffffffffu : floor_lazy_bound(A.fl, lane);
  __syncthreads();
  const RegTile W = reg_tile_of<REDO>(P, s_misc[0], tid);   // (ticket 0 of a first launch: also zeroes the REDO launch's counter)
  if (REDO && W.need == 0) return;   // whole workgroup
  const int64_t u = W.u, row = W.row, chunk = W.chunk;
  const int jt = W.jt, need = W.need;
  const bool floor_live = W.floor_live;
  stage_t2_plain<WAVES * 64, F20_F>(s_t2, A.tc.T2, need, 4.0, tid,
                                 [&](int f) { return t2_effective(A.tc, u, G.FS, f, need, floor_live, A.mag_scale, A.top_db); });
  constexpr int NF = O20_NF;
  const int64_t tf0 = A.h_begin - 3 + (int64_t)jt * NF;   // first frame of the tile
  cf v[32];
  bool valid;
  unsigned fl_mx = f20_gather<WAVES, true>(A, tw, regions, row, chunk, tf0, v, valid);
  if (!REDO && W.lazy) floor_scan_padding<WAVES * 64, F20_H, NF>(A, P, row, chunk, jt, NF, tid, fl_mx);   // the padding no tile stages
  if (!REDO) floor_lazy_report(A.tc, A.fl, fl_bound, fl_mx, u, G.FS, lane);
  const int64_t tq = tf0 + 2 * wave;
  // ---- forward transform + decisions (fast2048.hpp: f20_decide_pack) ------------------------------------------------------
  cf* fb = regions + wave * WAVE_CX_H + g * F20_FSL;
  const float nrm2 = f20_norm_fwd(v, fb, tw, c);
  const cf wl = A.tw[c];
  const int src = (lane & 32) | ((32 - c) & 31);
  const bool l0 = c == 0;
  // lane c < 17 of group g: word c of frame tq + g
  const unsigned long long myword =
      f20_decide_pack<true>(v, s_t2, nrm2, valid, need, floor_live, u, row, chunk, tq, lane, wl, regions + wave * WAVE_CX_H);
  // ---- publish this tile's bits; the spectra stay in v[] --------------------------------------------------------
  const int fr = 2 * wave + g;      // tile row of this lane group's frame
  unsigned long long* xb_mine = P.xbits + ((size_t)u * W.ntt + (jt + 1)) * O20_TILE_WORDS;
  if (c < O20_XW) {
    const op_v4u ga = {(unsigned)myword, P.epoch, (unsigned)(myword >> 32), P.epoch};
    op_st16_sc1(&xb_mine[(fr * O20_XW + c) * 2], ga);
  }
  __syncthreads();   // every wave is past its forward exchange: the slices are idle from here
  if (W.halo_tile) return;

  // ---- integer smoothing on the matrix cores ---------------------------------------------------------------------
  const int nt = P.nt;
  char* arena = reinterpret_cast<char*>(regions);
  unsigned long long* brow = reinterpret_cast<unsigned long long*>(arena);                           // [O20_ROWS][O20_BW]
  unsigned short* Ks = reinterpret_cast<unsigned short*>(arena + (size_t)O20_ROWS * O20_BW * 8);     // [8][O20_KP]
  static_assert(O20_ROWS * O20_BW * 8 + O20_NF * O20_KP * 2 <= WAVES * WAVE_CX_H * 8, "bits + K tile must fit the exchange slices");
  if (c < O20_XW) brow[(nt + fr) * O20_BW + 1 + c] = myword;
  zero_bit_row_margins<NF, O20_XW, O20_ROWS, WAVES * 64>(brow, nt, tid);
  poll_neighbour_rows<NF, O20_XW, O20_BW, WAVES * 64>(xb_mine, NF, nt, P, s_misc, brow, tid);
  const int q4 = lane >> 4, j16 = lane & 15;
  const long Bl = (long)P.tab[lane], Bh = (long)P.tab[64 + lane], At = (long)P.tab[128 + lane];
  __syncthreads();
  {
    // Per 16-bin block b:  H[row][16 b + j] = sum_k bit[row][16 b - 24 + k] vf[k - 24 - j] + sum_k bit[row][16 b + 8 + k] vf[k + 8 - j]
    // for the two row blocks (result: lane = bin column, 4 consecutive rows per lane group = the B layout of the time product);
    //   K[frame][bin] = sum_slot vt[row(slot) - nt - frame] H[row(slot)][bin],   k-slot 8 q + e = row 4 q + e of block 0 (e < 4) / 1
    // on the two base-128 digits of H.  Output frames 0..7 = lane groups q4 < 2.
    const reg_v4i zero4 = {0, 0, 0, 0};
    const unsigned char* wbb = reinterpret_cast<const unsigned char*>(brow);
    constexpr int WPB = O20_BW * 8;
    for (int b = wave; b < 65; b += WAVES) {
      unsigned lo[2], hi[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const unsigned char* rp = wbb + (16 * m + j16) * WPB + q4 + 2 * b;
        const long a0 = (long)s_exp[rp[5]], a1 = (long)s_exp[rp[9]];
        reg_v4i hv = __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, Bl, zero4, 0, 0, 0);
        hv = __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, Bh, hv, 0, 0, 0);
        lo[m] = ((unsigned)hv[0] & 127u) | (((unsigned)hv[1] & 127u) << 8) | (((unsigned)hv[2] & 127u) << 16) | (((unsigned)hv[3] & 127u) << 24);
        hi[m] = ((unsigned)hv[0] >> 7) | (((unsigned)hv[1] >> 7) << 8) | (((unsigned)hv[2] >> 7) << 16) | (((unsigned)hv[3] >> 7) << 24);
      }
      const long bt0 = (long)(((unsigned long long)lo[1] << 32) | (unsigned long long)lo[0]);
      const long bt1 = (long)(((unsigned long long)hi[1] << 32) | (unsigned long long)hi[0]);
      const reg_v4i d0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(At, bt0, zero4, 0, 0, 0);
      const reg_v4i d1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(At, bt1, zero4, 0, 0, 0);
      if (q4 < 2) {
        unsigned short* kd = Ks + (4 * q4) * O20_KP + 16 * b + j16;
        store_k4(kd, O20_KP, d0 + (d1 << 7));
      }
    }
  }
  __syncthreads();

  // ---- x mask, merge (k_apply_fast2048<K>, the mask entries read from the K tile in LDS) --------------------------
  const bool wave_live = tf0 + 2 * wave + 1 >= 0 && tf0 + 2 * wave < G.T;
  if (wave_live) {
    // pair_mask leaves out four 1/2 factors; the inverse transform a factor 1024; K / ktot for the integer sums
    const float ks = A.inv_ktot * (0.25f / 1024.0f) * P.prop;
    const bool propn = P.prop != 1.0f;   // + (1 - p) E / ktot (thresh.hpp: tri_valid)
    const float tq_ = propn ? (1.0f - P.prop) * A.inv_ktot * (0.25f / 1024.0f) * tri_valid(nt, tf0 + fr, G.T) : 0.f;
    const int nfw = P.nf;
    const unsigned short* Kf = Ks + fr * O20_KP;
    auto mval = [&](int k) -> float {
      float m = (float)Kf[k] * ks;
      if (propn) m = fmaf(tri_valid(nfw, k, F20_F), tq_, m);
      return m;
    };
    // (opaque copy: the 16 pair twiddles w_2048^c w_64^i are recomputed here -- kept from the decision stage they are 32 live
    // registers across the smoothing, 14 of which went to scratch)
    cf wl2 = wl;
    asm volatile("" : "+v"(wl2.x), "+v"(wl2.y));
    const cf a0 = v[0], a16 = v[16];
    cf carry = v[0];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const cf oa = v[i], ob = v[31 - i];
      cf ta;
      ta.x = __shfl(ob.x, src); ta.y = __shfl(ob.y, src);     // Zc[1024 - k]: lane 32 - c, register 31 - i
      cf ba = {l0 ? carry.x : ta.x, l0 ? carry.y : ta.y};      // lane 0: original register 32 - i (i = 0: itself)
      carry = ob;
      const int ka = c + 32 * i;
      cf xa = oa;
      pair_mask(xa, ba, f20_wk(wl2, i), mval(ka), mval(1024 - ka));          // (ka = 0: the second mask is bin 1024's)
      v[i] = xa;
      v[31 - i].x = __shfl(ba.x, src);                          // the partner's merged value for OUR register 31 - i
      v[31 - i].y = __shfl(ba.y, src);
    }
    if (l0) {
#pragma unroll
      for (int j = 31; j >= 17; --j) v[j] = v[j - 1];
      const float m16 = mval(512) * 4.0f;
      v[16] = {a16.x * m16, a16.y * m16};
      const float y0 = (a0.x + a0.y) * mval(0) * 4.0f;
      const float yN = (a0.x - a0.y) * mval(1024) * 4.0f;
      v[0] = {0.5f * (y0 + yN), 0.5f * (y0 - yN)};
    }
  }
  __syncthreads();   // every lane has used its mask entries: the slices are free for the inverse transform
  if (wave_live) {
    int zi = 0, ci = c;
    asm volatile("" : "+v"(zi), "+v"(ci));
    fft1k_inv(v, fb + zi, tw + zi, ci);
  }
  __syncthreads();   // every wave is past its exchanges: the regions become the tile's hop buffer
  // ---- window, overlap-add in four ordered rounds, store; straddling hops as partial sums (k_apply_fast2048, seam mode) ----
  float* hop = reinterpret_cast<float*>(regions);
  static_assert((NF + 3) * F20_XP * 4 <= WAVES * WAVE_CX_H * 8, "hop buffer must fit the regions");
  const float2* ws = reinterpret_cast<const float2*>(A.win + 2 * c);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool first = (j == 0) || (fr == NF - 1);
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      const int r = 8 * j + rr;
      const float2 w2 = ws[32 * r];
      float2* dst = reinterpret_cast<float2*>(hop + (fr + j) * F20_XP + 2 * c + 64 * rr);
      float2 nw = {wave_live ? v[r].x * w2.x : 0.f, wave_live ? v[r].y * w2.y : 0.f};
      if (!first) { const float2 old = *dst; nw.x += old.x; nw.y += old.y; }
      *dst = nw;
    }
    __syncthreads();
  }
  const float poison = s_misc[1] != 0u ? __uint_as_float(0x7fc00000u) : 0.f;
  const int s4 = (tid & 127) * 4;
  for (int jj = (tid >> 7); jj < NF + 3; jj += (WAVES * 64) >> 7) {
    const int64_t h = tf0 + jj;
    if (h < A.h_begin || h >= A.h_end) continue;
    float4 a4 = *reinterpret_cast<const float4*>(&hop[jj * F20_XP + s4]);
    a4.x += poison; a4.y += poison; a4.z += poison; a4.w += poison;
    if (jj < 3 || jj >= NF) {   // straddling hop: partial sum only (poisoned with the tile), k_ola_seam finishes it
      store_partial_hop<F20_H>(A, u, jt, jj, NF, s4, a4);
      continue;
    }
    finish_hop<F20_H>(A, row, chunk, h, s4, a4);
  }
}

}  // namespace fast
}  // namespace sg
