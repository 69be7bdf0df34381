// One-pass stationary gate for n_fft = win = 512, hop = 128 (round 6; VERDICT r3 / r4 / r5 "one-pass gates for n_fft != 1024").
//
//   k_decide_fast512 + k_smooth_bits2 + k_apply_fast512<K>      (3 transforms per frame pair, bit field and K field in HBM)
//     ->  k_gate_onepass512                                      (2 transforms per frame pair, neither field)
//
// The tile scaffold -- ticket and tile identity, floor test over the unstaged padding, parked spectra around the exact
// re-evaluation, published bits and the poll of the neighbours' rows, K rows, partial-sum slots and the finished hops -- is
// onepass_reg.hpp / fastpath.hpp (store_partial_hop, finish_hop), shared with onepass256.hpp and onepass2048.hpp.  This file's own:
//   * the tile: 32 consecutive frames (4 wavefronts x 4 lane groups x one frame PAIR per 512-point register transform of
//     fast512.hpp), 257 bins = 5 bit words per frame; decisions in float32 + exact float64 refinement on the pair split (the
//     bits of k_decide_fast512), packed by a 16 x 16 bit transpose across the lane group;
//   * the integer smoothing ON THE MATRIX CORES (v_mfma_i32_16x16x32_i8, the formulation of onepass.hpp): per 16-bin block,
//     H = bits x band matrix for the five 16-row blocks of the tile (32 + 2 nt <= 80 rows, nf <= 8), then K = time weights x H
//     for the two 16-frame halves (two 32-row k-blocks each: 16 + 2 nt <= 64 rows, nt <= 24); H never leaves the registers, bits
//     and the K tile (uint16) live in the exchange slices: 3 workgroups per CU as k_apply_fast512.  (A first build ran both
//     directions as sliding-window recurrences in LDS -- popcounts along f, two running boxcars along t: 203 us per two minutes
//     where the three kernels it replaces take 103.)
//   * x mask, merge, inverse transform and the wave-private overlap-add of k_apply_fast512<K>, any prop_decrease (a scale and
//     an offset on the mask entries).
// Tiles ABUT by default (A.part set: the 3 hops that straddle two tiles leave as partial sums, k_ola_seam -- fastpath.hpp --
// combines them after the launch: 1490 workgroups per two minutes instead of 1640, no redundant transforms) or,
// SG_OPT_FORCE_NOSEAM, overlap by 3 frames (29 complete hops per tile).
#pragma once
#include "fast512.hpp"
#include "onepass_reg.hpp"

namespace sg {
namespace fast {

constexpr int O5_NF = 32, O5_NH = 29;              // frames / complete hops per tile
constexpr int O5_XW = 5;                           // 64-bit words per bit row (257 bins)
constexpr int O5_TILE_WORDS = O5_NF * O5_XW * 2;   // payload of one tile: 320 tagged 8-byte halves = 2560 B
constexpr int O5_BW = O5_XW + 2;                   // bit row pitch in LDS: one zero word on each side
constexpr int O5_ROWS = 80;                        // bit rows in LDS: five 16-row blocks (32 + 2 nt <= 80)
constexpr int O5_KP = 272;                         // K row pitch (entries): 17 blocks of 16 bins
constexpr int O5_MAX_NT = 24;                      // 16 + 2 nt <= 64 rows = two k-blocks of the time product
constexpr int O5_MAX_NF = 8;                       // the 32 x 16 band matrix of the frequency product
// constant operands (device table `tab`, 64-bit entries): [0, 64) Bf (band matrix, per lane), [64, 128) At1, [128, 192) At2 (time
// weights of the two k-blocks), [192, 448) byte -> eight 0 / 1 bytes

#ifndef O5_OCC
#define O5_OCC 3   // workgroups per CU the register budget is set for
#endif
template <int WAVES, bool REDO = false>
__global__ __launch_bounds__(WAVES * 64, O5_OCC) void k_gate_onepass512(OnePassRegArgs P) {
  static_assert(WAVES == 4, "tile = 32 frames");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf* tw512 = reinterpret_cast<cf*>(smem);
  cf* regions = tw512 + FN;
  float* swin = reinterpret_cast<float*>(regions + WAVES * WAVE_CX_H);
  float* s_t2 = swin + F5_N;                 // [257] float32 compare constants x4 (the split works on 2 X)
  unsigned* s_misc = reinterpret_cast<unsigned*>(s_t2 + 264);   // [0] ticket, [1] lost hand-off
  unsigned long long* s_exp = reinterpret_cast<unsigned long long*>(s_misc + 4);   // [256] byte -> eight 0 / 1 bytes
  const RegArgs& A = P.A;
  if (REDO && A.fl.alim[1] != A.tc.need_tag) return;   // no unit of this call reported (the common case)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
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
  stage_t2_plain<WAVES * 64, F5_F>(s_t2, A.tc.T2, need, 4.0, tid,
                                 [&](int f) { return t2_effective(A.tc, u, G.FS, f, need, floor_live, A.mag_scale, A.top_db); });
  constexpr int NF = O5_NF, NH = O5_NH;
  const bool seam = A.part != nullptr;   // abutting tiles + k_ola_seam (fastpath.hpp); else tiles that overlap by 3 frames
  const int step = seam ? NF : NH;       // frames from one tile to the next
  const int64_t tf0 = A.h_begin - 3 + (int64_t)jt * step;   // first frame of the tile
  cf v[32];
  bool validA, validB;
  unsigned fl_mx = f5_gather<WAVES, true>(A, tw512, regions, swin, row, chunk, tf0, G.T, v, validA, validB);
  if (!REDO && W.lazy) floor_scan_padding<WAVES * 64, F5_H, NF>(A, P, row, chunk, jt, step, tid, fl_mx);   // the padding no tile stages
  if (!REDO) floor_lazy_report(A.tc, A.fl, fl_bound, fl_mx, u, G.FS, lane);
  const int64_t tq = tf0 + F5_FPW * wave;
  // ---- forward transform + decisions (fast512.hpp: f5_decide_pack) -------------------------------------------------------
  cf* fb = regions + wave * WAVE_CX_H + frame_base_h(g);
  float nA, nB;
  f5_norms_fwd(v, fb, tw512, c, nA, nB);
  const bool l0 = c == 0;
  unsigned long long wA, wB;   // lane c < 5 of group g: word c of frames tq + 2 g, tq + 2 g + 1
  f5_decide_pack<true>(v, s_t2, nA, nB, validA, validB, need, floor_live, u, row, chunk, tq, lane, regions + wave * WAVE_CX_H, wA,
                       wB);
  // ---- publish this tile's bits; the spectra stay in v[] --------------------------------------------------------
  const int fa = F5_FPW * wave + 2 * g;      // tile row of frame A (B: fa + 1)
  unsigned long long* xb_mine = P.xbits + ((size_t)u * W.ntt + (jt + 1)) * O5_TILE_WORDS;
  if (c < O5_XW) {
    const op_v4u ga = {(unsigned)wA, P.epoch, (unsigned)(wA >> 32), P.epoch};
    const op_v4u gb = {(unsigned)wB, P.epoch, (unsigned)(wB >> 32), P.epoch};
    op_st16_sc1(&xb_mine[((fa)*O5_XW + c) * 2], ga);
    op_st16_sc1(&xb_mine[((fa + 1) * O5_XW + c) * 2], gb);
  }
  __syncthreads();   // every wave is past its forward exchange: the slices are idle from here
  if (W.halo_tile) return;

  // ---- integer smoothing on the matrix cores (onepass.hpp) ----------------------------------------------------------
  const int nt = P.nt;
  char* arena = reinterpret_cast<char*>(regions);
  unsigned long long* brow = reinterpret_cast<unsigned long long*>(arena);                           // [O5_ROWS][O5_BW]
  unsigned short* Ks = reinterpret_cast<unsigned short*>(arena + (size_t)O5_ROWS * O5_BW * 8);       // [32][O5_KP]
  static_assert(O5_ROWS * O5_BW * 8 + O5_NF * O5_KP * 2 <= WAVES * WAVE_CX_H * 8, "bits + K tile must fit the exchange slices");
  if (c < O5_XW) {
    brow[(nt + fa) * O5_BW + 1 + c] = wA;
    brow[(nt + fa + 1) * O5_BW + 1 + c] = wB;
  }
  zero_bit_row_margins<NF, O5_XW, O5_ROWS, WAVES * 64>(brow, nt, tid);
  poll_neighbour_rows<NF, O5_XW, O5_BW, WAVES * 64>(xb_mine, step, nt, P, s_misc, brow, tid);
  const int q4 = lane >> 4, j16 = lane & 15;
  const long Bf = (long)P.tab[lane], At1 = (long)P.tab[64 + lane], At2 = (long)P.tab[128 + lane];
  __syncthreads();
  {
    // Per 16-bin block b:  H[row][bin] = sum_k bit[row][16 b - 8 + k] vf[k - 8 - j]   (A = 16 rows x 32 bins of 0 / 1 bytes, B = Bf)
    // for the five row blocks; the result layout (lane = bin column, 4 consecutive rows per lane group) IS the B layout of
    //   K[frame][bin] = sum_slot vt[row(slot) - nt - frame] H[row(slot)][bin]       (A = At1 / At2, B = two packed H blocks)
    // Output frames 16 hh + j (hh = 0, 1) sit at bit row nt + 16 hh + j and reach rows 16 hh + j .. 16 hh + j + 2 nt: row blocks
    // hh .. hh + 3; k-slot 8 q + e of the first product = row 4 q + e of block hh (e < 4) / block hh + 1 (e >= 4), of the second
    // = blocks hh + 2 / hh + 3 -- the same weights for both halves.
    const reg_v4i zero4 = {0, 0, 0, 0};
    const unsigned char* wbb = reinterpret_cast<const unsigned char*>(brow);
    constexpr int WPB = O5_BW * 8;
    for (int b = wave; b < 17; b += WAVES) {
      unsigned hp[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const long a = (long)s_exp[wbb[(16 * m + j16) * WPB + 7 + q4 + 2 * b]];
        const reg_v4i hv = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, Bf, zero4, 0, 0, 0);
        hp[m] = (unsigned)hv[0] | ((unsigned)hv[1] << 8) | ((unsigned)hv[2] << 16) | ((unsigned)hv[3] << 24);
      }
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const long bt1 = (long)(((unsigned long long)hp[hh + 1] << 32) | (unsigned long long)hp[hh]);
        const long bt2 = (long)(((unsigned long long)hp[hh + 3] << 32) | (unsigned long long)hp[hh + 2]);
        reg_v4i d = __builtin_amdgcn_mfma_i32_16x16x32_i8(At1, bt1, zero4, 0, 0, 0);
        d = __builtin_amdgcn_mfma_i32_16x16x32_i8(At2, bt2, d, 0, 0, 0);
        unsigned short* kd = Ks + (16 * hh + 4 * q4) * O5_KP + 16 * b + j16;   // lane group q4: output frames 4 q4 .. 4 q4 + 3
        store_k4(kd, O5_KP, d);
      }
    }
  }
  __syncthreads();
  float ma[16], mb[16], m256a, m256b;
  {
    const float ks = A.inv_ktot * (0.5f / 512.0f) * P.prop;   // p K / ktot, the 1/2 of the split and the 1/512 of the inverse transform
    const unsigned short* KA = Ks + fa * O5_KP;
    const unsigned short* KB = KA + O5_KP;
    const float ksA = validA ? ks : 0.f, ksB = validB ? ks : 0.f;   // frames outside [0, T): mask zero (k_apply_fast512)
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) {
      const int f = bin5(c, sl);
      ma[sl] = (float)KA[f] * ksA;
      mb[sl] = (float)KB[f] * ksB;
    }
    m256a = (float)KA[256] * (2.f * ksA);
    m256b = (float)KB[256] * (2.f * ksB);
    if (P.prop != 1.0f) {   // + (1 - p) E / ktot (thresh.hpp: tri_valid)
      const float kq = (1.0f - P.prop) * A.inv_ktot * (0.5f / 512.0f);
      const float tA = validA ? kq * tri_valid(nt, tf0 + fa, G.T) : 0.f, tB = validB ? kq * tri_valid(nt, tf0 + fa + 1, G.T) : 0.f;
#pragma unroll
      for (int sl = 0; sl < 16; ++sl) {
        const float wf = tri_valid(P.nf, bin5(c, sl), F5_F);
        ma[sl] = fmaf(wf, tA, ma[sl]);
        mb[sl] = fmaf(wf, tB, mb[sl]);
      }
      const float w256 = 2.f * tri_valid(P.nf, 256, F5_F);
      m256a = fmaf(w256, tA, m256a);
      m256b = fmaf(w256, tB, m256b);
    }
  }
  __syncthreads();   // every lane has its mask entries: the slices are free for the inverse transform

  // ---- x mask, merge, inverse transform, window, overlap-add, store (k_apply_fast512<K>) --------------------------
  const bool wave_live = tf0 + F5_FPW * wave + F5_FPW - 1 >= 0 && tf0 + F5_FPW * wave < G.T;
  if (wave_live) {
    cf na[16], nb[16];
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) {
      cf a, b;
      f5_pair(v, sl, l0, a, b);
      const cf E = {a.x + b.x, a.y - b.y}, O = {a.y + b.y, b.x - a.x};
      const cf Ya = {E.x * ma[sl], E.y * ma[sl]}, Yb = {O.x * mb[sl], O.y * mb[sl]};
      na[sl] = {Ya.x - Yb.y, Ya.y + Yb.x};
      nb[sl] = {Ya.x + Yb.y, Yb.x - Ya.y};
    }
    auto sel = [&](cf a0, cf a1) -> cf { return {sel_s(F5_L0, a0.x, a1.x), sel_s(F5_L0, a0.y, a1.y)}; };
    cf nv[32];
    {
      const cf z0 = {v[0].x * (2.f * ma[0]), v[0].y * (2.f * mb[0])};
      const cf z8 = {v[8].x * m256a, v[8].y * m256b};
      nv[0] = sel(z0, na[0]);
      nv[8] = z8;
      nv[31] = nb[0];
    }
#pragma unroll
    for (int i = 1; i < 8; ++i) nv[i] = na[i];
    {
      const cf keep8 = nv[8];
      nv[8] = sel(keep8, na[8]);
    }
#pragma unroll
    for (int i = 9; i < 16; ++i) nv[i] = sel(nb[16 - i], na[i]);
#pragma unroll
    for (int i = 16; i < 24; ++i) nv[i] = sel(na[i - 8], nb[31 - i]);
#pragma unroll
    for (int i = 24; i < 31; ++i) nv[i] = sel(nb[39 - i], nb[31 - i]);
    {
      const cf keep31 = nv[31];
      nv[31] = sel(nb[8], keep31);
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) v[i] = nv[i];
    {
      int zi = 0, ci = c;
      asm volatile("" : "+v"(zi), "+v"(ci));
      fft512_inv_half(v, fb + zi, tw512 + zi, ci);
    }
  }
  float* acc = reinterpret_cast<float*>(regions + wave * WAVE_CX_H);
  static_assert((F5_FPW + 3) * F5_HP * 4 <= WAVE_CX_H * 8, "hop accumulators must fit the wave's slice");
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int fA = 2 * g, fB = 2 * g + 1;
    const bool firstA = j == 0, firstB = (j == 0) || (g == 3);
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      const int r = 8 * j + rr;
      const float ws = swin[c + 16 * r];
      float* dA = acc + (fA + j) * F5_HP + c + 16 * rr;
      float* dB = acc + (fB + j) * F5_HP + c + 16 * rr;
      float ya = wave_live ? v[r].x * ws : 0.f, yb = wave_live ? v[r].y * ws : 0.f;
      if (!firstA) ya += *dA;
      *dA = ya;
      if (!firstB) yb += *dB;
      *dB = yb;
    }
    wave_lds_sync();
  }
  __syncthreads();
  const float poison = s_misc[1] != 0u ? __uint_as_float(0x7fc00000u) : 0.f;
  const float* fr = reinterpret_cast<const float*>(regions);
  const int s4 = (tid & 31) * 4;
  for (int jj = (seam ? 0 : 3) + (tid >> 5); jj < (seam ? NF + 3 : NF); jj += (WAVES * 64) >> 5) {
    const int64_t h = tf0 + jj;
    if (h < A.h_begin || h >= A.h_end) continue;
    const int wv = jj < NF ? jj >> 3 : WAVES - 1, lh = jj < NF ? jj & 7 : 8 + (jj - NF);   // (jj >= NF: the last wave's overflow rows)
    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (wv >= 1 && lh <= 2) a4 = *reinterpret_cast<const float4*>(&fr[(wv - 1) * WAVE_CX_H * 2 + (lh + 8) * F5_HP + s4]);
    {
      const float4 f4 = *reinterpret_cast<const float4*>(&fr[wv * WAVE_CX_H * 2 + lh * F5_HP + s4]);
      a4.x += f4.x; a4.y += f4.y; a4.z += f4.z; a4.w += f4.w;
    }
    a4.x += poison; a4.y += poison; a4.z += poison; a4.w += poison;
    if (seam && (jj < 3 || jj >= NF)) {   // straddling hop: partial sum only (poisoned with the tile), k_ola_seam finishes it
      store_partial_hop<F5_H>(A, u, jt, jj, NF, s4, a4);
      continue;
    }
    finish_hop<F5_H>(A, row, chunk, h, s4, a4);
  }
}

}  // namespace fast
}  // namespace sg
