// One-pass stationary gate for n_fft = win = 256, hop = 64 (round 6).
//
//   k_decide_fast256 + k_smooth_bits2 + k_apply_fast256<K>   ->   k_gate_onepass256   (no bit field, no K field in HBM)
//
// The tile scaffold is onepass_reg.hpp / fastpath.hpp (store_partial_hop, finish_hop), shared with onepass512.hpp and
// onepass2048.hpp.  This file's own:
//   * the tile: 64 frames, FOUR real frames per 512-point register transform of fast256.hpp, 129 bins = 3 bit words per frame
//     (abutting tiles + k_ola_seam by default, 61 complete hops per tile with SG_OPT_FORCE_NOSEAM); decisions on the four-frame
//     split (the bits of k_decide_fast256), packed with ballots;
//   * the integer smoothing on the matrix cores: 9 blocks of 16 bit rows (64 + 2 nt <= 144) x 9 blocks of 16 bins; per bin block
//     H = bits x band matrix for the nine row blocks, then K = time weights x H for the four 16-frame blocks of the tile, each
//     reaching 16 + 2 nt <= 96 rows = three k-blocks of 32 (the third only when nt > 24: at 48 kHz the 50 ms window is 37 frames);
//   * x mask, merge, inverse transform and the wave-private overlap-add of k_apply_fast256<K>.
#pragma once
#include "fast256.hpp"
#include "onepass_reg.hpp"

namespace sg {
namespace fast {

constexpr int O25_NF = 64, O25_NH = 61;               // frames / complete hops per tile
constexpr int O25_XW = 3;                             // 64-bit words per bit row (129 bins)
constexpr int O25_TILE_WORDS = O25_NF * O25_XW * 2;   // payload of one tile: 384 tagged 8-byte halves = 3072 B
constexpr int O25_BW = O25_XW + 2;                    // bit row pitch in LDS: one zero word on each side
constexpr int O25_ROWS = 144;                         // bit rows in LDS: nine 16-row blocks (64 + 2 nt <= 144)
constexpr int O25_KP = 144;                           // K row pitch (entries): 9 blocks of 16 bins
constexpr int O25_MAX_NT = 40;                        // 16 + 2 nt <= 96 rows = three k-blocks of the time product
constexpr int O25_MAX_NF = 8;
// constant operands (device table `tab`, 64-bit entries): [0, 64) Bf, [64, 128) At1, [128, 192) At2, [192, 256) At3,
// [256, 512) byte -> eight 0 / 1 bytes

#ifndef O25_OCC
#define O25_OCC 3
#endif
template <int WAVES, bool REDO = false>
__global__ __launch_bounds__(WAVES * 64, O25_OCC) void k_gate_onepass256(OnePassRegArgs P) {
  static_assert(WAVES == 4, "tile = 64 frames");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf* tw512 = reinterpret_cast<cf*>(smem);
  cf* regions = tw512 + FN;
  float* swin = reinterpret_cast<float*>(regions + WAVES * WAVE_CX_H);
  float* s_t2 = swin + F25_N;                // [129] float32 compare constants x4
  unsigned* s_misc = reinterpret_cast<unsigned*>(s_t2 + F25_T2);   // [0] ticket, [1] lost hand-off
  unsigned long long* s_exp = reinterpret_cast<unsigned long long*>(s_misc + 4);   // [256] byte -> eight 0 / 1 bytes
  const RegArgs& A = P.A;
  if (REDO && A.fl.alim[1] != A.tc.need_tag) return;   // no unit of this call reported (the common case)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15, cp = c >> 1;
  const Geom& G = A.g;
  reg_draw_ticket(P, s_misc, tid);
  s_exp[tid] = P.tab[256 + tid];
  const unsigned fl_bound = REDO ? 0xffffffffu : floor_lazy_bound(A.fl, lane);
  __syncthreads();
  const RegTile W = reg_tile_of<REDO>(P, s_misc[0], tid);   // (ticket 0 of a first launch: also zeroes the REDO launch's counter)
  if (REDO && W.need == 0) return;   // whole workgroup
  const int64_t u = W.u, row = W.row, chunk = W.chunk;
  const int jt = W.jt, need = W.need;
  const bool floor_live = W.floor_live;
  stage_t2_plain<WAVES * 64, F25_F>(s_t2, A.tc.T2, need, 4.0, tid,
                                 [&](int f) { return t2_effective(A.tc, u, G.FS, f, need, floor_live, A.mag_scale, A.top_db); });
  constexpr int NF = O25_NF, NH = O25_NH;
  const bool seam = A.part != nullptr;   // abutting tiles + k_ola_seam (fastpath.hpp); else tiles that overlap by 3 frames
  const int step = seam ? NF : NH;       // frames from one tile to the next
  const int64_t tf0 = A.h_begin - 3 + (int64_t)jt * step;   // first frame of the tile
  cf v[32];
  bool validX, validY;
  unsigned fl_mx = f25_gather<WAVES, true>(A, tw512, regions, swin, row, chunk, tf0, v, validX, validY);
  if (!REDO && W.lazy) floor_scan_padding<WAVES * 64, F25_H, NF>(A, P, row, chunk, jt, step, tid, fl_mx);   // the padding no tile stages
  if (!REDO) floor_lazy_report(A.tc, A.fl, fl_bound, fl_mx, u, G.FS, lane);
  const int64_t tq = tf0 + F25_FPW * wave;
  // ---- forward transform + decisions (fast256.hpp: f25_decide_pack) -------------------------------------------------------
  cf* fb = regions + wave * WAVE_CX_H + frame_base_h(g);
  float n1, n2;
  f25_norms_fwd(v, fb, tw512, lane, n1, n2);
  const bool l0 = c == 0;
  // lane c = 4 fr + w (w < 3) of a group: word w of frame tq + 4 g + fr
  const unsigned long long mine =
      f25_decide_pack<true>(v, s_t2, n1, n2, G.T, need, floor_live, u, row, chunk, tq, lane, regions + wave * WAVE_CX_H);
  // ---- publish this tile's bits; the spectra stay in v[] --------------------------------------------------------
  const int fq = F25_FPW * wave + 4 * g;     // tile row of the group's first frame
  const int my_row = fq + (c >> 2), my_w = c & 3;
  unsigned long long* xb_mine = P.xbits + ((size_t)u * W.ntt + (jt + 1)) * O25_TILE_WORDS;
  if (my_w < O25_XW) {
    const op_v4u gr = {(unsigned)mine, P.epoch, (unsigned)(mine >> 32), P.epoch};
    op_st16_sc1(&xb_mine[(my_row * O25_XW + my_w) * 2], gr);
  }
  __syncthreads();   // every wave is past its forward exchange: the slices are idle from here
  if (W.halo_tile) return;

  // ---- integer smoothing on the matrix cores --------------------------------------------------------------------
  const int nt = P.nt;
  char* arena = reinterpret_cast<char*>(regions);
  unsigned long long* brow = reinterpret_cast<unsigned long long*>(arena);                           // [O25_ROWS][O25_BW]
  unsigned short* Ks = reinterpret_cast<unsigned short*>(arena + (size_t)O25_ROWS * O25_BW * 8);     // [64][O25_KP]
  static_assert(O25_ROWS * O25_BW * 8 + O25_NF * O25_KP * 2 <= WAVES * WAVE_CX_H * 8, "bits + K tile must fit the exchange slices");
  if (my_w < O25_XW) brow[(nt + my_row) * O25_BW + 1 + my_w] = mine;
  zero_bit_row_margins<NF, O25_XW, O25_ROWS, WAVES * 64>(brow, nt, tid);
  poll_neighbour_rows<NF, O25_XW, O25_BW, WAVES * 64>(xb_mine, step, nt, P, s_misc, brow, tid);
  const int q4 = lane >> 4, j16 = lane & 15;
  const long Bf = (long)P.tab[lane], At1 = (long)P.tab[64 + lane], At2 = (long)P.tab[128 + lane], At3 = (long)P.tab[192 + lane];
  const bool three = 2 * nt > 48;      // a third k-block of rows (wave-uniform)
  __syncthreads();
  {
    const reg_v4i zero4 = {0, 0, 0, 0};
    const unsigned char* wbb = reinterpret_cast<const unsigned char*>(brow);
    constexpr int WPB = O25_BW * 8;
    for (int b = wave; b < 9; b += WAVES) {
      unsigned hp[10];
#pragma unroll
      for (int m = 0; m < 9; ++m) {
        const long a = (long)s_exp[wbb[(16 * m + j16) * WPB + 7 + q4 + 2 * b]];
        const reg_v4i hv = __builtin_amdgcn_mfma_i32_16x16x32_i8(a, Bf, zero4, 0, 0, 0);
        hp[m] = (unsigned)hv[0] | ((unsigned)hv[1] << 8) | ((unsigned)hv[2] << 16) | ((unsigned)hv[3] << 24);
      }
      hp[9] = 0u;
#pragma unroll
      for (int o = 0; o < 4; ++o) {   // output frames 16 o + j at bit row nt + 16 o + j: row blocks o .. o + 5
        const long bt1 = (long)(((unsigned long long)hp[o + 1] << 32) | (unsigned long long)hp[o]);
        const long bt2 = (long)(((unsigned long long)hp[o + 3] << 32) | (unsigned long long)hp[o + 2]);
        reg_v4i d = __builtin_amdgcn_mfma_i32_16x16x32_i8(At1, bt1, zero4, 0, 0, 0);
        d = __builtin_amdgcn_mfma_i32_16x16x32_i8(At2, bt2, d, 0, 0, 0);
        if (three) {
          const long bt3 = (long)(((unsigned long long)hp[o + 5 < 10 ? o + 5 : 9] << 32) | (unsigned long long)hp[o + 4]);
          d = __builtin_amdgcn_mfma_i32_16x16x32_i8(At3, bt3, d, 0, 0, 0);
        }
        unsigned short* kd = Ks + (16 * o + 4 * q4) * O25_KP + 16 * b + j16;
        store_k4(kd, O25_KP, d);
      }
    }
  }
  __syncthreads();
  float mk[4][8], m128[4];
  {
    const float ks = A.inv_ktot * (0.5f / 256.0f) * P.prop;
#pragma unroll
    for (int fr = 0; fr < 4; ++fr) {
      const unsigned short* Kr = Ks + (fq + fr) * O25_KP;
      const int64_t t = tf0 + fq + fr;
      const float kf = (t >= 0 && t < G.T) ? ks : 0.f;   // frames outside [0, T): mask zero (k_apply_fast256)
#pragma unroll
      for (int e = 0; e < 8; ++e) mk[fr][e] = (float)Kr[bin6(c, e)] * kf;
      m128[fr] = (float)Kr[128] * (2.f * kf);
    }
    if (P.prop != 1.0f) {   // + (1 - p) E / ktot (thresh.hpp: tri_valid)
      const float kq = (1.0f - P.prop) * A.inv_ktot * (0.5f / 256.0f);
#pragma unroll
      for (int fr = 0; fr < 4; ++fr) {
        const int64_t t = tf0 + fq + fr;
        const float tt = (t >= 0 && t < G.T) ? kq * tri_valid(nt, t, G.T) : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) mk[fr][e] = fmaf(tri_valid(P.nf, bin6(c, e), F25_F), tt, mk[fr][e]);
        m128[fr] = fmaf(2.f * tri_valid(P.nf, 128, F25_F), tt, m128[fr]);
      }
    }
  }
  __syncthreads();   // every lane has its mask entries: the slices are free for the inverse transform

  // ---- x mask, merge, inverse transform, window, overlap-add, store (k_apply_fast256<K>) ------------------------
  const bool wave_live = tf0 + F25_FPW * wave + F25_FPW - 1 >= 0 && tf0 + F25_FPW * wave < G.T;
  if (wave_live) {
    auto sel = [&](cf a0, cf a1) -> cf { return {sel_s(F25_L0, a0.x, a1.x), sel_s(F25_L0, a0.y, a1.y)}; };
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int off = 8 * s;
      cf na[8], nb[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        cf a, b;
        f25_pair(v, off, e, l0, a, b);
        const cf E = {a.x + b.x, a.y - b.y}, O = {a.y + b.y, b.x - a.x};
        const float mx = mk[2 * s][e], my = mk[2 * s + 1][e];
        const cf Yx = {E.x * mx, E.y * mx}, Yy = {O.x * my, O.y * my};
        na[e] = {Yx.x - Yy.y, Yx.y + Yy.x};
        nb[e] = {Yx.x + Yy.y, Yy.x - Yx.y};
      }
      const cf z0 = {v[off].x * (2.f * mk[2 * s][0]), v[off].y * (2.f * mk[2 * s + 1][0])};
      const cf z4 = {v[off + 4].x * m128[2 * s], v[off + 4].y * m128[2 * s + 1]};
      cf npa[8], npb[8];
      npa[0] = sel(z0, na[0]);
#pragma unroll
      for (int i = 1; i < 4; ++i) npa[i] = na[i];
      npa[4] = sel(z4, na[4]);
#pragma unroll
      for (int i = 5; i < 8; ++i) npa[i] = sel(nb[8 - i], na[i]);
#pragma unroll
      for (int i = 0; i < 4; ++i) npb[i] = sel(na[i + 4], nb[7 - i]);
#pragma unroll
      for (int i = 4; i < 8; ++i) npb[i] = sel(nb[11 - i], nb[7 - i]);
#pragma unroll
      for (int i = 0; i < 8; ++i) { v[off + i] = npa[i]; v[16 + off + i] = npb[i]; }
    }
    {
      int zi = 0, ci = c;
      asm volatile("" : "+v"(zi), "+v"(ci));
      f25_inv_half(v, fb + zi, tw512 + zi, ci);
    }
  }
  float* acc = reinterpret_cast<float*>(regions + wave * WAVE_CX_H);
  static_assert((F25_FPW + 3) * F25_HP * 4 <= WAVE_CX_H * 8, "hop accumulators must fit the wave's slice");
  {
    const int fX = 4 * g + 2 * (c & 1), fY = fX + 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool firstX = j == 0, firstY = (j == 0) || (fY == F25_FPW - 1);
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int r = 8 * j + rr;
        const float ws = swin[cp + 8 * r];
        float* dX = acc + (fX + j) * F25_HP + cp + 8 * rr;
        float* dY = acc + (fY + j) * F25_HP + cp + 8 * rr;
        float yx = wave_live ? v[r].x * ws : 0.f, yy = wave_live ? v[r].y * ws : 0.f;
        if (!firstX) yx += *dX;
        *dX = yx;
        if (!firstY) yy += *dY;
        *dY = yy;
      }
      wave_lds_sync();
    }
  }
  __syncthreads();
  const float poison = s_misc[1] != 0u ? __uint_as_float(0x7fc00000u) : 0.f;
  const float* fr = reinterpret_cast<const float*>(regions);
  const int s4 = (tid & 15) * 4;
  for (int jj = (seam ? 0 : 3) + (tid >> 4); jj < (seam ? NF + 3 : NF); jj += (WAVES * 64) >> 4) {
    const int64_t h = tf0 + jj;
    if (h < A.h_begin || h >= A.h_end) continue;
    const int wv = jj < NF ? jj >> 4 : WAVES - 1, lh = jj < NF ? jj & 15 : 16 + (jj - NF);   // (jj >= NF: the last wave's overflow rows)
    float4 a4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (wv >= 1 && lh <= 2) a4 = *reinterpret_cast<const float4*>(&fr[(wv - 1) * WAVE_CX_H * 2 + (lh + 16) * F25_HP + s4]);
    {
      const float4 f4 = *reinterpret_cast<const float4*>(&fr[wv * WAVE_CX_H * 2 + lh * F25_HP + s4]);
      a4.x += f4.x; a4.y += f4.y; a4.z += f4.z; a4.w += f4.w;
    }
    a4.x += poison; a4.y += poison; a4.z += poison; a4.w += poison;
    if (seam && (jj < 3 || jj >= NF)) {   // straddling hop: partial sum only (poisoned with the tile), k_ola_seam finishes it
      store_partial_hop<F25_H>(A, u, jt, jj, NF, s4, a4);
      continue;
    }
    finish_hop<F25_H>(A, row, chunk, h, s4, a4);
  }
}

}  // namespace fast
}  // namespace sg
