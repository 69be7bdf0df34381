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
  // ---- forward transform + decisions (k_decide_fast2048) ------------------------------------------------------
  float nrm2 = 0.f;
#pragma unroll
  for (int r = 0; r < 32; ++r) nrm2 += v[r].x * v[r].x + v[r].y * v[r].y;
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) nrm2 += __shfl_xor(nrm2, o);
  cf* fb = regions + wave * WAVE_CX_H + g * F20_FSL;
  {
    int z0 = 0;
    asm volatile("" : "+v"(z0));
    fft1k_fwd(v, fb, tw + z0, c);
  }
  const cf wl = A.tw[c];
  const int src = (lane & 32) | ((32 - c) & 31);
  const bool l0 = c == 0;
  unsigned long long myword = 0ull;   // lane c < 17 of group g: word c of frame tq + g
  {
    const float d2 = nrm2 > 0.f ? 8.0f * 2.3283064e-10f * nrm2 : -1.0f;
    unsigned pred = 0, amb = 0;
    bool predN = false, ambN = false;     // bin 1024 (lane 0)
    {
      auto decide = [&](float Pw, float T, int q) {
        const float diff = Pw - T;
        pred |= (diff > 0.f ? 1u : 0u) << q;
        amb |= ((diff * diff <= d2 * (Pw + T)) ? 1u : 0u) << q;
      };
      float Pp[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const cf ob = v[31 - i], own = v[(32 - i) & 31];
        cf ta;
        ta.x = __shfl(ob.x, src); ta.y = __shfl(ob.y, src);
        const cf ba = {l0 ? own.x : ta.x, l0 ? own.y : ta.y};
        cf xa, xb;
        split_pair(v[i], ba, f20_wk(wl, i), xa, xb);
        decide(xa.x * xa.x + xa.y * xa.y, s_t2[c + 32 * i], i);
        Pp[i] = xb.x * xb.x + xb.y * xb.y;
      }
      {   // lane 0, i = 0: the pair (Zc[0], Zc[0]) also yields bin 1024
        const float PN = Pp[0], TN = s_t2[1024], dN = PN - TN;
        predN = l0 && dN > 0.f;
        ambN = l0 && dN * dN <= d2 * (PN + TN);
      }
      const float P512 = 4.f * (v[16].x * v[16].x + v[16].y * v[16].y);   // lane 0: Zc[512] is its own partner
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float pu = __shfl(Pp[i], src);
        const float p0 = i < 15 ? Pp[i + 1] : P512;
        decide(l0 ? p0 : pu, s_t2[c + 32 * (31 - i)], 31 - i);
      }
    }
    if (need == 2 || !valid) { pred = 0; amb = 0; predN = false; ambN = false; }
    // exact re-evaluation of ambiguous cells, one at a time, whole wave cooperating; half of the spectra parked in the wave's
    // idle exchange slice for the duration (onepass_reg.hpp: park_upper_half)
    if (__ballot(amb != 0 || ambN) != 0ull) {
      float* park = reinterpret_cast<float*>(regions + wave * WAVE_CX_H) + lane;
      park_upper_half(v, park);
      while (true) {
        const unsigned long long pending = __ballot(amb != 0 || ambN);
        if (pending == 0) break;
        const int sl = __ffsll((long long)pending) - 1;
        const unsigned amb_s = (unsigned)__shfl((int)amb, sl);
        const int q = amb_s ? (__ffs((int)amb_s) - 1) : 32;
        const int cs = sl & 31, gs = sl >> 5;
        const int f = q < 32 ? cs + 32 * q : 1024;
        const RegArgs& L = *late_args<RegArgs>();     // (cold path: arguments re-read here; A is the FIRST member)
        const double Pe = f20_exact_power(L, row, chunk, tq + gs, f, lane);
        const bool pass = Pe > t2_effective(L.tc, u, L.g.FS, f, need, floor_live, L.mag_scale, L.top_db);
        if (lane == sl) {
          if (q < 32) {
            pred = (pred & ~(1u << q)) | ((pass ? 1u : 0u) << q);
            amb &= ~(1u << q);
          } else {
            predN = pass;
            ambN = false;
          }
        }
      }
      wave_lds_sync();
      unpark_upper_half(v, park);
      wave_lds_sync();
    }
    // pack (k_decide_fast2048): the ballot of register k2 is, per frame, the 32 bins 32 k2 .. 32 k2 + 31 in natural order
    const int sh = 32 * g;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const unsigned long long b0 = __ballot((pred >> (2 * w)) & 1u), b1 = __ballot((pred >> (2 * w + 1)) & 1u);
      const unsigned long long word = ((b0 >> sh) & 0xffffffffull) | (((b1 >> sh) & 0xffffffffull) << 32);
      if (c == w) myword = word;
    }
    {
      const unsigned long long bN = __ballot(predN);
      if (c == 16) myword = (bN >> sh) & 1ull;
    }
  }
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
