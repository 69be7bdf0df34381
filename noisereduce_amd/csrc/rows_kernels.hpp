// What the kernels of the rows path share (rows.hip: waveform and spectrum; rows_feat.hip: filterbank features): the row,
// noise and argument tables and the frame loader.  The feature kernels live in a translation unit of their own, so the
// code of rows.hip's kernels is what it was before they existed; rows.hip's host driver launches them through
// rw_feat_launch.  DESIGN sections 12, 14a and 14c.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "feat.hpp"
#include "tile_core.hpp"

namespace sg {

// ---- tables ------------------------------------------------------------------------------------------------------
struct RwRow {
  int64_t x_off;       // element of the source (x; backward: grad_out; spectrum backward: complex element of grad_spec)
                       // holding sample 0 (frame 0, bin 0) of the row
  int64_t len;         // readable samples (forward: lengths[i]; backward: H * (lengths[i] / H))
  int64_t T;           // frames: 1 + lengths[i] / H
  int64_t Lout;        // positions that receive a value (forward: H * (lengths[i] / H); backward: lengths[i])
  int64_t full;        // positions written, [Lout, full) with zeros (forward: H * (L / H); backward: L; spectrum forward: 0)
  int64_t out_off;     // element of out receiving position 0 (spectrum forward: complex element of frame 0, bin 0)
  int64_t frow;        // first row of this row's frames in the bits / magnitude / mask / segment fields
  int64_t mask_off;    // element of the caller's mask holding frame 0, band 0
  int32_t noise;       // local noise index (stationary)
  int32_t pad_;
};
struct RwNoise {
  int64_t off, len, T; // element of sample 0, readable samples, frames
  int64_t prow;        // first row in the noise power field
  int32_t in_x, pad_;  // 1: the row's own samples (xn = None)
};

struct RwArgs {
  const void* x; int in_dtype;
  const void* xn; int noise_dtype;
  void* out; int out_dtype;
  const RwRow* rows;
  const RwNoise* noises;
  const Tile* tiles;             // all tile lists, back to back
  int64_t t_np, n_np;            // noise power tiles (noise row, frames)
  int64_t t_nf, n_nf;            // noise final tiles (noise row, band block)
  int64_t t_dec, n_dec;          // frame tiles (row, frames)
  int64_t t_box, n_box;          // moving-mean tiles (row, band block)
  int64_t t_fs, n_fs;            // frequency smoothing tiles (row, frames)
  int64_t t_ap, n_ap;            // frame tiles of the apply stage
  int64_t t_ola, n_ola;          // output tiles (row, positions)
  double* Pn;                    // [noise rows][FS] float64 noise power
  double* T2n;                   // [local noise][FS] compare constant from the threshold alone
  double* thr;                   // [local noise][FS] thresholds (dB)
  unsigned long long* pmax;      // [rows][FS] band maxima of the row's power (bit patterns)
  unsigned long long* bits;      // [frame rows][wpr]
  float* mag;                    // [frame rows][FS] (non-stationary)
  float* sig;                    // [frame rows][FS] (non-stationary raw mask)
  float* R;                      // [frame rows][FS] frequency-smoothed mask
  float* seg;                    // [frame rows][n]
  float* mask_out;               // forward: nullptr or the caller's float[B][T][FS]
  const float* mask_in;          // backward: the mask of the forward call
  int kbox, bwd;
  TileConsts c;
};

// sum of w^2 over the row's OWN frames that cover output position p (torch.istft's envelope for a row of T frames)
__device__ __forceinline__ double rw_envelope(const RwArgs& A, int64_t T, int64_t p) {
  const int64_t e = p + A.c.padL;
  int64_t t_lo, t_hi;
  ola_span(e, A.c.n, A.c.H, T, &t_lo, &t_hi);
  return ola_envelope(A.c.wfull, e, A.c.H, t_lo, t_hi);
}

// sample g of a source of `len` readable samples starting at element off: 0 outside [0, len), never loaded there.
// Backward: the source is grad_out divided by the row's envelope.
__device__ __forceinline__ double rw_sample(const RwArgs& A, const void* src, int dt, int64_t off, int64_t len, int64_t T,
                                            int64_t g) {
  if (g < 0 || g >= len) return 0.0;
  double v = load_sample(src, dt, off + g);
  if (A.bwd) {
    const double norm = rw_envelope(A, T, g);
    v = norm > 1e-10 ? v / norm : v;
  }
  return v;
}

// window * frame t (samples [t H - padL, t H - padL + n)) into the team's buffer, forward transform, in place
template <int N>
__device__ __forceinline__ void rw_frame_fft(const RwArgs& A, const void* src, int dt, int64_t off, int64_t len, int64_t T,
                                             int64_t t, cx<double>* buf, const cx<double>* tw, int lane) {
  const int64_t s0 = t * A.c.H - A.c.padL;
  frame_fft<N>(buf, tw, lane, [&](int jj) -> double { return rw_sample(A, src, dt, off, len, T, s0 + jj) * A.c.wfull[jj]; });
}

// ---- the filterbank features (rows_feat.hip) -----------------------------------------------------------------------
// What the two feature kernels need beyond RwArgs, as a second kernel argument.
struct RwFeat {
  FeatBank bank;       // the handle's bank (sg_set_filterbank)
  const void* grad;    // backward: grad_feat [B][T][M] of the sample type
  double eps;
  double dead;         // forward: what a frame at or beyond T_i holds, 0 or ln(eps) (from the host: uniform, nothing to compute)
  int32_t power, take_log;
};

// k_rw_feat<N> (bwd false: the last forward launch, tiles over [0, T) of every row) or k_rw_feat_bwd<N> (backward launch
// 1 of 2, tiles over the rows' own frames) on A's apply tiles; N: the handle's half transform length
hipError_t rw_feat_launch(int N, bool bwd, const RwArgs& A, const RwFeat& Q, hipStream_t st);

}  // namespace sg
