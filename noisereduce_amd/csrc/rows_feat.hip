// Filterbank features of padded batches (sg_gate_features_rows / sg_gate_features_rows_backward): the two kernels that
// take the place of rows.hip's k_rw_spec and k_rw_spec_bwd, and their launcher.  Tables, loader and host driver are
// rows.hip's (rows_kernels.hpp); DESIGN section 14c.
#include <hip/hip_runtime.h>

#include "feat_sum.hpp"
#include "rows_kernels.hpp"

namespace sg {

// ---- the filterbank features of a padded batch (sg_gate_features_rows / sg_gate_features_rows_backward, DESIGN section
// 14c): k_rw_spec's frame and mask, reduced over the filters' supports while the frame is still in LDS.  What the two
// kernels need beyond RwArgs is a second kernel argument, so the kernels above keep theirs.  Power and log are run-time
// switches (uniform branches; one instantiation per frame length).
// Forward, the last launch, on k_rw_spec's tile list ([0, T) of every row).  A lane owns the bin pair (k, N - k), as
// mask_and_adjoint does: both bins come from buf[k] and buf[N - k] and both powers go back into the real parts of those
// two cells (bins 0 and N into the two halves of buf[0]), so the kernel asks for k_rw_spec's LDS and no more.  The mask
// is k_rw_spec's, call for call (the same bits), and the powers take it AS RETURNED (rounded to float32).  out:
// [B][T][M] of out_dtype, row i's frame 0 at element out_off; consecutive lanes store consecutive filters; frames at or
// beyond T_i load nothing and store 0 or ln(eps).
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) __attribute__((amdgpu_waves_per_eu(N <= 512 ? 3 : 2))) void k_rw_feat(RwArgs A, RwFeat Q) {
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_ap + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  const int M = Q.bank.M;
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    const int64_t frow = U.out_off + t * M;
    if (t >= U.T) {
      for (int m = fresh_lane(lane); m < M; m += NT) feat_store(A.out, A.out_dtype, frow + m, Q.dead);
      continue;
    }
    rw_frame_fft<N>(A, A.x, A.in_dtype, U.x_off, U.len, U.T, t, buf, tw, lane);
    const TimeTaps tp = time_taps(t, A.c.nt, U.T);
    const int64_t mrow = U.mask_off + t * A.c.FS;
    auto power_at = [&](int k) -> double {
      const double K = time_smooth(A.R, A.c.FS, [&](int64_t q) { return U.frow + q; }, tp, t, A.c.nt, k);
      const float m = (float)mask_stationary(A.c, K, tp.Et, k);
      if (A.mask_out) A.mask_out[mrow + k] = m;
      return feat_power(packed_bin<N>(buf, tw, k), (double)m, Q.power);
    };
    const int ln = fresh_lane(lane);
#pragma unroll 1
    for (int k = ln; k <= N / 2; k += NT) {
      if (k == 0) {
        const double p0 = power_at(0), pN = power_at(N);
        buf[lp<double>(0)] = {p0, pN};
      } else {
        const double pk = power_at(k), pn = (k != N - k) ? power_at(N - k) : 0.0;
        buf[lp<double>(k)].x = pk;
        if (k != N - k) buf[lp<double>(N - k)].x = pn;
      }
    }
    team_sync<SY>();
    const double pN = buf[lp<double>(0)].y;
    for (int m = ln; m < M; m += NT) {
      const double lin = feat_filter_sum(Q.bank, A.c.F, m, [&](int k) { return buf[lp<double>(k)].x; }, pN);
      feat_store(A.out, A.out_dtype, frow + m, Q.take_log ? log(lin + Q.eps) : lin);
    }
    team_sync<SY>();
  }
}

// Backward launch 1 of 2 (k_rw_ola's plain sum follows), on the tiles of the rows' own frames: frame t < T_i is
// transformed again from x (nothing of size B x T x F is read but the forward's mask), g'[m] = grad[m] (/ (lin[m] + eps),
// lin from a p row of its own: the spectrum is needed again after it) into an M-double LDS row, then per bin
// G[k] = (sum_m fb[k][m] g'[m] over the bin's hull) d(|X| m)^power / dX, formed from buf in place by the lane that owns
// the pair (k, N - k) and merged with mask 1 (mask_and_adjoint) -> window * un-normalised inverse into seg.
// grad_feat[i][T_i:] is never read.  LDS: launch_tile_kernel's + (M + (log ? N + 1 : 0)) doubles.
template <int N>
__global__ __launch_bounds__(tile_nt<N>()) void k_rw_feat_bwd(RwArgs A, RwFeat Q) {
  constexpr int NT = tile_nt<N>(), SY = tile_sy<N>();
  if ((int64_t)blockIdx.x >= A.n_ap) return;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cx<double>* tw = reinterpret_cast<cx<double>*>(smem);
  cx<double>* buf = tw + N;
  const int M = Q.bank.M;
  double* grow = reinterpret_cast<double*>(buf + lpn<double>(N));
  double* prow = grow + M;
  const int lane = threadIdx.x;
  const Tile tl = A.tiles[A.t_ap + blockIdx.x];
  const RwRow U = A.rows[tl.idx];
  const int64_t g0 = U.mask_off / A.c.FS * M;   // row i's frame 0 in grad_feat: i * T * M
  stage_tile_twiddles<N>(tw, A.c.tw);
  for (int64_t t = tl.a; t < tl.b; ++t) {
    const int64_t s0 = t * A.c.H - A.c.padL;
    frame_fft<N>(buf, tw, lane, [&](int jj) -> double {
      const int64_t g = s0 + jj;
      return ((g < 0 || g >= U.len) ? 0.0 : load_sample(A.x, A.in_dtype, U.x_off + g)) * A.c.wfull[jj];
    });
    const float* mrow = A.mask_in + U.mask_off + t * A.c.FS;
    if (Q.take_log) {   // lin[m] as the forward formed it
      for (int k = lane; k <= N; k += NT) prow[k] = feat_power(packed_bin<N>(buf, tw, k), (double)mrow[k], Q.power);
      team_sync<SY>();
    }
    const int64_t grad_row = g0 + t * M;
    for (int m = lane; m < M; m += NT) {
      double gm = A.in_dtype == 1 ? ((const double*)Q.grad)[grad_row + m] : (double)((const float*)Q.grad)[grad_row + m];
      if (Q.take_log) gm = gm / (feat_filter_sum(Q.bank, A.c.F, m, [&](int k) { return prow[k]; }, prow[N]) + Q.eps);
      grow[m] = gm;
    }
    team_sync<SY>();
    auto grad_at = [&](int k) -> cx<double> {
      const cx<double> X = packed_bin<N>(buf, tw, k);
      const double m = (double)mrow[k];
      const int2 hull = Q.bank.mhull[k];
      const float* __restrict__ row = Q.bank.fb + (int64_t)k * M;
      double gp = 0.0;
      for (int j = hull.x; j < hull.y; ++j) gp += (double)row[j] * grow[j];
      double s;
      if (Q.power == 2) {
        s = 2.0 * gp * m * m;
      } else {
        const double a = sqrt(X.x * X.x + X.y * X.y);
        s = a > 0.0 ? gp * m / a : 0.0;   // the derivative of |X| at 0 is defined as 0
      }
      return {s * X.x, s * X.y};
    };
    // (the merge's trailing barrier separates this frame's last read of g' and p from the next frame's writes)
    mask_and_adjoint<N>(buf, tw, lane, grad_at, [](int) -> double { return 1.0; }, A.c.wfull,
                        A.seg + (U.frow + t) * (int64_t)A.c.n);
  }
}

namespace {
// a feature kernel of geometry N: launch_tile_kernel's LDS plus `extra` bytes (the backward's g' and p rows)
template <int N>
hipError_t launch_feat_kernel(void (*kernel)(RwArgs, RwFeat), int64_t ntiles, size_t extra, hipStream_t st, const RwArgs& A,
                              const RwFeat& Q) {
  const size_t lds = (size_t)(N + lpn<double>(N)) * sizeof(cx<double>) + extra;
  return host::launch_lds_if(lds > 65536, kernel, tile_grid(ntiles), dim3(tile_nt<N>()), lds, st, A, Q);
}
// g'[M] and, with log, p[N + 1], in doubles: 24584 bytes at M = 1024, N = 2048 (94216 with the transform's, under 160 KB)
size_t feat_bwd_lds(int N, const RwFeat& Q) { return ((size_t)Q.bank.M + (Q.take_log ? (size_t)N + 1 : 0)) * sizeof(double); }
}  // namespace

hipError_t rw_feat_launch(int N, bool bwd, const RwArgs& A, const RwFeat& Q, hipStream_t st) {
  if (bwd) return dispatch_N(N, [&](auto n) { return launch_feat_kernel<n()>(k_rw_feat_bwd<n()>, A.n_ap, feat_bwd_lds(N, Q), st, A, Q); });
  return dispatch_N(N, [&](auto n) { return launch_feat_kernel<n()>(k_rw_feat<n()>, A.n_ap, 0, st, A, Q); });
}

}  // namespace sg
