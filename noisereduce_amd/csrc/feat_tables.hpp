// Host side of sg_set_filterbank: the transpose and the two support tables of a dense [F][M] filterbank.  Plain C++ (no
// HIP), so that a host test can compile it alone.
#pragma once
#include <cmath>
#include <cstdint>

namespace sg {

// fb: float[F][M].  fbT: float[M][F].  khull: 2 ints per filter, the hull [k_lo, k_hi) of its non-zero bins (0, 0 for an
// all-zero filter).  mhull: 2 ints per bin, the hull [m_lo, m_hi) of the filters that are non-zero there (0, 0 for none).
// Returns false when an entry is not finite (the tables are then unspecified).
inline bool feat_tables(const float* fb, int F, int M, float* fbT, int32_t* khull, int32_t* mhull) {
  for (int m = 0; m < M; ++m) khull[2 * m] = khull[2 * m + 1] = 0;
  for (int k = 0; k < F; ++k) {
    int lo = 0, hi = 0;
    for (int m = 0; m < M; ++m) {
      const float v = fb[(int64_t)k * M + m];
      if (!std::isfinite(v)) return false;
      fbT[(int64_t)m * F + k] = v;
      if (v == 0.0f) continue;
      if (hi == 0) lo = m;
      hi = m + 1;
      if (khull[2 * m + 1] == 0) khull[2 * m] = k;
      khull[2 * m + 1] = k + 1;
    }
    mhull[2 * k] = lo;
    mhull[2 * k + 1] = hi;
  }
  return true;
}

}  // namespace sg
