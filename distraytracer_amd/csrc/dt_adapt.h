// Adaptive sampling: the one definition of "this pixel has converged", shared by the selection
// kernel (dt_kernels.hip dt_adapt_flag_kernel) and the host export dt_adapt_converged (dt_api.cpp).
// Both sides are built with -ffp-contract=off, so they run the same IEEE operations in the same order.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DT_ADAPT_HD __host__ __device__ __forceinline__
#else
#define DT_ADAPT_HD inline
#endif

namespace dtd {

// a pixel may stop only with this many samples (one 64-sample chunk, the unit a window is made of)
#define DT_ADAPT_MIN_COUNT 64u

// s1: the pixel's three sums of sample colours (accum), s2: of their squares (accum2), count: the
// samples in them. thr2 = (tol / 255)^2, the variance of the mean allowed per channel (tol: the
// standard error in grey levels of the 0..255 output). Every comparison is <=: a NaN sum never
// converges (the pixel keeps sampling), a d that rounding makes slightly negative does.
DT_ADAPT_HD bool adapt_converged(const double s1[3], const double s2[3], uint32_t count, double thr2,
                                 int32_t min_samples)
{
  if (count < DT_ADAPT_MIN_COUNT || (int64_t)count < (int64_t)min_samples) return false;
  const double n = (double)count;
  for (int c = 0; c < 3; ++c) {
    const double d = s2[c] - (s1[c] * s1[c]) / n;
    const double v = d / (n * (n - 1.0));   // variance of the mean
    if (!(v <= thr2)) return false;
  }
  return true;
}

}  // namespace dtd
