// dt_rays_resolve.h -- one output element of dt_rays_resolve (include/dt.h), the one definition that the host
// loop and the kernel of dt_rays_resolve.hip both call: the f64 sum of a pixel's rows from +0, left to right
// in ascending row order, the count of rows that count, one f64 division and one cast, exactly as
// dt_features_kernel forms albedo (S / n), depth (H ? S / H : 0) and coverage (H / n).
// No HIP include: tests/rays_resolve_host_check.cpp drives the host loop under ASan and UBSan, with no GPU.
#pragma once
#include <stdint.h>

#include "dt_scene_dev.h"

namespace rr {

enum { MEAN = 0, HIT_MEAN = 1 };   // DT_RESOLVE_MEAN, DT_RESOLVE_HIT_MEAN

// the call by value (a kernel argument); the tile fields are DParams' (dtd::slot_pixel)
struct Args {
  int64_t n_slots;   // dt_accum_doubles / 3
  int32_t n, width, mode;
  int32_t xRes, yRes, x0, y0, x1, y1, tw, th, rank, world, layout, tiles_x;
  int64_t n_owned_tiles, n_tiles;
  const double* values;   // n_slots * n rows of `width`
  const int32_t* shape;   // one per row, or null
  float* out;             // n_slots * width
  float* coverage;        // n_slots, or null
};

// element e = width * q + k: component k of slot q. A row with shape < 0 is skipped, which is what adding
// its value would be had it been written as zeros (the sum starts at +0 and never holds -0).
DT_HD void element(const Args& a, int64_t e)
{
  const int64_t q = e / a.width;
  const int k = (int)(e - q * a.width);
  int x, y;
  if (!dtd::slot_pixel(a, q, x, y)) return;
  const double* v = a.values + (q * a.n) * a.width + k;
  const int32_t* sh = a.shape ? a.shape + q * a.n : nullptr;
  double S = 0;
  int32_t H = 0;
  for (int i = 0; i < a.n; ++i) {
    if (sh && sh[i] < 0) continue;
    S = S + v[(int64_t)i * a.width];
    ++H;
  }
  const double n = (double)a.n, h = (double)H;
  a.out[e] = a.mode == HIT_MEAN ? (H > 0 ? (float)(S / h) : 0.0f) : (float)(S / n);
  if (a.coverage && k == 0) a.coverage[q] = (float)(h / n);
}

inline void host_loop(const Args& a)
{
  for (int64_t e = 0; e < a.n_slots * a.width; ++e) element(a, e);
}

}  // namespace rr
