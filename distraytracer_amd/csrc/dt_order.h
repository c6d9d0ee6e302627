// Ray ordering: the one definition of the sort key of dt_ray_order (include/dt.h), shared by the host loop, the
// key kernel (dt_rayorder.hip) and the host export dt_ray_order_key. Both sides are built with
// -ffp-contract=off and correctly rounded division, so they run the same IEEE f64 operations in the same
// order; nothing here calls libm. tests/rayorder_ref.py restates it in numpy, bit for bit.
#pragma once
#include <stdint.h>

#include "../../include/dt.h"

#if defined(__HIPCC__)
#define DT_ORDER_HD __host__ __device__ __forceinline__
#else
#define DT_ORDER_HD inline
#endif

namespace dto {

DT_ORDER_HD bool order_finite(double x) { return x - x == 0.0; }   // inf - inf and NaN - NaN are NaN

// dt_trace_rays's void rule: a non-finite component, or an all-zero dir
DT_ORDER_HD bool order_void(const double* o, const double* d)
{
  const bool fin = order_finite(o[0]) && order_finite(o[1]) && order_finite(o[2]) && order_finite(d[0]) &&
                   order_finite(d[1]) && order_finite(d[2]);
  return !fin || (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0);
}

DT_ORDER_HD double order_abs(double x) { return x < 0.0 ? -x : (x == 0.0 ? 0.0 : x); }   // |-0| = +0

// the cell of a fraction f in [0, 1) at `bits` bits: !(f > 0) (a NaN included) -> 0, f >= 1 -> the last
DT_ORDER_HD uint32_t order_cell(double f, int bits)
{
  const uint32_t cells = 1u << bits;
  if (!(f > 0.0)) return 0u;
  if (f >= 1.0) return cells - 1u;
  return (uint32_t)(f * (double)cells);
}

// bit (stride*i + k) of the result is bit i of c
DT_ORDER_HD uint32_t order_spread(uint32_t c, int bits, int stride, int k)
{
  uint32_t m = 0;
  for (int i = 0; i < bits; ++i) m |= ((c >> i) & 1u) << (stride * i + k);
  return m;
}

// the key of one ray inside the box (lo, hi); void rays: 1u << B
DT_ORDER_HD uint32_t order_key(int ob, int db, int dir_major, const double* lo, const double* hi, const double* o,
                               const double* d)
{
  if (order_void(o, d)) return 1u << (3 * ob + 2 * db);
  uint32_t M3 = 0;
  for (int k = 0; k < 3; ++k) {
    const double e = hi[k] - lo[k];
    const double f = e > 0.0 ? (o[k] - lo[k]) / e : 0.0;
    M3 |= order_spread(order_cell(f, ob), ob, 3, k);
  }
  const double s = (order_abs(d[0]) + order_abs(d[1])) + order_abs(d[2]);
  double u = d[0] / s, v = d[1] / s;
  if (d[2] < 0.0) {
    const double fu = (1.0 - order_abs(v)) * (u >= 0.0 ? 1.0 : -1.0);
    const double fv = (1.0 - order_abs(u)) * (v >= 0.0 ? 1.0 : -1.0);
    u = fu;
    v = fv;
  }
  const double gu = u * 0.5 + 0.5, gv = v * 0.5 + 0.5;
  const uint32_t M2 = order_spread(order_cell(gu, db), db, 2, 0) | order_spread(order_cell(gv, db), db, 2, 1);
  return dir_major ? (M2 << (3 * ob)) | M3 : (M3 << (2 * db)) | M2;
}

}  // namespace dto
