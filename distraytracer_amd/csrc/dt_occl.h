// Occlusion feature buffers: the one definition of the two probe-ray generators of dt_render_occlusion
// (include/dt.h), shared by the kernel (dt_occlusion.hip dt_occlusion_kernel) and the host exports
// dt_occlusion_ao_ray / dt_occlusion_light_ray (dt_api.cpp). Both sides are built with -ffp-contract=off,
// so they run the same IEEE operations in the same order; nothing here calls libm.
// The draws are the render's counter RNG (Philox4x32-10, key (seed, frame), counter (pixel, sample,
// node 0, (purpose << 24) | sub)) under two purposes of their own, restated here for host and device:
// the kernel's own philox() is device code with a key trick for the trace kernels' register budget.
#pragma once
#include <stdint.h>

#include "../../include/dt.h"
#include "dt_math.h"

namespace dtd {

enum { OCCL_P_AO = 6, OCCL_P_LIGHT = 7 };   // the render's node-0 draws use purposes 1..5

// what a probe needs of a dt_light_desc; at most DT_OCCL_MAX_LIGHTS of them travel with a launch
struct OcclLight {
  int32_t type, shape_index;
  double radius;   // (double) of the descriptor's float
  double center[3], A[3], B[3], D[3];
};

DT_HD void occl_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t o[4])
{
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

DT_HD void occl_words(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, uint32_t purpose, uint32_t sub,
                      uint32_t o[4])
{
  occl_philox(pixel, sample, 0u, (purpose << 24) | sub, seed, (uint32_t)frame, o);
}

DT_HD double occl_u01(uint32_t w0, uint32_t w1)
{
  return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) * (1.0 / 9007199254740992.0);
}

// A point of the unit ball by rejection from the cube: try a = 0 .. DT_OCCL_TRIES-1 draws the words at
// sub = base*16 + a; the first with s <= 1 is the point, none: the origin. word * 2^-31 - 1 is exact.
DT_HD dtm::V3 occl_ball(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, uint32_t purpose, int base)
{
  for (int a = 0; a < DT_OCCL_TRIES; ++a) {
    uint32_t o[4];
    occl_words(seed, frame, pixel, sample, purpose, (uint32_t)(base * 16 + a), o);
    const double x = (double)o[0] * (1.0 / 2147483648.0) - 1.0;
    const double y = (double)o[1] * (1.0 / 2147483648.0) - 1.0;
    const double z = (double)o[2] * (1.0 / 2147483648.0) - 1.0;
    const double s = (x * x + y * y) + z * z;
    if (s <= 1.0) return dtm::v3(x, y, z);
  }
  return dtm::v3(0, 0, 0);
}

// ambient-occlusion probe r of a hitting sample: towards a point of the ball of radius R resting on the
// surface at the hit, R * (n + v); v = -n gives the zero vector, a void ray
DT_HD dtm::V3 occl_ao_dir(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, int r, float ao_radius, dtm::V3 n)
{
  const dtm::V3 v = occl_ball(seed, frame, pixel, sample, OCCL_P_AO, r);
  return dtm::mul((double)ao_radius, dtm::add(n, v));
}

// light probe of slot j from p: towards the point light's centre, a point of the rectangle light's frame
// or a point of the sphere light's volume
DT_HD dtm::V3 occl_light_dir(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, int j, const OcclLight& L,
                             dtm::V3 p)
{
  using namespace dtm;
  V3 T = v3a(L.center);
  if (L.type == DT_LIGHT_RECT) {
    uint32_t o[4];
    occl_words(seed, frame, pixel, sample, OCCL_P_LIGHT, (uint32_t)(j * 16), o);
    const double u0 = occl_u01(o[0], o[1]), u1 = occl_u01(o[2], o[3]);
    const V3 A = v3a(L.A);
    T = add(add(A, mul(u0, sub(v3a(L.B), A))), mul(u1, sub(v3a(L.D), A)));
  } else if (L.type == DT_LIGHT_SPHERE) {
    T = add(T, mul(L.radius, occl_ball(seed, frame, pixel, sample, OCCL_P_LIGHT, j)));
  }
  return sub(T, p);
}

}  // namespace dtd
