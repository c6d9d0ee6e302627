// Irradiance queries at surface points: the one definition of what dt_points_irradiance (include/dt.h) adds to
// the probe generators of dt_occl.h, shared by the kernel (dt_points_irr.hip dt_points_irr_kernel) and the host
// exports dt_irradiance_gather_ray / dt_irradiance_cosine (dt_api_aux.cpp): the cosine weight, the gather probe
// and the light probe from a gather probe's hit. Both sides are built with -ffp-contract=off, so they run the
// same IEEE operations in the same order; nothing here calls libm beyond the sqrt of dt_math.h's normalized.
// The draws are dt_occl.h's (occl_words, occl_ball, occl_u01) under two more purposes.
#pragma once
#include "dt_occl.h"

namespace dtd {

enum { OCCL_P_GATHER = 8, OCCL_P_GLIGHT = 9 };   // dt_occl.h: 6 and 7; the render's node-0 draws: 1..5

// a launch's light record: the probe's OcclLight as it is, and the light's colour
struct IrrLight {
  OcclLight L;
  double color[3];
};

// dt_rays_occluded's void-ray rule for a direction: a non-finite component, or all zero
DT_HD bool irr_void_dir(dtm::V3 d)
{
  return !(isfinite(d.x) && isfinite(d.y) && isfinite(d.z)) || (d.x == 0 && d.y == 0 && d.z == 0);
}

// the cosine weight of a probe along dir at a surface with normal n (as given: no fixNorm, no normalisation)
DT_HD double irr_cosine(dtm::V3 n, dtm::V3 dir)
{
  if (irr_void_dir(dir)) return 0.0;
  return dtm::dmax(0.0, dtm::dot(n, dtm::normalized(dir)));
}

// Gather probe r of a sample: dir = n + u with u the direction of a ball point (cosine-weighted about a unit
// n), start = p + 1e-3 dir, as the light loop builds its box start. false: a void probe (no ball point within
// DT_OCCL_TRIES, or a void dir); then dir is the zero vector and start is p.
DT_HD bool irr_gather_ray(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, int r, dtm::V3 p, dtm::V3 n,
                          dtm::V3& start, dtm::V3& dir)
{
  using namespace dtm;
  const V3 ball = occl_ball(seed, frame, pixel, sample, OCCL_P_GATHER, r);
  const V3 d = add(n, normalized(ball));
  const bool live = !(ball.x == 0 && ball.y == 0 && ball.z == 0) && !irr_void_dir(d);
  dir = live ? d : v3(0, 0, 0);
  start = live ? add(p, mul(1e-3, d)) : p;
  return live;
}

// occl_light_dir under a purpose of the caller's and a generalised slot (dt_occl.h's sub-index layout with
// `slot` in the place of j): the light probe from the hit q of gather probe r towards light slot j draws at
// (OCCL_P_GLIGHT, slot = r * DT_OCCL_MAX_LIGHTS + j)
DT_HD dtm::V3 irr_light_dir(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, uint32_t purpose, int slot,
                            const OcclLight& L, dtm::V3 p)
{
  using namespace dtm;
  V3 T = v3a(L.center);
  if (L.type == DT_LIGHT_RECT) {
    uint32_t o[4];
    occl_words(seed, frame, pixel, sample, purpose, (uint32_t)(slot * 16), o);
    const double u0 = occl_u01(o[0], o[1]), u1 = occl_u01(o[2], o[3]);
    const V3 A = v3a(L.A);
    T = add(add(A, mul(u0, sub(v3a(L.B), A))), mul(u1, sub(v3a(L.D), A)));
  } else if (L.type == DT_LIGHT_SPHERE) {
    T = add(T, mul(L.radius, occl_ball(seed, frame, pixel, sample, purpose, slot)));
  }
  return sub(T, p);
}

}  // namespace dtd
