// Specular-path feature buffers: the one definition of "the guide ray goes on from this hit, and with
// which ray", shared by the kernel (dt_features_path.hip dt_features_path_kernel) and the host export
// dt_guide_bounce (dt_api.cpp). Both sides are built with -ffp-contract=off, so they run the same IEEE
// operations in the same order.
// It restates the trace kernel's bounce arithmetic (dt_kernels.hip run_pass: the mirror ray, the glass
// branch; oracle.c rayColor) without the Fresnel weights: a pure function of the hit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dt.h"
#include "dt_math.h"

namespace dtd {

enum { DT_GUIDE_STOP = 0, DT_GUIDE_REFLECT = 1, DT_GUIDE_REFRACT = 2 };

// in: the normalised ray, n: the fixNorm'ed normal, p: the hit point. STOP: this surface is the guide
// (refl_err: the mirror ray left on the wrong side, the render's reflect_errors). Otherwise the next
// segment's unnormalised direction and start.
// Glass follows transmission; total internal reflection (chk < 0) falls through to the mirror rule. At
// normal incidence sin_theta is 0 and b = 1 / sin_theta is inf: next_dir comes out non-finite, a void ray.
DT_HD int guide_bounce(int32_t reflect, int32_t nogloss, float refr_air, float refr_glass, int32_t material,
                       uint32_t flags, int32_t inside, dtm::V3 in, dtm::V3 n, dtm::V3 p, dtm::V3& next_dir,
                       dtm::V3& next_start, bool& refl_err)
{
  using namespace dtm;
  refl_err = false;
  const float eps = 1e-3f;
  const bool refl_mat = material == DT_MAT_GLASS || material == DT_MAT_STEEL || material == DT_MAT_ALUMINUM ||
                        material == DT_MAT_WATER || material == DT_MAT_LINOLEUM;
  const bool specular = reflect != 0 && refl_mat && !((flags & DT_F_GLOSSY) && !nogloss);
  if (!specular) return DT_GUIDE_STOP;
  if (material == DT_MAT_GLASS) {
    const float cos_theta = (float)dot(n, neg(in));
    const double ct = (double)cos_theta;
    const float sin_theta = (float)sqrt(1 - ct * ct);
    const float r1 = inside ? refr_glass : refr_air, r2 = inside ? refr_air : refr_glass;
    const float q = r1 / r2;
    const double qd = (double)q, dn = dot(in, n);
    const float chk = (float)(1 - (qd * qd) * (1 - dn * dn));
    if (chk >= 0) {
      const float a = q * sin_theta;
      const float b = 1 / sin_theta;
      const float sq = sqrtf(chk);
      next_dir = sub(mul(a, mul(b, add(in, mul(cos_theta, n)))), mul(sq, n));
      next_start = add(p, mul(eps, in));
      return DT_GUIDE_REFRACT;
    }
  }
  const V3 refl = sub(in, mul(2 * dot(n, in), n));
  const double rn = dot(refl, n);
  if (rn <= 0) {
    refl_err = true;
    return DT_GUIDE_STOP;
  }
  if (rn <= eps) return DT_GUIDE_STOP;
  next_dir = refl;
  next_start = add(p, mul(eps, refl));
  return DT_GUIDE_REFLECT;
}

}  // namespace dtd
