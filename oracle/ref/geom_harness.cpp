// TEST INFRASTRUCTURE ONLY. C-linkage access to the REFERENCE's geometry.cpp, compiled unmodified as
// its own translation unit against oracle/ref/eigen_shim (oracle/Makefile: _ref/libref_geom.so).
// Each export builds a reference object from a flat record (the project's dt_shape_desc: doubles,
// floats and flags; `holes` is the hole array of a RectPrismWithCylinder) and calls one method.
// tools/gen_golden_geom.py turns the answers into tests/golden/geom_ref.npz; tests/test_oracle_geom.py
// compares them with oracle/oracle.c. Nothing of the reference is copied here.
#include <cfloat>
#include <cstring>
#include <memory>
#include <vector>

#include "geometry.h"

#include "../../include/dt.h"
#include "make_shape.h"

namespace {

int last_hit(const dt_shape_desc* s, const std::shared_ptr<GeoPrimitive>& p)
{
  if (s->type == DT_SHAPE_RECTPRISM_CYL) return static_cast<RectPrismWithCylinder*>(p.get())->lastHit;
  return -1;
}

}  // namespace

extern "C" {

// intersect: *t and *inside keep the caller's values where the reference leaves them unwritten.
// color_after = GeoPrimitive::color after the call, last_hit = RectPrismWithCylinder::lastHit after it
int ref_intersect(const dt_shape_desc* s, const dt_shape_desc* holes, const double* ray, const double* start,
                  float* t, int* inside, double* color_after, int* last_hit_out)
{
  auto p = make(s, holes);
  bool ins = *inside != 0;
  const bool hit = p->intersect(V(ray), V(start), *t, ins);
  *inside = ins ? 1 : 0;
  if (color_after) put(p->color, color_after);
  if (last_hit_out) *last_hit_out = last_hit(s, p);
  return hit ? 1 : 0;
}

int ref_shadow(const dt_shape_desc* s, const dt_shape_desc* holes, const double* ray, const double* start,
               float t_max)
{
  return make(s, holes)->intersectShadow(V(ray), V(start), t_max) ? 1 : 0;
}

// Sphere / Cylinder only (the base class's body is empty)
int ref_intersect_max(const dt_shape_desc* s, const double* ray, const double* start, float* t)
{
  return make(s, nullptr)->intersectMax(V(ray), V(start), *t) ? 1 : 0;
}

// Cylinder / CheckerCylinder records only
int ref_intersect_cap(const dt_shape_desc* s, const double* ray, const double* start, float* t, int* inside)
{
  auto c = make_cyl(s);
  bool ins = *inside != 0;
  const bool hit = c->intersectCap(V(ray), V(start), *t, ins);
  *inside = ins ? 1 : 0;
  return hit ? 1 : 0;
}

// getNorm(point). pre_ray != NULL: intersect(pre_ray, pre_start) on the same object first, so that the
// state it leaves (RectPrismWithCylinder::lastHit) is the one getNorm sees; *last_hit_out reports it.
// Returns 0, or 1 when the reference threw (RectPrismWithCylinder::getNorm off the three faces).
int ref_norm(const dt_shape_desc* s, const dt_shape_desc* holes, const double* point, const double* pre_ray,
             const double* pre_start, double* out, int* last_hit_out)
{
  auto p = make(s, holes);
  if (pre_ray) {
    float t = 0;
    bool ins = false;
    p->intersect(V(pre_ray), V(pre_start), t, ins);
  }
  if (last_hit_out) *last_hit_out = last_hit(s, p);
  try {
    put(p->getNorm(V(point)), out);
  } catch (const char*) {
    return 1;
  }
  return 0;
}

void ref_bounds(const dt_shape_desc* s, const dt_shape_desc* holes, double* lb, double* ub)
{
  VEC3 l, u;
  make(s, holes)->getBounds(l, u);
  put(l, lb);
  put(u, ub);
}

// getUV: returns 0, or 1 when the reference threw (a Triangle without UV vertices)
int ref_uv(const dt_shape_desc* s, const dt_shape_desc* holes, const double* point, double* uv, int* valid)
{
  auto p = make(s, holes);
  try {
    const VEC2 r = p->getUV(V(point), *valid);
    uv[0] = r[0];
    uv[1] = r[1];
  } catch (const char*) {
    return 1;
  }
  return 0;
}

// the members the constructor derives: center[3], axis[3], length, width, height, radius, objM[16]
// (row-major). Only the members the class's constructor sets are read (the others are uninitialised
// in the reference); the rest is reported as 0.
void ref_derived(const dt_shape_desc* s, const dt_shape_desc* holes, double* center, double* axis, float* lwh_r,
                 double* objM)
{
  auto p = make(s, holes);
  const int t = s->type;
  const bool cyl = t == DT_SHAPE_CYLINDER || t == DT_SHAPE_CHECKER_CYLINDER;
  const bool quad = t == DT_SHAPE_RECTANGLE || t == DT_SHAPE_CHECKERBOARD || t == DT_SHAPE_CHECKERBOARD_HOLE;
  const bool prism = t == DT_SHAPE_RECTPRISM_V2 || t == DT_SHAPE_RECTPRISM_CYL;
  for (int i = 0; i < 3; ++i) axis[i] = 0.0;
  for (int i = 0; i < 4; ++i) lwh_r[i] = 0.0f;
  for (int i = 0; i < 16; ++i) objM[i] = 0.0;
  put(p->center, center);
  if (cyl) put(p->axis, axis);
  if (quad || prism) { lwh_r[0] = p->length; lwh_r[1] = p->width; }
  if (prism) lwh_r[2] = p->height;
  if (cyl || t == DT_SHAPE_SPHERE) lwh_r[3] = p->radius;
  if (t == DT_SHAPE_CHECKER_CYLINDER || t == DT_SHAPE_RECTPRISM_CYL)
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) objM[4 * i + j] = p->objM(i, j);
}

void ref_fix_norm(const double* ray, const double* norm, double* out)
{
  VEC3 n = V(norm);
  fixNorm(V(ray), n);
  put(n, out);
}

void ref_build_cob(const double* z, double* out16)
{
  const MATRIX4 m = buildCOB(V(z));
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) out16[4 * i + j] = m(i, j);
}

void ref_barycentric3d(const double* p, const double* A, const double* B, const double* C, double* out)
{
  put(getBarycentricCoords3D(V(p), V(A), V(B), V(C)), out);
}

void ref_shortest_line(const double* P1, const double* P2, const double* P3, const double* P4, float* u1, float* u2)
{
  shortestLine(V(P1), V(P2), V(P3), V(P4), *u1, *u2);
}

int ref_segment_intersect(const double* A, const double* B, const double* ray, const double* origin, float* t)
{
  return segmentIntersect(V(A), V(B), V(ray), V(origin), *t) ? 1 : 0;
}

int ref_line_intersect(const double* l1, const double* o1, const double* l2, const double* o2, float* t)
{
  return lineIntersect(V(l1), V(o1), V(l2), V(o2), *t) ? 1 : 0;
}

// BoundingVolume over the one shape: its bounds, and intersect(ray, inv_ray, start) when ray != NULL
int ref_box(const dt_shape_desc* s, const dt_shape_desc* holes, int leaf, const double* ray, const double* inv_ray,
            const double* start, double* lb, double* ub)
{
  std::vector<std::shared_ptr<GeoPrimitive>> shapes;
  shapes.push_back(make(s, holes));
  BoundingVolume bv(std::vector<int>{0}, shapes, leaf != 0);
  if (lb) put(bv.lbound, lb);
  if (ub) put(bv.ubound, ub);
  if (!ray) return bv.leaf ? 1 : 0;
  return bv.intersect(V(ray), V(inv_ray), V(start)) ? 1 : 0;
}

}  // extern "C"
