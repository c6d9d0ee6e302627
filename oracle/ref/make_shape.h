// TEST INFRASTRUCTURE ONLY. Reference objects from flat records (the project's dt_shape_desc: doubles,
// floats and flags; `holes` is the hole array of a RectPrismWithCylinder), built with the reference's own
// constructors. Shared by geom_harness.cpp and shade_harness.cpp; geometry.h must be included first.
// Nothing of the reference is copied here.
#ifndef DT_REF_MAKE_SHAPE_H
#define DT_REF_MAKE_SHAPE_H

#include <memory>

#include "../../include/dt.h"

namespace {


VEC3 V(const double* a) { return VEC3(a[0], a[1], a[2]); }
void put(const VEC3& v, double* o) { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }

std::shared_ptr<Cylinder> make_cyl(const dt_shape_desc* s)
{
  return std::make_shared<Cylinder>(V(s->v[0]), V(s->v[1]), s->radius, V(s->color));
}

std::shared_ptr<GeoPrimitive> make(const dt_shape_desc* s, const dt_shape_desc* holes)
{
  const VEC3 col = V(s->color);
  // the light objects that are also shapes: their own constructors run the base class's default one
  // first (a rectangleLight keeps Rectangle()'s length = width = 1)
  if (s->type == DT_SHAPE_RECTANGLE && s->emit == DT_EMIT_RECT)
    return std::make_shared<rectangleLight>(V(s->v[0]), V(s->v[1]), V(s->v[2]), V(s->v[3]), col);
  if (s->type == DT_SHAPE_SPHERE && s->emit == DT_EMIT_SPHERE)
    return std::make_shared<sphereLight>(V(s->v[0]), s->radius, col);
  switch (s->type) {
    case DT_SHAPE_SPHERE: return std::make_shared<Sphere>(V(s->v[0]), s->radius, col);
    case DT_SHAPE_CYLINDER: return make_cyl(s);
    case DT_SHAPE_TRIANGLE: {
      auto t = std::make_shared<Triangle>(V(s->v[0]), V(s->v[1]), V(s->v[2]), col);
      if (s->flags & DT_F_MESH) { t->mesh = true; t->mesh_normal = V(s->mesh_normal); }
      if (s->flags & DT_F_UV_VERTS) {
        t->uv_verts = true;
        t->uvA = VEC2(s->uv[0][0], s->uv[0][1]);
        t->uvB = VEC2(s->uv[1][0], s->uv[1][1]);
        t->uvC = VEC2(s->uv[2][0], s->uv[2][1]);
      }
      return t;
    }
    case DT_SHAPE_RECTANGLE:
      return std::make_shared<Rectangle>(V(s->v[0]), V(s->v[1]), V(s->v[2]), V(s->v[3]), col);
    case DT_SHAPE_RECTPRISM_V2:
      return std::make_shared<RectPrismV2>(V(s->v[0]), V(s->v[1]), V(s->v[2]), V(s->v[3]), V(s->v[4]), V(s->v[5]),
                                           V(s->v[6]), V(s->v[7]), col);
    case DT_SHAPE_CHECKERBOARD:
      return std::make_shared<Checkerboard>(V(s->v[0]), V(s->v[1]), V(s->v[2]), V(s->v[3]), V(s->color1),
                                            V(s->color2), s->S);
    case DT_SHAPE_CHECKERBOARD_HOLE: {
      auto hole = std::make_shared<Rectangle>(V(s->v[4]), V(s->v[5]), V(s->v[6]), V(s->v[7]), col);
      auto c = std::make_shared<CheckerboardWithHole>(V(s->v[0]), V(s->v[1]), V(s->v[2]), V(s->v[3]), V(s->color1),
                                                      V(s->color2), s->S, hole);
      c->borderwidth = s->borderwidth;
      return c;
    }
    case DT_SHAPE_CHECKER_CYLINDER: {
      auto c = std::make_shared<CheckerCylinder>(V(s->v[0]), V(s->v[1]), s->radius, col, s->S);
      c->borderwidth = s->borderwidth;
      return c;
    }
    case DT_SHAPE_RECTPRISM_CYL: {
      auto p = std::make_shared<RectPrismWithCylinder>(V(s->v[0]), V(s->v[1]), V(s->v[2]), V(s->v[3]), V(s->v[4]),
                                                       V(s->v[5]), V(s->v[6]), V(s->v[7]), col);
      for (int i = 0; i < s->n_holes; ++i) p->holes.push_back(make_cyl(&holes[s->hole_first + i]));
      return p;
    }
  }
  return nullptr;
}

}  // namespace

#endif
