// TEST INFRASTRUCTURE ONLY. C-linkage access to the REFERENCE's rayColor and generateBVH. The reference's
// render_final_project.cpp is included below from where it lies, unmodified (its main is renamed on the
// compiler's command line), against oracle/ref/eigen_shim, and linked with the reference's other
// translation units (oracle/Makefile: _ref/libref_shade.so, _ref/libref_shade_cr.so).
// ref_scene_set fills the reference's globals, `shapes` and `lights` from flat records (the project's
// dt_shape_desc / dt_light_desc / dt_globals) with the reference's constructors and builds `bvh` with its
// generateBVH; ref_load_texture is its loadTexture; ref_ray_color is one rayColor call tree.
// tools/gen_golden_shade.py turns the answers into tests/golden/shade_ref.npz. Nothing of the reference
// is copied here.
// With -DREF_TAPE (and ref/tape_random.h force-included, here and into a second compile of geometry.cpp)
// every uniform draw of rayColor's call tree comes from the tape set by ref_tape_set.
#include "render_final_project.cpp"

#include "../../include/dt.h"
#include "make_shape.h"

namespace {

const char* model_name(int m)
{
  switch (m) {
    case DT_MODEL_OREN_NAYAR: return "oren-nayar";
    case DT_MODEL_COOK_TORRANCE: return "cook-torrance";
    case DT_MODEL_RAW: return "raw";
  }
  return "lambert";
}

const char* material_name(int m)
{
  switch (m) {
    case DT_MAT_GLASS: return "glass";
    case DT_MAT_STEEL: return "steel";
    case DT_MAT_ALUMINUM: return "aluminum";
    case DT_MAT_WATER: return "water";
    case DT_MAT_LINOLEUM: return "linoleum";
    case DT_MAT_OTHER: return "other";
  }
  return "";
}

// pre-order, last child first: the order the reference's traversal stack pops (dt_bvh_node, include/dt.h)
void export_bvh(const shared_ptr<BoundingVolume>& b, int depth, dt_bvh_node* out, int cap, int* n, int* inds,
                int icap, int* ni)
{
  const int me = *n;
  const bool leaf = b->leaf;
  if (me < cap) {
    dt_bvh_node* o = &out[me];
    o->leaf = leaf ? 1 : 0;
    o->n_children = leaf ? 0 : (int)b->nodes.size();
    o->first_child = o->n_children ? me + 1 : -1;
    o->depth = depth;
    o->first_index = leaf ? *ni : -1;
    o->n_indices = leaf ? (int)b->indices.size() : 0;
    for (int a = 0; a < 3; ++a) { o->lbound[a] = b->lbound[a]; o->ubound[a] = b->ubound[a]; }
  }
  (*n)++;
  if (leaf) {
    for (int i : b->indices) {
      if (*ni < icap) inds[*ni] = i;
      (*ni)++;
    }
    return;
  }
  for (int c = (int)b->nodes.size() - 1; c >= 0; --c) export_bvh(b->nodes[c], depth + 1, out, cap, n, inds, icap, ni);
}

}  // namespace

extern "C" {

void ref_reset(void)
{
  shapes.clear();
  lights.clear();
  texture_frames.clear();
  texture_dims.clear();
  bvh.reset();
}

// the reference's loadTexture (helpers.h): 0, or 1 when it threw
int ref_load_texture(const char* path)
{
  try {
    loadTexture(path);
  } catch (...) {
    return 1;
  }
  return 0;
}

int ref_scene_set(const dt_shape_desc* sh, int n_shapes, const dt_shape_desc* holes, const dt_light_desc* li,
                  int n_lights, const dt_globals* g)
{
  shapes.clear();
  lights.clear();
  bvh.reset();
  reflect = g->reflect != 0;
  nogloss = g->nogloss != 0;
  refr_air = g->refr_air;
  refr_glass = g->refr_glass;
  phong = g->phong;
  brdf_samples = g->brdf_samples;
  max_depth = g->max_depth;
  c_isect = g->c_isect;
  c_trav = g->c_trav;
  for (int i = 0; i < n_shapes; ++i) {
    const dt_shape_desc* s = &sh[i];
    shared_ptr<GeoPrimitive> p = make(s, holes);
    if (!p) return -1;
    // what the scene builders set on a shape after its constructor (scene.h)
    p->model = model_name(s->model);
    p->reflect_params.material = material_name(s->material);
    p->reflect_params.roughness = s->roughness;
    p->reflect_params.glossy = (s->flags & DT_F_GLOSSY) != 0;
    p->reflect_params.refr = VEC2(s->refr[0], s->refr[1]);
    p->motion = (s->flags & DT_F_MOTION) != 0;
    p->texture = (s->flags & DT_F_TEXTURE) != 0;
    p->tex_frame = s->tex_frame;
    p->bordercolor = V(s->bordercolor);
    if (s->emit == DT_EMIT_NONE) p->light = (s->flags & DT_F_LIGHT) != 0;
    shapes.push_back(p);
  }
  for (int i = 0; i < n_lights; ++i) {
    const dt_light_desc* l = &li[i];
    shared_ptr<LightPrimitive> lp;
    if (l->type == DT_LIGHT_POINT) {
      lp = make_shared<pointLight>(V(l->center), V(l->color));
    } else if (l->type == DT_LIGHT_SPHERE) {
      shared_ptr<sphereLight> sl;
      if (l->shape_index >= 0) sl = dynamic_pointer_cast<sphereLight>(shapes[l->shape_index]);
      else sl = make_shared<sphereLight>(V(l->center), l->radius, V(l->color));
      if (!sl) return -2;
      sl->baxis = V(l->baxis);
      lp = sl;
    } else if (l->type == DT_LIGHT_RECT) {
      shared_ptr<rectangleLight> rl;
      if (l->shape_index >= 0) rl = dynamic_pointer_cast<rectangleLight>(shapes[l->shape_index]);
      else {
        const VEC3 C = V(l->B) + (V(l->D) - V(l->A));
        rl = make_shared<rectangleLight>(V(l->A), V(l->B), C, V(l->D), V(l->color));
      }
      if (!rl) return -2;
      lp = rl;
    } else {
      return -3;
    }
    lp->color = V(l->color);
    lp->center = V(l->center);
    lights.push_back(lp);
  }
  if (n_shapes > 0) {
    vector<int> all(n_shapes);
    for (int i = 0; i < n_shapes; ++i) all[i] = i;
    bvh = generateBVH(all);
  }
  return 0;
}

// one rayColor call tree; colour (unclamped) starts at 0. Returns 0, or 1 when the reference threw a
// value (a bare `throw;` with no exception in flight terminates the process: the generator keeps its
// scenes clear of those)
int ref_ray_color(const double* ray, const double* start, int depth, float k, double* color, int* hit_out,
                  int* in_motion_out)
{
  VEC3 col(0, 0, 0);
  bool hit = false, in_motion = false;
  int rc = 0;
  try {
    rayColor(V(ray), V(start), depth, col, hit, in_motion, k);
  } catch (...) {
    rc = 1;
  }
  color[0] = col[0]; color[1] = col[1]; color[2] = col[2];
  *hit_out = hit ? 1 : 0;
  *in_motion_out = in_motion ? 1 : 0;
  return rc;
}

// the tree generateBVH built, in dt_bvh_build's export format
int ref_bvh(dt_bvh_node* nodes, int cap, int* indices, int index_cap, int* n_nodes, int* n_indices)
{
  int n = 0, ni = 0;
  if (bvh) export_bvh(bvh, 0, nodes, cap, &n, indices, index_cap, &ni);
  *n_nodes = n;
  *n_indices = ni;
  return 0;
}

#ifdef REF_TAPE
// the one definition of the draw tape (ref/tape_random.h)
const double* ref_tape_values = nullptr;
int ref_tape_len = 0, ref_tape_pos = 0, ref_tape_over = 0;

// the next draws are values[0 .. n-1] (the caller keeps them alive); rewinds and clears the over-ask flag
void ref_tape_set(const double* values, int n)
{
  ref_tape_values = values;
  ref_tape_len = n;
  ref_tape_pos = 0;
  ref_tape_over = 0;
}

// draws asked for since ref_tape_set, the ones past the end included
int ref_tape_consumed(void) { return ref_tape_pos; }

// 1 when the reference asked for more than it was given (each such draw got 0.5)
int ref_tape_overasked(void) { return ref_tape_over; }
#endif

}  // extern "C"
