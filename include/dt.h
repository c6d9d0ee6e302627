/*
 * dt.h — C-ABI boundary of the MI355X-native distraytracer render loop.
 *
 * The reference has no FFI: its render loop is the C++ function
 *     void renderImage(const string& filename, const int frame,
 *                      const function<void(float)> sceneBuilder)
 *         (/root/reference/render_final_project.cpp:965)
 * reading ~60 mutable globals (render_final_project.cpp:48-137, re-declared
 * extern in helpers.h:32-84 and scene.h:17-101), plus the sky-only
 *     void renderImageCloud(const string& filename, const float frame)
 *         (render_final_project.cpp:1224).
 * This header is the drop-in replacement for that boundary: plain C structs,
 * plain pointers, integer status codes, no exceptions and no exit() across it.
 *
 *   reference                                   this ABI
 *   ------------------------------------------  -----------------------------------
 *   globals render_final_project.cpp:48-137     dt_globals (1:1 field mapping)
 *   vector<shared_ptr<GeoPrimitive>> shapes     dt_scene_desc.shapes (dt_shape_desc)
 *   vector<shared_ptr<LightPrimitive>> lights   dt_scene_desc.lights (dt_light_desc)
 *   texture_frames / texture_dims (helpers.h)   dt_scene_desc.textures
 *   generateBVH (helpers.h:381) at renderImage  dt_scene_create (same topology)
 *   renderImage pixel loop (…cpp:1031-1218)     dt_render
 *   renderImageCloud (…cpp:1224-1279)           dt_render_sky
 *   printf+throw / exit         status codes + dt_stats counters
 *   scene.h builders (buildFinal, …)            dt_build_scene (host input generation)
 *
 * Output layout is the reference's ppmOut (render_final_project.cpp:986,1215-1217):
 * float[3*W*H], index 3*((H-1-y)*W + x) + c, value clamp(c)*255.0f.
 */
#ifndef DT_H
#define DT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: dt_tiles ownership by hashed tile groups (dtd::tile_of) with equal-size slabs,
 *    dt_scene_prepare / dt_scene_upload / dt_accel_info_build, RectPrismWithCylinder
 *    (DT_SHAPE_RECTPRISM_CYL with the dt_scene_desc.holes array) */
/* 3: dt_stats.donations / donate_overflow (DFS work sharing inside a wave, DT_DONATE) */
/* 4: dt_scene_set_kernel (the trace-kernel choice per scene, not through the environment) */
/* 5: dt_accel_info.features */
/* 6: dt_trace_build (the trace-kernel build a render launches, and the features it covers) */
/* 7: dt_render_repeat_async; dt_accel_info.sg_sub_blocks / sg_sub_nodes / sg_sub_hash */
/* 8: dt_render_repeat_async removed (a measurement stand-in with no product caller) */
/* (still 8, new exports only, no struct changed: dt_accum_doubles, dt_window_check, dt_render_window,
 *    dt_render_window_async, dt_resolve -- progressive rendering) */
/* (still 8, new exports only, no struct changed: dt_adapt_converged, dt_render_window_adaptive,
 *    dt_render_window_adaptive_async, dt_resolve_adaptive, dt_adapt_select_ms -- adaptive sampling) */
/* (still 8, new exports only, no struct changed: dt_render_features and its dt_features argument --
 *    first-hit feature buffers) */
/* (still 8, new exports and one new struct, no struct changed: dt_denoise_params_default,
 *    dt_denoise_workspace_floats, dt_denoise and its dt_denoise_params -- preview denoising) */
/* (still 8, new exports and one new struct, no struct changed: dt_variance, dt_denoise_var_params_default,
 *    dt_denoise_var_workspace_floats, dt_denoise_var and its dt_denoise_var_params -- variance-guided
 *    preview denoising) */
/* (still 8, new exports and new structs, no struct changed: dt_camera_get and its dt_camera,
 *    dt_temporal_params_default, dt_reproject and its dt_temporal_params and dt_history -- temporal reuse
 *    for animation previews) */
/* (still 8, new exports and one new struct, no struct changed: dt_trace_rays and its dt_ray_hits,
 *    dt_rays_occluded -- ray queries: closest hit and visibility for caller-supplied rays) */
/* (still 8, new exports and one new struct, no struct changed: dt_render_mattes and its dt_mattes,
 *    dt_matte_mask -- object mattes: ranked per-pixel group coverage) */
/* (still 8, new exports and one new struct, no struct changed: dt_upsample_params_default, dt_upsample and
 *    its dt_upsample_params -- guided upsampling of previews) */
/* (still 8, new exports only, no struct changed: dt_guide_bounce, dt_render_features_path -- specular-path
 *    feature buffers: guides seen through mirrors and glass) */
/* (still 8, new exports and two new structs, no struct changed: dt_occlusion_params_default,
 *    dt_render_occlusion and its dt_occlusion_params and dt_occlusion, dt_occlusion_ao_ray,
 *    dt_occlusion_light_ray -- occlusion feature buffers: ambient occlusion and per-light visibility) */
/* (still 8, new exports only, no struct changed: dt_points_occlusion -- occlusion queries at surface points
 *    the caller supplies, for baking) */
/* (still 8, new exports and one new struct, no struct changed: dt_ray_order_params_default, dt_ray_order_key,
 *    dt_ray_order_workspace_bytes, dt_ray_order and its dt_ray_order_params, dt_permute_rows -- ray ordering:
 *    sort caller-supplied rays into coherent waves) */
/* (still 8, one new export and one new struct, no struct changed: dt_trace_rays_multi and its
 *    dt_ray_multihits -- multi-hit ray queries: the k nearest surfaces along caller-supplied rays) */
/* (still 8, new exports only, no struct changed: dt_camera_rays_rows, dt_camera_rays, dt_rays_resolve --
 *    camera rays as arrays, and per-ray answers resolved back to pixels) */
/* (still 8, new exports and two new structs, no struct changed: dt_rays_transmittance and its
 *    dt_ray_transmittance, dt_points_occlusion_glass and its dt_occlusion_panes -- transmittance queries:
 *    shadow probes that pass through glass) */
/* (still 8, one new export and one new struct, no struct changed: dt_trace_rays_path and its dt_ray_paths --
 *    path ray queries: caller-supplied rays followed through mirrors and glass) */
/* (still 8, new exports and two new structs, no struct changed: dt_points_irradiance and its
 *    dt_irradiance_params and dt_irradiance, dt_irradiance_gather_ray, dt_irradiance_cosine -- irradiance
 *    queries at surface points: cosine-weighted direct light and one diffuse gather bounce, for light baking) */
#define DT_ABI_VERSION 8

/* ---- status codes ------------------------------------------------------- */
#define DT_OK              0
#define DT_E_INVALID      -1   /* bad argument / descriptor */
#define DT_E_NO_DEVICE    -2   /* no HIP device or HIP runtime error */
#define DT_E_OOM          -3
#define DT_E_UNSUPPORTED  -4   /* shape/light type the device path does not implement */
#define DT_E_IO           -5   /* builder data file missing */
#define DT_E_LIMIT        -6   /* recursion stack / scene size above compiled limit */

/* ---- shapes (geometry.h:28-256) ----------------------------------------- */
enum dt_shape_type {
  DT_SHAPE_SPHERE           = 1, /* Sphere            geometry.cpp:83-210   */
  DT_SHAPE_CYLINDER         = 2, /* Cylinder          geometry.cpp:212-432  */
  DT_SHAPE_TRIANGLE         = 3, /* Triangle          geometry.cpp:434-602  */
  DT_SHAPE_RECTANGLE        = 4, /* Rectangle         geometry.cpp:604-782  */
  DT_SHAPE_RECTPRISM_V2     = 5, /* RectPrismV2       geometry.cpp:784-948  */
  DT_SHAPE_CHECKERBOARD     = 6, /* Checkerboard      geometry.cpp:2248-2341 */
  DT_SHAPE_CHECKERBOARD_HOLE= 7, /* CheckerboardWithHole geometry.cpp:2344-2561 */
  DT_SHAPE_CHECKER_CYLINDER = 8, /* CheckerCylinder   geometry.cpp:2563-2630 */
  DT_SHAPE_RECTPRISM_CYL    = 9  /* RectPrismWithCylinder geometry.cpp:1467-1821 (axis-aligned
                                    box of the 8 vertices with cylinder holes; holes[] below) */
};

/* GeoPrimitive::model (render_final_project.cpp:894-948) */
enum dt_model {
  DT_MODEL_PHONG         = 0,  /* any other string, e.g. "lambert": Lambert + Phong(phong) */
  DT_MODEL_OREN_NAYAR    = 1,  /* "oren-nayar"    */
  DT_MODEL_COOK_TORRANCE = 2,  /* "cook-torrance" */
  DT_MODEL_RAW           = 3   /* "raw"           */
};

/* reflect_params.material; refl_materials = {glass, steel, aluminum, water,
 * linoleum} (render_final_project.cpp:64) */
enum dt_material {
  DT_MAT_NONE = 0, DT_MAT_GLASS = 1, DT_MAT_STEEL = 2, DT_MAT_ALUMINUM = 3,
  DT_MAT_WATER = 4, DT_MAT_LINOLEUM = 5, DT_MAT_OTHER = 6
};

/* GeoPrimitive::name values with behaviour attached to them */
enum dt_emit {
  DT_EMIT_NONE   = 0,
  DT_EMIT_SPHERE = 1,  /* name "spherelight"    (render_final_project.cpp:777) */
  DT_EMIT_RECT   = 2   /* name "rectanglelight" (render_final_project.cpp:783) */
};

/* flag bits */
#define DT_F_LIGHT       (1u << 0)  /* GeoPrimitive::light                 */
#define DT_F_MOTION      (1u << 1)  /* GeoPrimitive::motion                */
#define DT_F_TEXTURE     (1u << 2)  /* GeoPrimitive::texture               */
#define DT_F_GLOSSY      (1u << 3)  /* reflect_params.glossy               */
#define DT_F_NAMED_RECT  (1u << 4)  /* name == "rectangle" (motion-blur shift, cpp:1113) */
#define DT_F_MESH        (1u << 5)  /* Triangle::mesh                      */
#define DT_F_UV_VERTS    (1u << 6)  /* Triangle::uv_verts                  */

typedef struct dt_shape_desc {
  int32_t  type;        /* dt_shape_type */
  int32_t  model;       /* dt_model      */
  int32_t  material;    /* dt_material   */
  int32_t  emit;        /* dt_emit       */
  uint32_t flags;       /* DT_F_*        */
  int32_t  tex_frame;   /* index into dt_scene_desc.textures, -1 none */
  float    roughness;   /* reflect_params.roughness */
  float    radius;      /* Sphere / Cylinder radius */
  float    S;           /* checker square side      */
  float    borderwidth; /* checker border width     */
  float    length;      /* Rectangle::length = |B-A| (float member) */
  float    width;       /* Rectangle::width  = |D-A| (float member) */
  double   refr[2];     /* reflect_params.refr (VEC2) */
  double   color[3];    /* GeoPrimitive::color       */
  double   color1[3];   /* Checkerboard colors       */
  double   color2[3];
  double   bordercolor[3];
  double   center[3];   /* GeoPrimitive::center (BVH centroid, emissive falloff) */
  /* geometry, by type:
   *   SPHERE            v[0] = center
   *   CYLINDER / CHECKER_CYLINDER  v[0] = c1, v[1] = c2
   *   TRIANGLE          v[0..2] = A,B,C
   *   RECTANGLE / CHECKERBOARD     v[0..3] = A,B,C,D
   *   RECTPRISM_V2      v[0..7] = A..H
   *   CHECKERBOARD_HOLE v[0..3] = A,B,C,D ; v[4..7] = hole rectangle A,B,C,D
   *   RECTPRISM_CYL     v[0..7] = A..H ; holes: dt_scene_desc.holes[hole_first ..
   *                     hole_first + n_holes) (RectPrismWithCylinder::holes, geometry.h:196) */
  double   v[8][3];
  double   mesh_normal[3];
  double   uv[3][2];    /* Triangle uvA, uvB, uvC */
  int32_t  hole_first;  /* RECTPRISM_CYL: first entry in dt_scene_desc.holes */
  int32_t  n_holes;     /* RECTPRISM_CYL: number of holes (0 for every other type) */
} dt_shape_desc;

/* ---- lights (geometry.h:279-307, geometry.cpp:2745-2849) ---------------- */
enum dt_light_type {
  DT_LIGHT_POINT  = 1,  /* pointLight::sampleRay = center - p          */
  DT_LIGHT_SPHERE = 2,  /* sphereLight::sampleRay = sampled point (Q11) */
  DT_LIGHT_RECT   = 3   /* rectangleLight::sampleRay = A + x(B-A) + y(D-A) - p */
};

typedef struct dt_light_desc {
  int32_t type;          /* dt_light_type */
  int32_t shape_index;   /* shapes[] entry that IS this light object (skipped by its own
                            shadow test, cpp:812-818), or -1 */
  float   radius;        /* sphere light radius */
  float   _pad;
  double  center[3];     /* LightPrimitive::center */
  double  color[3];      /* LightPrimitive::color  */
  double  baxis[3];      /* sphereLight::baxis     */
  double  A[3], B[3], D[3]; /* rectangle light sampling frame */
} dt_light_desc;

/* texture_frames[i] / texture_dims[i] (helpers.h:92-113): 8-bit RGB as decoded by
 * stb_image; the renderer uses byte/255.0 as the reference does. */
typedef struct dt_texture_desc {
  int32_t        width;
  int32_t        height;
  int32_t        channels;   /* bytes per texel (>=3), first 3 used */
  int32_t        _pad;
  const uint8_t* pixels;     /* row-major, width*height*channels */
} dt_texture_desc;

typedef struct dt_scene_desc {
  int32_t                n_shapes;
  int32_t                n_lights;
  int32_t                n_textures;
  int32_t                _pad;
  const dt_shape_desc*   shapes;
  const dt_light_desc*   lights;
  const dt_texture_desc* textures;
  /* Cylinder holes of RECTPRISM_CYL shapes (type CYLINDER records: v[0] = c1, v[1] = c2, radius,
   * color; geometry.cpp:227-240). They are not shapes of the scene: only their prism tests them. */
  int32_t                n_holes;
  int32_t                _pad2;
  const dt_shape_desc*   holes;
} dt_scene_desc;

/* ---- globals (render_final_project.cpp:48-137) -------------------------- */
typedef struct dt_globals {
  int32_t xRes, yRes;                    /* 52-53 */
  double  eye[3], lookingAt[3], up[3];   /* 56-58 */
  float   aspect, near_plane, fov;       /* 59-61 (aspect frozen at 1920/1080, Q3) */
  float   aperture, focal_length;        /* 62-63 */
  int32_t use_model, nogloss;            /* 64-65 */
  float   refr_air, refr_glass;          /* 69-70 */
  int32_t max_depth;                     /* 71 */
  float   phong;                         /* 76 */
  double  default_col[3];                /* 77 */
  float   c_isect, c_trav;               /* 81-82 */
  int32_t antialias_samples, brdf_samples, blur_samples, frame_range; /* 85-88 */
  int32_t frame_prism, frame_cloud, frame_blur, frame_start;  /* 112-115 */
  int32_t frame_move1, frame_move2, frame_sculp, total;       /* 116-119 */
  float   far_dist, move_per_frame, tot_move, accel_t;        /* 120-123 */
  double  cap_center[3];                                       /* 124 */
  double  sundir[3];                     /* 127 */
  int32_t perlin_cloud;                  /* 128 */
  float   saturation, clouddist, cloudhoff; /* 129-131 */
  double  sun_outer[3], sun_inner[3], sun_core[3], bluesky[3], redsky[3]; /* 132-136 */
  int32_t reflect;                       /* 138 */
  uint32_t seed;                         /* counter-RNG seed (reference RNG is unseeded, F7) */
} dt_globals;

/* ---- tiles / multi-GPU partition ---------------------------------------- */
enum dt_out_layout {
  DT_OUT_IMAGE = 0,  /* full ppmOut layout float[3*xRes*yRes]; only owned pixels written */
  DT_OUT_SLAB  = 1   /* owned tiles packed in tile order: dt_slab_floats() floats */
};

typedef struct dt_tiles {
  int32_t x0, y0, x1, y1;    /* pixel window [x0,x1) x [y0,y1); x1<=0 means full width/height */
  int32_t tile_w, tile_h;    /* tile size (<=0: 32x32) */
  int32_t rank, world;       /* the window's tiles (row-major) fall into groups of `world`
                                consecutive tiles; each rank owns one tile of every group, the
                                ranks rotated by a hash of the group (dt_scene_dev.h tile_of) */
  int32_t layout;            /* dt_out_layout */
  int32_t _pad;
} dt_tiles;

/* ---- stats --------------------------------------------------------------- */
typedef struct dt_stats {
  uint64_t pixels;            /* pixels rendered                                 */
  uint64_t samples;           /* pixel-samples (W*H*spp) = metric numerator      */
  uint64_t rays;              /* rayColor invocations with depth>0 (incl. blur)  */
  uint64_t shadow_rays;       /* light samples tested for occlusion              */
  uint64_t sky_pixels;        /* pixels that needed cloudColor                   */
  uint64_t uv_out_of_range;   /* reference terminates here (cpp:870-877), we count */
  uint64_t glossy_exhausted;  /* >10 invalid glossy resamples (cpp:724-740)      */
  uint64_t spherelight_exhausted; /* geometry.cpp:2785-2789                      */
  uint64_t prism_norm_fallback;   /* RectPrismV2::getNorm off-surface (geometry.cpp:895);
                                     RectPrismWithCylinder::getNorm's throw (geometry.cpp:1819-1820) */
  uint64_t reflect_errors;    /* refl.n <= 0 (cpp:631-638)                       */
  uint64_t nan_pixels;
  uint64_t tex_fetches;       /* texel reads (algorithmic bytes) */
  uint64_t stack_overflows;   /* DFS entries dropped (device stack limit); 0 when validated */
  uint64_t box_tests;         /* lane-level BVH slab tests      (these three: diagnostic builds */
  uint64_t prim_tests;        /* lane-level primitive tests       with -DDT_WORK_COUNTERS only; */
  uint64_t wave_node_visits;  /* wave-level BVH node visits        0 otherwise)  */
  double   kernel_ms;         /* device time of the render kernels (hipEvents, same stream) */
  double   trace_kernel_ms;   /* device time of the dominant (trace) kernel alone */
  uint64_t donations;         /* pending DFS subtrees run by another lane of the wave (work sharing) */
  uint64_t donate_overflow;   /* work-sharing records dropped (per-wave pool full); 0 when validated */
} dt_stats;

/* ---- API ------------------------------------------------------------------ */
typedef struct dt_scene dt_scene;   /* opaque: device-resident scene + BVH */

int         dt_abi_version(void);
const char* dt_last_error(void);

/* fill with the reference's initial global values (render_final_project.cpp:48-137) */
void dt_globals_default(dt_globals* g);

/* Build the reference-topology BVH (helpers.h:381-472) on the host and upload the
 * scene to the current HIP device. */
int  dt_scene_create(const dt_scene_desc* desc, const dt_globals* g, dt_scene** out);
void dt_scene_destroy(dt_scene* s);
/* dt_scene_create in two halves. dt_scene_prepare does the host work (flatten, BVH, acceleration
 * structures, primary-ray lists) and touches no device memory, so it can run on a worker thread
 * while a render fills the GPU; dt_scene_upload allocates and uploads (a few ms). A render of a
 * scene that was prepared but not uploaded uploads it first. No reference counterpart: the
 * reference builds its BVH inside renderImage (render_final_project.cpp:965-1030). */
int  dt_scene_prepare(const dt_scene_desc* desc, const dt_globals* g, dt_scene** out);
int  dt_scene_upload(dt_scene* s);

/* Which trace kernel the renders of scene s launch. No reference counterpart (the reference has
 * one loop, render_final_project.cpp:1031-1218); every choice renders the same bits.
 *   DT_KERNEL_AUTO     the DT_DONATE environment variable decides (default: the product kernels)
 *   DT_KERNEL_PRODUCT  the product kernels (dt_trace_kernel / _w5 by spp)
 *   DT_KERNEL_DONATE   DFS work sharing inside the wave (dt_trace_kernel_dn) where it applies
 *                      (max_depth <= 11, brdf_samples <= 6, no RectPrismWithCylinder)
 * A caller choosing per frame (tools/animate.py) sets it on that frame's scene instead of writing
 * the process environment while another thread builds the next scene. Calls on one scene must not
 * overlap across host threads (this one included). */
#define DT_KERNEL_AUTO     0
#define DT_KERNEL_PRODUCT  1
#define DT_KERNEL_DONATE   2
int  dt_scene_set_kernel(dt_scene* s, int32_t kernel);

/* BVH export for parity tests: node i = {first child or -1, n_children, first shape,
 * n_shapes, leaf, lbound[3], ubound[3]} in the reference's push order. */
typedef struct dt_bvh_node {
  int32_t first_child, n_children, first_index, n_indices, leaf, depth;
  double  lbound[3], ubound[3];
} dt_bvh_node;
int  dt_scene_bvh(const dt_scene* s, dt_bvh_node* nodes, int32_t cap,
                  int32_t* indices, int32_t index_cap, int32_t* n_nodes, int32_t* n_indices);

/* generateBVH (helpers.h:381-472) alone, on the host, no device needed: same export format
 * as dt_scene_bvh. */
int  dt_bvh_build(const dt_scene_desc* desc, const dt_globals* g, dt_bvh_node* nodes, int32_t cap,
                  int32_t* indices, int32_t index_cap, int32_t* n_nodes, int32_t* n_indices);

/* The acceleration structures dt_scene_create would upload for (desc, g), built on the host
 * only (no device): counts and FNV-1a content hashes, for A/B checks of build options
 * (DT_SG_BLOCK, DT_SG_ORDER, ...). No reference counterpart: the reference walks its own BVH
 * (helpers.h:381-472, geometry.cpp:2657-2740) and has no shadow grid. */
typedef struct dt_accel_info {
  int32_t n_nodes, n_fnodes, n_bnodes, boxes_ordered;
  int32_t sg_lights, sg_dim[3];
  int64_t sg_cells, sg_tree_cells, sg_list_pool, sg_list_entries;
  uint64_t nodes_hash, fnodes_hash, bnodes_hash;
  uint64_t sg_hash;            /* cells + list pool in storage order */
  uint64_t sg_contents_hash;   /* each cell's list as a sorted set (order-free) */
  float bump_pad, sg_reach;
  int64_t sg_umbra_cells;      /* (light, cell) records whose every segment to the light is occluded */
  uint32_t features;           /* the scene's trace-kernel feature mask: bit t for shape type t,
                                  12 sphere lights/emitters, 13 Oren-Nayar, 14 glass, 15 rectangle
                                  lights/emitters (the build dt_render launches) */
  int32_t sg_sub_blocks;       /* shadow-grid block subtrees (DT_SG_SUBTREE=1) and their nodes */
  int64_t sg_sub_nodes;
  uint64_t sg_sub_hash;        /* FNV-1a over the block records and subtree nodes */
} dt_accel_info;
int dt_accel_info_build(const dt_scene_desc* desc, const dt_globals* g, dt_accel_info* info);

/* The trace-kernel build dt_render launches for (desc, g) at `frame` with the automatic kernel
 * choice (the DT_* environment switches apply as in dt_render), decided on the host only (no
 * device): its kernel name (NUL-terminated, truncated to name_cap), the scene's feature mask (as
 * dt_accel_info.features) and the mask the build was compiled for (dt_kernels.hip DT_FEATURES).
 * dt_render refuses (DT_E_INVALID) a scene with a feature outside its build's mask rather than
 * launching code that has that case compiled out. No reference counterpart: the reference has one
 * CPU render loop (render_final_project.cpp:965-1222). */
int dt_trace_build(const dt_scene_desc* desc, const dt_globals* g, int32_t frame, char* name, int32_t name_cap,
                   uint32_t* scene_features, uint32_t* build_features);

/* number of floats a DT_OUT_SLAB output needs for (g, tiles) */
int64_t dt_slab_floats(const dt_globals* g, const dt_tiles* tiles);
int64_t dt_slab_floats_max(const dt_globals* g, const dt_tiles* tiles); /* max over ranks */

/* renderImage's pixel loop (render_final_project.cpp:1031-1218) for `frame`.
 * out: host pointer (out_on_device=0) or device pointer (1). stream: hipStream_t or NULL.
 * Synchronous unless dt_render_async is used. */
int dt_render(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
              float* out, int32_t out_on_device, void* stream, dt_stats* stats);
/* enqueue only (device output, no host sync, stats device-side until dt_collect_stats).
 * A scene's launches must be ordered: keep one scene object per stream (two frames in flight take
 * two scene objects, as bench.py does). A scene keeps two launch records and two counter blocks
 * on the device and alternates between them; each launch clears the other block, and a record is
 * uploaded only when its bytes change, so repeated renders of a still frame enqueue nothing but
 * their kernels. dt_collect_stats reports the scene's last launch. */
int dt_render_async(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                    float* out_device, void* stream);
int dt_collect_stats(const dt_scene* s, void* stream, dt_stats* stats);

/* ---- progressive rendering: sample windows into a resident accumulator ----
 * No reference counterpart: the reference takes a frame whole (render_final_project.cpp:1031-1218).
 * A window [begin, end) is the samples begin..end-1 of every owned pixel; a window render adds them,
 * in sample order, onto an f64 accumulator on the device, and dt_resolve turns the accumulator into
 * the usual output at any time (the mean of the samples added so far).
 *
 * The accumulator has one double per float of the output, in the output's layout (element i of the
 * accumulator belongs to element i of the image): 3*xRes*yRes in ppmOut indexing for DT_OUT_IMAGE,
 * dt_slab_floats for DT_OUT_SLAB. 24 bytes per pixel. dt_accum_doubles: its length (host only;
 * < 0: invalid globals or tiles). */
int64_t dt_accum_doubles(const dt_globals* g, const dt_tiles* tiles);
/* The window rules, host only; spp = int(sqrt(antialias_samples))^2:
 *   0 <= begin < end <= spp;
 *   spp >= 64: begin % 64 == 0, and end % 64 == 0 or end == spp (whole 64-sample chunks, the unit
 *              one wave traces);
 *   spp <  64: the only window is [0, spp).
 * DT_E_INVALID with a dt_last_error naming the rule otherwise. */
int dt_window_check(const dt_globals* g, int32_t begin, int32_t end);
/* Render the window onto accum_device (dt_accum_doubles doubles, device memory). Synchronous; stats
 * reports this window alone: samples = pixels * (end - begin), rays etc. of the window's samples,
 * nan_pixels 0 (dt_resolve counts them). A null scene, a null accumulator or a bad window:
 * DT_E_INVALID before any device work.
 * THE CALLER ORDERS THE WINDOWS. The accumulator equals the one-shot render's per-pixel sums (and
 * dt_resolve with n_samples = spp dt_render's output, bit for bit) only for ascending, gap-free
 * windows starting at 0 on a zeroed accumulator: f64 addition is not associative, and each window
 * continues the pixel's chain from the value it finds. One window at a time per accumulator. */
int dt_render_window(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                     int32_t begin, int32_t end, double* accum_device, void* stream, dt_stats* stats);
/* enqueue only, as dt_render_async; dt_collect_stats then reports the window */
int dt_render_window_async(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                           int32_t begin, int32_t end, double* accum_device, void* stream);
/* out[i] = clamp01((float)(accum[i] / n_samples)) * 255.0f for every element of the accumulator: the
 * division and store of dt_render's epilogue (cpp:1213-1217) on the sums of the first n_samples
 * samples. accum and out on the same side: host (on_device=0, a plain loop) or device (1, a kernel
 * on `stream`). Elements of pixels the rank does not own (DT_OUT_IMAGE with a tile share) are 0 in
 * a zeroed accumulator and resolve to 0. nan_pixels (optional): pixels with a NaN channel; on the
 * device the call is synchronous when it is asked for and only enqueues otherwise. */
int dt_resolve(const dt_globals* g, const dt_tiles* tiles, const double* accum, int32_t n_samples,
               float* out, int32_t on_device, void* stream, uint64_t* nan_pixels);

/* ---- adaptive sampling: converged pixels stop between sample windows ----
 * No reference counterpart. Beside the accumulator the caller owns two more device buffers:
 *   accum2: dt_accum_doubles doubles, indexed like the accumulator; element i is the left-to-right
 *           f64 sum of c*c over the sample colours c whose sum is accum[i];
 *   count:  uint32, dt_accum_doubles / 3 entries; entry q (the pixel of accum[3q..3q+2]) is the
 *           number of samples added to that pixel so far.
 * 52 bytes per pixel in all, zeroed before the first window. A pixel is LIVE at a window
 * [begin, end) iff count[q] == begin: there is no other state. A live pixel is traced unless it has
 * converged. With n = (double)count, per channel c:
 *   d = S2[c] - (S1[c] * S1[c]) / n;   v = d / (n * (n - 1.0));      (variance of the mean)
 *   converged iff v <= thr2 for all three channels, thr2 = (tol / 255.0) * (tol / 255.0),
 * and only when count >= min_samples and count >= 64. tol: the standard error allowed, in grey
 * levels of the 0..255 output, finite and >= 0. The comparisons are <=: a NaN sum never converges, a
 * d that rounding makes slightly negative does. min_samples >= spp: nothing ever stops.
 * dt_adapt_converged: the rule on host values, 1 or 0 (DT_E_INVALID for a bad tol). */
int dt_adapt_converged(const double s1[3], const double s2[3], uint32_t count, double tol, int32_t min_samples);
/* dt_render_window over the live, unconverged pixels only: a selection on the device lists them in
 * ascending item order and the window's trace launch runs over that list; each traced pixel gets its
 * samples added to accum and accum2 and count[q] = end. Windows as dt_window_check; with spp < 64
 * the one window traces every pixel. stats.pixels: the pixels traced in this window,
 * stats.samples = pixels * (end - begin), rays etc. of those samples. A pixel that is never stopped
 * receives dt_render_window's chain of adds: its accumulator bits are the one-shot render's.
 * A null scene or buffer, a bad tol or a bad window: DT_E_INVALID before any device work. */
int dt_render_window_adaptive(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                              int32_t begin, int32_t end, double* accum_device, double* accum2_device,
                              uint32_t* count_device, double tol, int32_t min_samples, void* stream,
                              dt_stats* stats);
int dt_render_window_adaptive_async(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                                    int32_t begin, int32_t end, double* accum_device, double* accum2_device,
                                    uint32_t* count_device, double tol, int32_t min_samples, void* stream);
/* dt_resolve with every pixel divided by its own count:
 * out[3q+k] = clamp01((float)(accum[3q+k] / count[q])) * 255.0f, 0 where count[q] == 0. */
int dt_resolve_adaptive(const dt_globals* g, const dt_tiles* tiles, const double* accum, const uint32_t* count,
                        float* out, int32_t on_device, void* stream, uint64_t* nan_pixels);
/* the device time of the selection kernels of the scene's last adaptive window launch (waits for them) */
int dt_adapt_select_ms(const dt_scene* s, float* ms);

/* diagnostic builds (-DDT_STAMPS): per-phase cycle sums of the last render; zeros otherwise */
int dt_debug_counters(const dt_scene* s, uint64_t* out, int32_t n);
/* diagnostic builds (-DDT_ITEM_TIMES=2) with DT_ITEM_COSTS=1 in the environment: the last launch's
 * per-item durations (100 MHz clock ticks) by queue code (chunk items: pixel item * chunks + chunk),
 * min(n, items) of them into out; returns the number of items (0: none recorded; < 0: an error code) */
int64_t dt_debug_item_costs(const dt_scene* s, uint32_t* out, int64_t n);
/* numerics check: the device kernels' normalisation of n VEC3s (Eigen normalized(), dt_math.h),
 * host arrays of 3n doubles; synchronous */
int dt_debug_normalize(const double* in, double* out, int64_t n);
/* numerics check of the device kernels' division of a VEC3 by one scalar (dt_math.h divs): n vectors
 * in[3i..3i+2] and divisors den[i]; out: four blocks of 3n doubles, a / den by the shared-reciprocal
 * path, a / den by three plain divisions, normalized(a) by either; fallback[0], fallback[1]: the
 * vectors whose shared a / den and whose shared normalisation divided plainly after all (their three
 * scaled divisors differ). Host arrays; synchronous. A diagnostic added under ABI 8. */
int dt_debug_vdiv(const double* in, const double* den, double* out, uint64_t* fallback, int64_t n);
/* numerics check of the device kernels' fused length and normalisation (dt_math.h vnorm_fused): n vectors
 * in[3i..3i+2]; out: two blocks of 4n doubles, (|a|, a / |a|) per vector by the fused path and by plain
 * sqrt and three plain divisions (a itself where dot(a, a) > 0 does not hold); fallback[0]: the vectors
 * whose fused call took the plain branch (out of range). Host arrays; synchronous. A diagnostic added
 * under ABI 8. */
int dt_debug_vnorm(const double* in, double* out, uint64_t* fallback, int64_t n);
/* the device light records' sampling frame for (desc, g), on the host only (no device): per light 15
 * doubles A, B, D, B - A, D - A as the kernels read them; cap: the lights out has room for. A diagnostic
 * added under ABI 8. */
int dt_debug_light_edges(const dt_scene_desc* desc, const dt_globals* g, double* out, int32_t cap);

/* Intersection micro-benchmark (2^24 primary rays of the C3 camera). rayColor's first
 * step (render_final_project.cpp:491-538: BVH gather + closest hit) for primary rays of the globals'
 * camera (getDOFSamples + getPerspEyeRay, 195-210 / 1044-1072), as dt_render takes it. Ray r:
 * q = r / 8 -> pixel q mod (xRes*yRes) in raster order, sample r mod 8 + 8 * (q div (xRes*yRes)).
 * hit_shape[i], hit_t[i] for ray first_ray + i: the closest shape (-1: none) and its t (FLT_MAX:
 * none); host (out_on_device=0) or device (1) arrays of n_rays. Synchronous; kernel_ms (optional):
 * the kernel's HIP-event time. Scenes with a RectPrismWithCylinder: DT_E_UNSUPPORTED. It shares the
 * scene's primary-ray lists, which depend on the camera and resolution only (not on a tile split):
 * called with the globals of the scene's renders it rebuilds nothing. Its launch record, counters
 * and events are its own, but like every call on one scene it must not overlap another call on
 * that scene from another host thread. */
int dt_intersect_primary(const dt_scene* s, const dt_globals* g, int32_t frame, int64_t first_ray,
                         int64_t n_rays, int32_t* hit_shape, float* hit_t, int32_t out_on_device,
                         void* stream, float* kernel_ms);

/* First-hit feature buffers ("AOVs": the per-pixel companions of the colour image a denoiser, a
 * compositor or an object picker reads). No reference counterpart. For the samples 0 .. n_samples-1 of
 * every owned pixel (n_samples as dt_window_check(g, 0, n_samples): whole 64-sample chunks or spp; with
 * spp < 64, spp) the render's own primary ray is traced to its closest hit, exactly as dt_render's
 * root ray: RNG pixel y*xRes+x, sample i, key (seed, frame); in dt_intersect_primary's numbering ray
 * ((i/8)*W*H + y*W + x)*8 + i%8. A miss adds nothing; a hit on shape h at t along the unnormalised ray:
 *   p      = eye_sample + (double)t * ray
 *   normal = fixNorm(normalized(ray), getNorm(p))              world space
 *   colour = the colour intersect() leaves in the shape (a Checkerboard's square, else the shape's);
 *            for a DT_F_TEXTURE shape, by getUV(p): type 1 with a texture the texel / 255.0 (the light
 *            loop's index arithmetic and clamp; counted in tex_fetches), type 2 bordercolor, type 0
 *            unchanged; a uv outside [0,1] (types 1, 2) counts uv_out_of_range
 *   d      = (double)t * |ray|
 * All sums are f64, left to right in ascending sample order. With A, N, D the sums over the H hitting
 * samples of n = n_samples:
 *   albedo[3q+k] = (float)(A[k] / n)      normal[3q+k] = (float)(N[k] / n)      (premultiplied by
 *   coverage[q]  = (float)(H / n)         depth[q] = H ? (float)(D / H) : 0      coverage, no clamp,
 *   shape[q]     = the shape sample 0 hit (-1: none)                             not renormalised)
 * q is the pixel's slot in the output layout: its colour occupies floats 3q..3q+2 of dt_render's output
 * (DT_OUT_IMAGE and DT_OUT_SLAB alike; the entry of dt_render_window_adaptive's count). Planes hold
 * dt_accum_doubles(g, tiles) (albedo, normal) or a third of that (depth, coverage, shape) elements, all
 * host (out_on_device=0) or all device (1); a NULL plane is not wanted. Only owned pixels are written.
 * On frames >= frame_prism the planes describe the unshifted hit, not the motion-blur re-traces.
 * Synchronous. stats (optional): pixels produced, samples = rays = pixels * n, tex_fetches,
 * uv_out_of_range, prism_norm_fallback, kernel_ms; everything else 0. Like dt_intersect_primary it has
 * a launch record, counters and events of its own and shares only the scene's primary-ray lists: a
 * render of the scene afterwards is unaffected. A null scene, globals or out, an out with every plane
 * NULL or a bad n_samples: DT_E_INVALID; a scene with a RectPrismWithCylinder: DT_E_UNSUPPORTED; both
 * before any device work. */
typedef struct dt_features {      /* each plane optional (NULL: not wanted); all on one side */
  float*   albedo;    /* 3 per pixel, indexed exactly like dt_render's output (element 3q+k) */
  float*   normal;    /* 3 per pixel, same indexing; world space */
  float*   depth;     /* 1 per pixel, entry q */
  float*   coverage;  /* 1 per pixel, entry q */
  int32_t* shape;     /* 1 per pixel, entry q */
} dt_features;

int dt_render_features(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                       int32_t n_samples, const dt_features* out, int32_t out_on_device,
                       void* stream, dt_stats* stats);

/* ---- specular-path feature buffers: guides seen through mirrors and glass ----
 * No reference counterpart. dt_render_features describes the first hit, so for a mirror or a pane of glass
 * every guide is the flat reflector's and says nothing of what it shows. Here a sample's guide ray follows
 * perfect specular bounces, and the planes describe the first surface that is not a perfect reflector or
 * refractor. The planes are a dt_features: dt_denoise, dt_denoise_var and dt_upsample take them as they are.
 *
 * The bounce rule (dt_guide_bounce; csrc/dt_guide.h, one definition for host and kernel): the render's own
 * mirror and glass arithmetic (rayColor) without the Fresnel weights, a pure function of the hit. With
 * in = normalized(ray), n = the fixNorm'ed normal, p = the hit point, eps = 1e-3f:
 *   specular := g->reflect && material in {GLASS, STEEL, ALUMINUM, WATER, LINOLEUM}
 *               && !((flags & DT_F_GLOSSY) && !g->nogloss)
 *   not specular                -> 0 (stop: this surface is the guide)
 *   GLASS: cos_theta = (float)dot(n, -in); sin_theta = (float)sqrt(1 - (double)cos_theta^2);
 *          q = r1 / r2 with (r1, r2) = inside ? (refr_glass, refr_air) : (refr_air, refr_glass);
 *          chk = (float)(1 - (double)q^2 * (1 - dot(in, n)^2))
 *          chk >= 0 -> next_dir = (q * sin_theta) * ((1 / sin_theta) * (in + cos_theta * n)) - sqrtf(chk) * n,
 *                      next_start = p + eps * in                                   -> 2 (refract)
 *          otherwise the mirror rule (total internal reflection)
 *   refl = in - (2 * dot(n, in)) * n; rn = dot(refl, n)
 *          rn <= 0 -> 0 (the call below counts it in reflect_errors); rn <= eps -> 0;
 *          else next_dir = refl, next_start = p + eps * refl                       -> 1 (reflect)
 * At normal incidence on glass 1 / sin_theta is inf and next_dir is not finite: a void ray (dt_trace_rays).
 * next_dir and next_start are written only for 1 and 2. A null argument: DT_E_INVALID. No device work. */
int dt_guide_bounce(const dt_globals* g, int32_t material, uint32_t flags, int32_t inside, const double in[3],
                    const double n[3], const double p[3], double next_dir[3], double next_start[3]);

/* dt_render_features_path: samples, rays, slots q, layouts, sides, staging, the window rule for n_samples and
 * "only owned pixels are written" are exactly dt_render_features's. Per sample, segment k = 0, 1, ...
 * (segment 0 is the primary ray (ray, eye_sample)):
 *   the segment (dir_k, start_k) is traced to its closest hit as dt_trace_rays specifies it (shift 0, dir
 *   unnormalised): shape h_k, t_k, inside_k. A void ray (dt_trace_rays's rule) is not traced. A void ray or
 *   a miss ends the sample as a MISS, which adds nothing to A, N, D, H below. On a hit
 *     L   = L + (double)t_k * |dir_k|                      (f64, from 0)
 *     p_k = start_k + (double)t_k * dir_k,   n_k = fixNorm(normalized(dir_k), getNorm(p_k))
 *   and if k < max_bounces and the bounce rule at (h_k's material and flags, inside_k, normalized(dir_k), n_k,
 *   p_k) says reflect or refract, the sample goes on with its next ray. Otherwise it ENDS ON h_k: its
 *   colour is dt_render_features's colour rule at (h_k, p_k), its normal n_k (world space, not un-reflected:
 *   the normal of what the mirror shows), its depth L, the length of the whole path.
 * Planes, from the f64 left-to-right sums over the samples in ascending order, n = n_samples, H = the samples
 * that ended on a surface, B = the sum over all n samples of the segments followed beyond the first:
 *   albedo = (float)(A / n)   normal = (float)(N / n)   coverage = (float)(H / n)
 *   depth = H ? (float)(D / H) : 0       shape[q] = the shape sample 0 ended on (-1: a miss)
 *   bounces[q] = (float)(B / n)          (optional; 1 per pixel, entry q, on the side of the planes)
 * max_bounces = 0 is dt_render_features bit for bit in every plane (bounces is 0).
 * stats (optional): pixels, samples = pixels * n, rays = the segments traced, reflect_errors, tex_fetches,
 * uv_out_of_range and prism_norm_fallback (every segment's hit takes its normal), kernel_ms; everything else 0.
 * Errors as dt_render_features (bounces counts as a plane: with it, every pointer of out may be NULL), with a
 * dt_last_error starting "dt_render_features_path: ", plus max_bounces outside 0..DT_GUIDE_MAX_BOUNCES:
 * DT_E_INVALID; a scene with a RectPrismWithCylinder: DT_E_UNSUPPORTED; all before any device work.
 * Synchronous, with a launch record, counters and events of its own; it shares only the scene's primary-ray
 * lists, and a render of the scene afterwards is unaffected.
 * Limits. Glossy reflectors (DT_F_GLOSSY with nogloss = 0) stop the chain: they are rough, and their own
 * surface is the right guide. Glass follows transmission only, never its reflection. dt_reproject must keep
 * first-hit guides: its world point is the first hit's, and a path's depth and normal do not reproject.
 * Cost: after the first bounce a wave visits the union of its lanes' nodes, so a later segment costs nearer
 * dt_trace_rays's scattered figure than its camera-order one. */
#define DT_GUIDE_MAX_BOUNCES 8
int dt_render_features_path(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                            int32_t n_samples, int32_t max_bounces /* 0..DT_GUIDE_MAX_BOUNCES */,
                            const dt_features* out, float* bounces /* optional, 1 per pixel */,
                            int32_t out_on_device, void* stream, dt_stats* stats);

/* ---- object mattes: ranked per-pixel group coverage ----
 * No reference counterpart. What a compositor cuts antialiased mattes from (the Cryptomatte-style answer):
 * for every owned pixel the `layers` groups that cover most of it, ranked, each with its share of the
 * pixel's samples, taken from the render's own primary rays, so that the mattes line up with the colour
 * image edge for edge, depth of field included.
 * Rays: the samples 0 .. n_samples-1 of every owned pixel (n_samples as for dt_render_features:
 * dt_window_check(g, 0, n_samples)), each the render's own primary ray (RNG pixel y*xRes+x, sample i, key
 * (seed, frame)) traced to its closest hit at shift 0 on every frame, exactly as dt_render_features traces
 * it; in dt_intersect_primary's numbering ray ((i/8)*W*H + y*W + x)*8 + i%8.
 * Group: a hit on shape h has group group_of_shape ? group_of_shape[h] : h. group_of_shape is always a
 * host array of n_shapes entries, each >= 0 (the call uploads it, 4 bytes per shape); n_shapes must be the
 * scene's shape count, with or without a map. A miss has no group.
 * Histogram: a pixel's samples are taken in ascending sample order. A sample whose group is in the table
 * adds 1 to its count; a sample with a new group takes the next entry while the table holds fewer than
 * DT_MATTE_TABLE groups; after that the sample is dropped and the pixel is an overflow pixel.
 * *overflow_pixels (optional): the owned overflow pixels, each counted once (with spp < 64 there are none).
 * Ranking: the table's entries by count descending, ties by group ascending; layer j < layers is entry j of
 * that order, layers beyond the table's size hold id -1, weight 0. weight is exactly
 * (float)((double)count / (double)n_samples); distinct[q] is the table's size.
 * Slots and sides: q is the pixel's slot exactly as in dt_render_features (DT_OUT_IMAGE and DT_OUT_SLAB
 * alike); id and weight hold layers * dt_accum_doubles(g, tiles)/3 elements, distinct dt_accum_doubles/3.
 * Only owned pixels are written. All planes are host (out_on_device=0: staged through device copies of the
 * caller's arrays, as dt_render_features stages) or device (1); a NULL plane is not wanted. Synchronous.
 * Like dt_render_features it has a launch record, counters and events of its own and shares only the
 * scene's primary-ray lists: a render of the scene afterwards is unaffected.
 * stats (optional): pixels produced, samples = rays = pixels * n_samples, kernel_ms; everything else 0.
 * DT_E_INVALID, with a dt_last_error starting "dt_render_mattes: " and naming the argument: a null scene,
 * globals or out, an out with every plane NULL, a bad n_samples, layers outside 1..DT_MATTE_MAX_LAYERS, an
 * n_shapes that is not the scene's, a negative map entry (with its index); DT_E_UNSUPPORTED: a scene with a
 * RectPrismWithCylinder; all before any device work. */
typedef struct dt_mattes {      /* each plane optional (NULL: not wanted), not all NULL; all on one side */
  int32_t* id;        /* layers per pixel, entry layers*q + j: the group ranked j, -1: no such layer */
  float*   weight;    /* layers per pixel, same indexing: (float)((double)count / (double)n_samples), 0 for -1 */
  int32_t* distinct;  /* 1 per pixel, entry q: distinct groups in the pixel's table (<= DT_MATTE_TABLE) */
} dt_mattes;
#define DT_MATTE_TABLE      64   /* distinct groups a pixel's histogram holds */
#define DT_MATTE_MAX_LAYERS 8

int dt_render_mattes(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                     int32_t n_samples, const int32_t* group_of_shape /* host, n_shapes entries, or NULL */,
                     int32_t n_shapes, int32_t layers, const dt_mattes* out, int32_t out_on_device,
                     void* stream, dt_stats* stats, uint64_t* overflow_pixels /* optional */);

/* The matte of a set of groups: mask[q] is the f32 sum, from 0.0f, in layer order j = 0 .. layers-1, of
 * weight[layers*q + j] over the layers whose id is in groups (a host array of 1..64 entries, each >= 0;
 * -1 never matches). id, weight (layers * n_pixels) and mask (n_pixels) are all host (on_device=0: a host
 * loop) or all device (1: one kernel on stream, enqueue only). DT_E_INVALID, with a dt_last_error starting
 * "dt_matte_mask: " and naming the argument: a null pointer, n_pixels < 0, layers outside
 * 1..DT_MATTE_MAX_LAYERS, n_groups outside 1..64, a negative group. n_pixels == 0: DT_OK, nothing is
 * launched. */
int dt_matte_mask(int64_t n_pixels, int32_t layers, const int32_t* id, const float* weight,
                  const int32_t* groups, int32_t n_groups /* host array, 1..64 entries */,
                  float* mask, int32_t on_device, void* stream);

/* ---- ray queries: closest hit and visibility for rays the caller supplies ----
 * No reference counterpart: the reference traces only what its camera and its bounces produce. The
 * primitive under picking, line of sight, light visibility from a set of surface points (baking, probes,
 * ambient occlusion) and a second bounce computed by the caller from the point and normal of the first.
 * start and dir hold 3 doubles per ray; every array of a call is on one side, host (on_device=0: staged
 * through temporaries, as dt_render_features stages its planes) or device (1). Both calls are synchronous,
 * with a launch record, counters and events of their own: they neither read nor rebuild the scene's
 * primary-ray lists, and a render of the scene afterwards is unaffected. Like every call on one scene
 * they must not overlap another call on that scene from another host thread. g: the globals of the
 * scene's renders, as for dt_intersect_primary; only what traversal reads matters, the camera is not read.
 *
 * A ray is VOID if start or dir has a non-finite component or dir is all zero. A void ray is never
 * traced and reports a miss (not occluded); its neighbours are unaffected.
 *
 * dt_trace_rays: rayColor's gather and closest hit (render_final_project.cpp:491-538) for the ray
 * (dir, start) on the unshifted scene (shift 0 on every frame): every leaf whose box the ray passes, in the
 * reference's stack order, then the shapes in that order, strictly closer wins, t carried from shape to
 * shape (oracle.c or_primary_hit). dir is used unnormalised, as the renders use their primary rays. Per
 * hit the attributes are those dt_render_features computes for one sample; a miss writes -1, FLT_MAX and
 * zeros. The normal and the colour are computed only for the planes that take them.
 * stats (optional): rays = the rays traced (the non-void ones), prism_norm_fallback (counted iff normal
 * is wanted), tex_fetches and uv_out_of_range (iff albedo is), kernel_ms; everything else 0.
 *
 * The walk is the renders' wave-uniform one: 64 consecutive rays share a wave, which visits the union of
 * its rays' nodes. Rays that are neighbours in the arrays should be neighbours in space (README.md);
 * dt_ray_order (below) sorts rays that are not. */
typedef struct dt_ray_hits {   /* each plane optional (NULL: not wanted); n_rays entries; all on one side */
  int32_t* shape;    /* closest shape, -1: none */
  float*   t;        /* its t along the unnormalised dir, FLT_MAX: none */
  double*  point;    /* 3 per ray: start + (double)t * dir */
  double*  normal;   /* 3 per ray: fixNorm(normalized(dir), getNorm(point)), world space */
  double*  albedo;   /* 3 per ray: the colour rule of dt_render_features (checker square, texel / 255.0,
                        bordercolor), one hit, no averaging */
} dt_ray_hits;

/* DT_E_INVALID, with a dt_last_error starting "dt_trace_rays: " and naming the argument: a null scene,
 * globals, start, dir or out, an out with every plane NULL, n_rays < 0; DT_E_UNSUPPORTED: a scene with a
 * RectPrismWithCylinder; all before any device work. n_rays == 0: DT_OK, nothing is launched. */
int dt_trace_rays(const dt_scene* s, const dt_globals* g, int64_t n_rays, const double* start, const double* dir,
                  const dt_ray_hits* out, int32_t on_device, void* stream, dt_stats* stats);

/* Is start + dir hidden from start? The light loop's shadow test (render_final_project.cpp:806-852) with
 * sray = dir: t_max = (float)|dir|, sn = normalized(dir); the gather runs along dir from start + 1e-3*dir,
 * and intersectShadow(sn, start + 1e-3*sn, t_max) on every gathered shape but skip_shape[i] (optional,
 * n_rays entries, -1: none; NULL: none for any ray -- the shape a light is, or the surface a ray leaves).
 * occluded[i] = 1 or 0. Tree walks only: the renders' shadow grid is built per light and for the camera's
 * origin box. A walk skips one shape for the whole wave, so a wave is served in groups of equal
 * skip_shape: sort or group the rays by it where it varies.
 * stats (optional): shadow_rays = the rays tested (the non-void ones), kernel_ms; everything else 0.
 * Errors as dt_trace_rays ("dt_rays_occluded: ", a null occluded in the place of out). */
int dt_rays_occluded(const dt_scene* s, const dt_globals* g, int64_t n_rays, const double* start, const double* dir,
                     const int32_t* skip_shape /* optional, n_rays; -1: none */, uint8_t* occluded,
                     int32_t on_device, void* stream, dt_stats* stats);

/* ---- transmittance ray queries: shadow probes that pass through glass ----
 * No reference counterpart. dt_rays_occluded is the light loop's test, for which a glass pane shadows like a
 * wall. This call is that test with a filter: a probe passes through glass shapes, counts them, and is stopped
 * only by a shape that is not glass. Line of sight through windows, light visibility behind a pane and a
 * caller's own tint or Beer's law start here. Rays, the void-ray rule, sides and staging, g, skip_shape (and
 * the advice to group rays by it), synchrony, "a render afterwards is unaffected" and the thread rule are
 * dt_rays_occluded's.
 *
 * Every answer is an integer defined per shape, bit for bit and independent of the order of the work:
 *   CANDIDATES  the shapes dt_rays_occluded gathers: every leaf whose box the ray passes along dir from
 *     start + 1e-3*dir.
 *   PER-SHAPE TEST  a gathered shape h COUNTS iff h != skip_shape[i] and intersectShadow(sn, start + 1e-3*sn,
 *     t_max) is true, with sn = normalized(dir) and t_max = (float)|dir|: exactly the values dt_rays_occluded
 *     passes. Nothing is carried from shape to shape.
 *   GLASS  a shape is glass iff its material is DT_MAT_GLASS.
 *   PANES  panes[i] = -1 if any counting shape is not glass (blocked); otherwise the number of counting glass
 *     shapes, 0: clear. A void ray writes 0. A shape counts once (a sphere, a prism or a pane alike: the test
 *     is intersectShadow's yes or no, not its number of crossings).
 *   PANE_SHAPE  (optional, k per ray, needs k >= 1) the min(k, panes) smallest shape indices among the counting
 *     glass shapes, ascending, then -1s; every entry is -1 where panes[i] <= 0. No floating-point product is
 *     defined here: tint, Beer's law or anything else is the caller's, from the ids.
 * Relation to dt_rays_occluded: occluded[i] == (panes[i] != 0) for every ray, by construction (some shape
 * counts there iff some shape counts here).
 * stats (optional): shadow_rays = the rays tested (the non-void ones), kernel_ms; everything else 0.
 *
 * The walk is dt_rays_occluded's wave-uniform one (groups of equal skip_shape, the same box cull); a lane
 * leaves it only when blocked, so a ray behind glass walks as far as a clear ray does. The list of pane ids is
 * kept in registers, in a capacity of 0 (no pane_shape), 1, 2, 4 or 8 slots, the smallest that holds k.
 * Cost: BASELINE.md "Transmittance queries".
 *
 * DT_E_INVALID, with a dt_last_error starting "dt_rays_transmittance: " and naming the argument: a null scene,
 * globals, start, dir or out, an out with every plane NULL, n_rays < 0, k outside 0..DT_TRANSMIT_MAX_PANES,
 * out->pane_shape given with k == 0; DT_E_UNSUPPORTED: a scene with a RectPrismWithCylinder; all before any
 * device work. n_rays == 0: DT_OK, nothing is launched. */
#define DT_TRANSMIT_MAX_PANES 8
typedef struct dt_ray_transmittance {   /* each plane optional (NULL: not wanted), not both NULL; all on one side */
  int32_t* panes;        /* 1 per ray: -1 blocked, else the counting glass shapes (0: clear) */
  int32_t* pane_shape;   /* k per ray, entry k*i + j: the j-th smallest counting glass shape; -1 beyond */
} dt_ray_transmittance;
int dt_rays_transmittance(const dt_scene* s, const dt_globals* g, int64_t n_rays, const double* start,
                          const double* dir, const int32_t* skip_shape /* optional, n_rays; -1: none */,
                          int32_t k /* 0..DT_TRANSMIT_MAX_PANES */, const dt_ray_transmittance* out,
                          int32_t on_device, void* stream, dt_stats* stats);

/* ---- path ray queries: caller-supplied rays followed through mirrors and glass ----
 * No reference counterpart. dt_trace_rays stops at the first surface; dt_render_features_path follows the
 * render's own camera samples through the scene's perfect reflectors and reports per-pixel means. This call
 * runs that chain for rays the caller hands over and answers per ray: where the ray ends up after the mirrors
 * and panes, the vertices on the way, the length of the path. Picking the object seen in a mirror, a polyline
 * of a ray through the scene's optics, a caller's own next bounce (the last segment's ray is returned, and
 * `inside` is handled here) start from it. Geometry only: no Fresnel weights, no radiance.
 * Rays, the void-ray rule, sides and staging, g, synchrony, "a render afterwards is unaffected" and the thread
 * rule are dt_trace_rays's.
 *
 * Per ray, segment k = 0, 1, ... (segment 0 is the caller's ray (dir, start)) -- exactly the per-sample chain of
 * dt_render_features_path:
 *   a VOID segment (dt_trace_rays's rule on (dir_k, start_k); tested before every segment, the caller's own
 *   included) is not traced: the path ends as DT_PATH_VOID. This is the caller's ray, or the successor of
 *   normal incidence on glass, whose next_dir is not finite (dt_guide_bounce).
 *   Otherwise the segment is traced to its closest hit as dt_trace_rays specifies it (shift 0, dir
 *   unnormalised): shape h_k, t_k, inside_k. No hit: the path ends as DT_PATH_MISS. On a hit
 *     L   = L + (double)t_k * |dir_k|                      (f64, from +0)
 *     p_k = start_k + (double)t_k * dir_k,   n_k = fixNorm(normalized(dir_k), getNorm(p_k))
 *   and iff k < max_bounces the bounce rule (dt_guide_bounce) is evaluated at (h_k's material and flags,
 *   inside_k, normalized(dir_k), n_k, p_k): reflect or refract gives segment k+1 = (next_dir, next_start); stop
 *   ends the path as DT_PATH_SURFACE on h_k. The hit of segment max_bounces ends it as DT_PATH_CUT on h_k, the
 *   rule not evaluated. n_k is computed iff k < max_bounces or the normal plane is wanted; the colour
 *   (dt_render_features's rule at (h_k, p_k)) only at the terminal hit, and only if albedo is wanted.
 * max_bounces = 0 is dt_trace_rays in shape, point, normal and albedo, and length = (double)t * |dir|.
 * Every element of every wanted plane is written. The per-segment planes hold max_bounces + 1 entries per ray:
 * entry (max_bounces+1)*i + k describes segment k of ray i, -1 and zeros where the segment was not traced or
 * hit nothing.
 * stats (optional): rays = the segments traced, reflect_errors (the rule's refl_err), prism_norm_fallback (per
 * normal computed), tex_fetches and uv_out_of_range (the terminal colour only), kernel_ms; everything else 0.
 *
 * The walk is dt_trace_rays's wave-uniform one: 64 consecutive rays share a wave, and the wave runs segment k
 * for the rays still travelling while the others wait. After the first bounce a wave's rays scatter, so a later
 * segment costs what dt_trace_rays costs on scattered rays (BASELINE.md "Path ray queries").
 * Limits, as dt_render_features_path: glossy reflectors (DT_F_GLOSSY with nogloss = 0) stop the chain, glass
 * follows transmission only (total internal reflection takes the mirror rule), never its reflection.
 *
 * DT_E_INVALID, with a dt_last_error starting "dt_trace_rays_path: " and naming the argument: a null scene,
 * globals, start, dir or out, an out with every plane NULL, n_rays < 0, max_bounces outside
 * 0..DT_RAY_PATH_MAX_BOUNCES; DT_E_UNSUPPORTED: a scene with a RectPrismWithCylinder; all before any device
 * work. n_rays == 0: DT_OK, nothing is launched. */
#define DT_RAY_PATH_MAX_BOUNCES 8          /* == DT_GUIDE_MAX_BOUNCES */
enum { DT_PATH_VOID = 0, DT_PATH_MISS = 1, DT_PATH_SURFACE = 2, DT_PATH_CUT = 3 };
typedef struct dt_ray_paths {   /* every plane optional (NULL: not wanted), not all NULL; all on one side */
  int32_t* end;        /* n: one of DT_PATH_* */
  int32_t* segments;   /* n: segments traced, 0 .. max_bounces+1 (0: the caller's ray was void) */
  int32_t* shape;      /* n: the shape the path ended on (SURFACE, CUT), else -1 */
  double*  length;     /* n: L, the f64 sum over the path's hits of (double)t_k * |dir_k|, from +0 */
  double*  point;      /* 3n: the terminal hit p_k; zeros unless SURFACE or CUT */
  double*  normal;     /* 3n: the terminal hit's fixNorm'ed normal n_k; zeros unless SURFACE or CUT */
  double*  albedo;     /* 3n: dt_render_features's colour rule at the terminal hit; zeros unless SURFACE or CUT */
  double*  last_start; /* 3n: the ray of the last segment traced (zeros when segments == 0) */
  double*  last_dir;   /* 3n */
  int32_t* seg_shape;  /* (max_bounces+1) per ray, entry (max_bounces+1)*i + k: the shape segment k hit, else -1 */
  double*  seg_point;  /* 3 per entry, same indexing: p_k; zeros where seg_shape is -1 */
} dt_ray_paths;
int dt_trace_rays_path(const dt_scene* s, const dt_globals* g, int64_t n_rays, const double* start, const double* dir,
                       int32_t max_bounces /* 0..DT_RAY_PATH_MAX_BOUNCES */, const dt_ray_paths* out,
                       int32_t on_device, void* stream, dt_stats* stats);

/* ---- multi-hit ray queries: the k nearest surfaces along caller-supplied rays ----
 * No reference counterpart. dt_trace_rays says what a ray hits first; this call says what lies behind it: per
 * ray the k nearest shapes along it, ordered. Seeing through the panes of a scene, picking the object behind
 * the front one, thickness, X-ray views, depth peeling and a caller's own transparent-shadow rule start here.
 * Rays, the void-ray rule, sides and staging, g, synchrony, "a render afterwards is unaffected" and the thread
 * rule are dt_trace_rays's. A void ray has count 0.
 *
 * Every answer is defined bit for bit and independent of the order of the work:
 *   CANDIDATES  the shapes dt_trace_rays gathers for the ray (dir, start) at shift 0: every leaf whose box the
 *     ray passes.
 *   PER-SHAPE TEST  each gathered shape h is tested on its own: intersect(dir, start) with t entering as
 *     FLT_MAX. Nothing is carried from shape to shape (dt_trace_rays carries t).
 *   HIT  h is a hit iff intersect returns true and t_h < FLT_MAX (false for a NaN). An edge-on checkerboard
 *     hit, which returns true without writing t (Q16, oracle.c shape_intersect), is therefore not a hit here.
 *   ONE HIT PER SHAPE  a shape contributes at most one hit, its own first intersection: the far side of a
 *     sphere, a cylinder or a prism is not a second hit.
 *   RANKING  hits are ordered by t ascending (float compare), ties by shape index ascending. The first
 *     min(k, hits) are recorded; count is that number. Tree and visiting order cannot matter.
 *   ATTRIBUTES  each recorded hit gets what dt_trace_rays computes for its one hit: point, getNorm + fixNorm,
 *     the colour rule with the checker square, texel and border colour; computed only for the planes that
 *     take them.
 * Relation to dt_trace_rays: with k = 1, shape[i] and t[i] equal dt_trace_rays's wherever the smallest t is
 * attained by one gathered shape only and no gathered shape takes the edge-on path. Nothing more is promised
 * (dt_trace_rays breaks ties by gather order and lets an edge-on hit keep the previous shape's t).
 * stats (optional): rays = the non-void rays; prism_norm_fallback per recorded hit, iff normal is wanted;
 * tex_fetches and uv_out_of_range per recorded hit, iff albedo is; kernel_ms; everything else 0.
 *
 * The walk is dt_trace_rays's wave-uniform one, with a per-ray sorted list of k hits in registers; a ray's
 * list culls the tree by its k-th distance once it is full, so a larger k walks further. The ordering advice
 * of dt_trace_rays holds (dt_ray_order). Cost: BASELINE.md "Multi-hit ray queries". */
#define DT_MULTIHIT_MAX 8
typedef struct dt_ray_multihits {   /* each plane optional (NULL: not wanted), not all NULL; all on one side */
  int32_t* count;   /* 1 per ray: hits recorded, 0..k */
  int32_t* shape;   /* k per ray, entry k*i + j: the shape ranked j; -1 for j >= count[i] */
  float*   t;       /* k per ray, same indexing: its t along the unnormalised dir; FLT_MAX for j >= count */
  double*  point;   /* 3k per ray, entry 3*(k*i + j) + c: start + (double)t * dir; zeros beyond count */
  double*  normal;  /* same indexing: fixNorm(normalized(dir), getNorm(point)); zeros beyond count */
  double*  albedo;  /* same indexing: dt_trace_rays's colour rule at that hit; zeros beyond count */
} dt_ray_multihits;

/* DT_E_INVALID, with a dt_last_error starting "dt_trace_rays_multi: " and naming the argument: a null scene,
 * globals, start, dir or out, an out with every plane NULL, n_rays < 0, k outside 1..DT_MULTIHIT_MAX;
 * DT_E_UNSUPPORTED: a scene with a RectPrismWithCylinder; all before any device work. n_rays == 0: DT_OK,
 * nothing is launched. */
int dt_trace_rays_multi(const dt_scene* s, const dt_globals* g, int64_t n_rays, const double* start,
                        const double* dir, int32_t k /* 1..DT_MULTIHIT_MAX */, const dt_ray_multihits* out,
                        int32_t on_device, void* stream, dt_stats* stats);

/* ---- camera rays as arrays, and per-ray answers resolved back to pixels ----
 * The ray queries answer rays the caller hands over; picking under a cursor, X-ray views, depth peeling and
 * thickness start from the render's own camera rays. dt_camera_rays writes those rays out, dt_rays_resolve
 * reduces per-ray answers of any query back to per-pixel planes with the project's fixed summation order, so
 * a query becomes a plane that lines up with the colour image edge for edge. By the definitions here,
 * dt_camera_rays(samples 0..n) -> dt_trace_rays(shape, albedo, normal) -> dt_rays_resolve reproduces
 * dt_render_features' albedo, normal and coverage planes bit for bit.
 *
 * Slots and rows. q is a pixel's output slot: its colour sits at floats 3q .. 3q+2 of dt_render's output
 * (DT_OUT_IMAGE and DT_OUT_SLAB alike; tiles == NULL: the whole image), so there are dt_accum_doubles / 3
 * slots. With ns = sample_end - sample_begin samples per pixel, sample i of slot q is row
 * q*ns + (i - sample_begin); the arrays hold dt_camera_rays_rows = (dt_accum_doubles / 3) * ns rows (-1 for
 * globals, tiles or a sample range the calls refuse). Only the rows of pixels the tile share owns are
 * written; the others are left as they came.
 *
 * dt_camera_rays: no scene is needed, the camera is the globals' alone (the CPU oracle's or_primary_ray is the
 * counterpart). Row (q, i) is the ray dt_render starts sample i of that pixel from, bit for bit: RNG pixel
 * y*xRes + x, sample i, key (seed, frame), one draw of the depth-of-field purpose iff aperture > 0; start is
 * the eye sample (3 doubles), dir the unnormalised ray through the pixel's focal point (3 doubles). In
 * dt_intersect_primary's numbering it is ray ((i/8)*W*H + y*W + x)*8 + i%8. The range is free of spp and of
 * the 64-sample chunks: 0 <= sample_begin < sample_end, at most DT_CAMERA_RAYS_MAX_SAMPLES samples.
 * Limits: only the render's thin-lens perspective camera (no orthographic, panoramic or fisheye model); the
 * motion-blur re-trace of frames >= frame_prism is not reproduced (as for the feature buffers).
 * Both arrays on one side: the device (on_device=1: one kernel on `stream`, one ray per lane, a wave's 64
 * rows 1536 contiguous bytes per array) or the host (0: staged through device copies of the caller's arrays,
 * so unowned rows go back as they came). The call waits for its work; kernel_ms (optional): the kernel's
 * HIP-event time. DT_E_INVALID before any device work, with a dt_last_error starting "dt_camera_rays: " and
 * naming the argument: null globals, start or dir, a bad sample range, globals or tiles the renders refuse. */
#define DT_CAMERA_RAYS_MAX_SAMPLES 1024
int64_t dt_camera_rays_rows(const dt_globals* g, const dt_tiles* tiles, int32_t sample_begin, int32_t sample_end);
int dt_camera_rays(const dt_globals* g, int32_t frame, const dt_tiles* tiles, int32_t sample_begin,
                   int32_t sample_end, double* start, double* dir, int32_t on_device, void* stream,
                   float* kernel_ms);

/* dt_rays_resolve: values holds `width` (1..3) doubles per row, rows as above with ns = n_samples
 * (1..DT_CAMERA_RAYS_MAX_SAMPLES); shape (optional) one int32 per row: a row with shape < 0 adds nothing
 * (a miss of dt_trace_rays). Per owned pixel q and component k, every operation one rounded IEEE f64
 * operation (csrc/dt_rays_resolve.h is the one definition for the host loop and the kernel;
 * tests/camera_rays_ref.py restates it in numpy):
 *   S = 0.0 ; H = 0 ; for i = 0 .. n_samples-1 in this order: if the row counts { S = S + values[..k] ; H += 1 }
 *   DT_RESOLVE_MEAN:      out[width*q + k] = (float)(S / (double)n_samples)
 *   DT_RESOLVE_HIT_MEAN:  out[width*q + k] = H > 0 ? (float)(S / (double)H) : 0.0f
 *   coverage[q] (optional) = (float)((double)H / (double)n_samples)
 * which is how dt_render_features forms albedo and normal (MEAN), depth (HIT_MEAN) and coverage. Without
 * shape every row counts. Only owned pixels are written. f64 rows only.
 * All arrays on one side: host (on_device=0: a plain loop) or device (1: one kernel on `stream`, enqueue
 * only). DT_E_INVALID before any device work, with a dt_last_error starting "dt_rays_resolve: " and naming
 * the argument: null globals, values or out, n_samples, width or mode out of range, bad globals or tiles. */
#define DT_RESOLVE_MEAN     0
#define DT_RESOLVE_HIT_MEAN 1
int dt_rays_resolve(const dt_globals* g, const dt_tiles* tiles, int32_t n_samples, int32_t width /* 1..3 */,
                    const double* values, const int32_t* shape /* optional */, int32_t mode, float* out,
                    float* coverage /* optional */, int32_t on_device, void* stream);

/* ---- ray ordering: sort caller-supplied rays into coherent waves ----
 * No reference counterpart. The ray queries serve 64 consecutive array entries with one wave, and a wave walks
 * the union of its lanes' nodes: rays with no natural order cost up to 4x. dt_ray_order gives
 * every ray a key (the cell of its start in a box and the cell of its direction on the octahedral map, both
 * Morton-interleaved) and returns the stable ascending order of the keys as a permutation; dt_permute_rows
 * gathers rows by it (the rays, skip_shape) and puts the answers back in the caller's order.
 *
 * The key. B = 3*origin_bits + 2*dir_bits, 1 <= B <= 30. Every operation below is one rounded IEEE f64
 * operation in the parenthesisation written (no contraction, no libm; csrc/dt_order.h is the one definition
 * for the host loop, the kernel and dt_ray_order_key; tests/rayorder_ref.py restates it in numpy).
 *   A VOID ray (dt_trace_rays's rule: a non-finite component of start or dir, or an all-zero dir) has the key
 *   1u << B: void rays sort last, and they contribute nothing to the box.
 *   The box (lo, hi): box_lo, box_hi if box_given; else per axis the minimum and the maximum of the non-void
 *   rays' starts, each reported as x + 0.0 (a -0 becomes +0, whichever zero a reduction met first); with no
 *   non-void ray, all zeros.
 *   cell(f, bits): !(f > 0) (a NaN included) -> 0; f >= 1 -> 2^bits - 1; otherwise (uint32_t)(f * 2^bits).
 *   Origin cell, per axis k: e = hi_k - lo_k; f = e > 0 ? (o_k - lo_k) / e : 0; c_k = cell(f, origin_bits).
 *   Direction cell: s = (|dx| + |dy|) + |dz|; u = dx / s; v = dy / s; if dz < 0:
 *     (u, v) = ((1 - |v|) * (u >= 0 ? 1 : -1), (1 - |u|) * (v >= 0 ? 1 : -1)), both from the old u and v;
 *   g_u = u * 0.5 + 0.5, g_v = v * 0.5 + 0.5; d_0 = cell(g_u, dir_bits), d_1 = cell(g_v, dir_bits).
 *   (Huge finite components may overflow s or o_k - lo_k to inf: the rules above still give one key.)
 *   Packing: bit 3i + k of M3 is bit i of c_k; bit 2i + k of M2 is bit i of d_k;
 *     dir_major == 0: key = (M3 << 2*dir_bits) | M2     (rays of one place together, then by direction)
 *     dir_major == 1: key = (M2 << 3*origin_bits) | M3  (rays of one direction together, then by place).
 * dt_ray_order_params_default: origin_bits 5, dir_bits 6, dir_major 0, box_given 0. The defaults are a choice,
 * not a measurement: 32 cells per axis and 64 x 64 directions for rays scattered through a scene. Rays that
 * all start on one lens (a camera's) cannot be told apart by an origin cell: use origin_bits 0, dir_bits 8.
 * Fewer key bits mean fewer sort passes (below).
 * dt_ray_order_key: the key of one ray inside the box (lo, hi), on the host, for tests and callers. DT_OK; a
 * null argument or a bad bit count: DT_E_INVALID ("dt_ray_order_key: ").
 *
 * dt_ray_order: perm[i] is the caller's index of the ray that goes to place i, in the stable ascending order
 * of the keys: exactly numpy's argsort(keys, kind="stable"). keys (optional): the n_rays keys in the caller's
 * order. box (optional, always a host pointer): lo[3], hi[3] as used. start, dir, perm and keys are all host
 * (on_device = 0: a host loop with std::stable_sort that touches no device; workspace is not read and may be
 * NULL) or all device (1; workspace: dt_ray_order_workspace_bytes(n_rays) bytes of device memory, any
 * alignment). The device path enqueues on `stream`: a min / max reduction for the box (unless it is given;
 * exact and order-free), a key kernel, and an LSD radix sort of (key, index) pairs with 8-bit digits in
 * ceil((B + 1) / 8) passes, each pass a histogram of DT_RAY_ORDER_TILE keys per workgroup, a scan of the
 * histograms and a scatter, every step a kernel of its own: no workgroup ever waits on another. The call
 * returns without waiting unless kernel_ms (optional: the HIP-event time of the whole chain) or a box that
 * the device computed (box given as a pointer while box_given == 0) is asked for; then it is synchronous.
 * Errors, all before any device work: DT_E_INVALID, with a dt_last_error starting "dt_ray_order: " and naming
 * the argument, for a null start, dir, params or perm, a null workspace with on_device, n_rays < 0,
 * origin_bits outside 0..10, dir_bits outside 0..8, B outside 1..30, dir_major or box_given other than 0 or
 * 1, a given box that is not finite or has lo > hi; DT_E_LIMIT for n_rays > 2^30. n_rays == 0: DT_OK, nothing
 * is launched (box: the given one, or zeros).
 *
 * dt_permute_rows: rows of row_bytes (1..64) bytes. inverse == 0: dst[i] = src[perm[i]], a gather that puts
 * rays in order; inverse == 1: dst[perm[i]] = src[i], which puts answers back in the caller's order. perm, src
 * and dst all host or all device (1: one kernel on stream, enqueue only); src and dst must not overlap. The
 * rows move as 8-byte words where row_bytes and both addresses are multiples of 8 (the 24-byte rays, points
 * and normals), as dwords for multiples of 4 (shape, t, skip_shape), as bytes otherwise (occluded). The host
 * path checks perm[i] < n (DT_E_INVALID naming the entry); the device path trusts the caller: an entry >= n
 * reads or writes outside the arrays. DT_E_INVALID ("dt_permute_rows: ") for a null perm, src or dst, n < 0,
 * row_bytes outside 1..64, inverse other than 0 or 1, overlapping src and dst; DT_E_LIMIT for n > 2^32.
 *
 * What ordering costs and when it pays: BASELINE.md "Ray ordering". dt_points_occlusion takes no order: its
 * RNG counter is the point's index. */
#define DT_RAY_ORDER_TILE 4096   /* keys per workgroup of the radix sort's histogram and scatter kernels */
typedef struct dt_ray_order_params {
  int32_t origin_bits;   /* 0..10 per axis */
  int32_t dir_bits;      /* 0..8 per axis of the octahedral map */
  int32_t dir_major;     /* 0: origin cell in the high bits; 1: direction cell in the high bits */
  int32_t box_given;     /* 0: the box is the min/max of the non-void rays' starts */
  double  box_lo[3], box_hi[3];   /* read iff box_given: finite, lo <= hi */
} dt_ray_order_params;
void    dt_ray_order_params_default(dt_ray_order_params* p);
int     dt_ray_order_key(const dt_ray_order_params* p, const double lo[3], const double hi[3], const double start[3],
                         const double dir[3], uint32_t* key);
int64_t dt_ray_order_workspace_bytes(int64_t n_rays);
int     dt_ray_order(int64_t n_rays, const double* start, const double* dir, const dt_ray_order_params* p,
                     uint32_t* perm, uint32_t* keys /* optional, caller order */, double box[6] /* optional, host */,
                     void* workspace, int32_t on_device, void* stream, float* kernel_ms /* optional */);
int     dt_permute_rows(int64_t n, int32_t row_bytes /* 1..64 */, const uint32_t* perm, const void* src, void* dst,
                        int32_t inverse, int32_t on_device, void* stream);

/* ---- occlusion feature buffers: ambient occlusion and per-light visibility ----
 * No reference counterpart. The guides of dt_render_features say what a surface is; these say how exposed it
 * is: an ambient-occlusion plane and one visibility ("shadow") plane per chosen light, at the render's own
 * samples. The standard compositor companions of the feature planes and the mattes; a guide that tells a
 * soft shadow on a flat, single-coloured floor from noise.
 *
 * Samples, rays, slots q, layouts, sides, staging, the n_samples window rule and "only owned pixels are
 * written" are exactly dt_render_features's. Per sample i of pixel (x, y) the primary ray is traced to its
 * closest hit exactly as dt_render_features traces it (shift 0 on every frame). A miss adds nothing; a hit
 * gives p = eye_sample + (double)t * ray and n = fixNorm(normalized(ray), getNorm(p)). H counts the hitting
 * samples of the pixel.
 *
 * RNG: Philox4x32-10, key (g->seed, (uint32_t)frame), counter (pixel = y*xRes + x, sample = i, node = 0,
 * (purpose << 24) | sub) with the two purposes P_AO = 6 and P_OLIGHT = 7; the render's own draws at node 0
 * use purposes 1..5, so no stream is shared. u01(w0, w1) is the render's: ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53.
 *
 * Ball point v(purpose, base): for a = 0 .. DT_OCCL_TRIES-1 draw the words o at sub = base*16 + a,
 *   x = (double)o[0] * 2^-31 - 1.0, y and z likewise from o[1], o[2] (all exact in f64),
 *   s = (x*x + y*y) + z*z;
 * the first a with s <= 1.0 gives v = (x, y, z); none: v = (0, 0, 0). No normalisation, no libm.
 *
 * Ambient occlusion: probe r = 0 .. ao_rays-1 of a hitting sample has v = v(P_AO, r) and
 *   dir[k] = R * (n[k] + v[k]),  R = (double)ao_radius                (each operation one rounded f64 one):
 * "is a point of the ball of radius R resting on the surface at p visible from p?", answered exactly as
 * dt_rays_occluded(start = p, dir, skip_shape = -1) answers it, its void-ray rule included (v = -n gives a
 * zero dir: not traced, not occluded). With V the unoccluded probes of the pixel,
 *   ao[q] = (float)((double)V / ((double)n_samples * (double)ao_rays)),
 * premultiplied by coverage like albedo and normal (sky: 0; divide by the coverage plane to un-premultiply).
 *
 * Light visibility: slot j selects light L = lights[j] of the scene, with the target T
 *   DT_LIGHT_POINT:  T = center
 *   DT_LIGHT_RECT:   the words o at (P_OLIGHT, sub = j*16), u0 = u01(o[0], o[1]), u1 = u01(o[2], o[3]),
 *                    T = (A + u0*(B-A)) + u1*(D-A)
 *   DT_LIGHT_SPHERE: T = center + (double)radius * v(P_OLIGHT, j): a point of the light's volume (the light's
 *                    own shape is skipped, so no far-side rule is needed)
 * and dir = T - p, answered as dt_rays_occluded(start = p, dir, skip_shape = L.shape_index). There is no
 * facing test: a surface turned away from the light is shadowed by its own geometry through the 1e-3
 * offset, as in the light loop. With V_j the unoccluded probes,
 *   light[n_lights*q + j] = (float)((double)V_j / (double)n_samples).
 * All sums are integers: the planes do not depend on any summation order.
 *
 * First hits only: a probe starts on the first surface a sample sees, a mirror's or a pane's own, and a
 * probe does not pass through glass (a glass shape occludes, as in the light loop's shadow test).
 *
 * stats (optional): pixels, samples = rays = pixels * n_samples, shadow_rays = the probes tested (the
 * non-void ones), prism_norm_fallback, kernel_ms; everything else 0. A plane that is not wanted (NULL while
 * ao_rays > 0 or n_lights > 0) costs no probes: its probes are neither generated nor counted.
 * Errors, with a dt_last_error starting "dt_render_occlusion: " and naming the argument: DT_E_INVALID for a
 * null scene, globals, params or out, a bad n_samples, ao_rays outside 0..DT_OCCL_MAX_AO_RAYS, n_lights
 * outside 0..DT_OCCL_MAX_LIGHTS, a non-finite or non-positive ao_radius while ao_rays > 0, a light index
 * outside the scene, out->ao given with ao_rays == 0, out->light given with n_lights == 0, every plane
 * NULL; DT_E_UNSUPPORTED for a scene with a RectPrismWithCylinder; all before any device work.
 * Synchronous, with a launch record, counters and events of its own; it shares only the scene's
 * primary-ray lists, and a render of the scene afterwards is unaffected.
 *
 * dt_occlusion_params_default: ao_rays 4, n_lights 0, ao_radius 1.0. The radius is a choice, not a
 * measurement: a plain constant, one world unit, which the Python wrapper and the CLI take as well. The
 * shipped scenes are built to human scale (the room of `final` is 20 units wide, its steps and furniture 0.5
 * to 2), and ambient occlusion is meant to show contact and corner darkening at the scale of the objects,
 * not the room's own walls. A fraction of the scene's BVH root box is not used although the call's wrappers
 * have the scene: the builders put far geometry into it (the root box of `final` has a diagonal of 2000
 * units, so 5% of it, 100 units, finds every probe of the room occluded: a mean ao of 0.0014 on C3). */
#define DT_OCCL_MAX_AO_RAYS 16
#define DT_OCCL_MAX_LIGHTS   8
#define DT_OCCL_TRIES       16
typedef struct dt_occlusion_params {
  int32_t ao_rays;      /* 0..DT_OCCL_MAX_AO_RAYS occlusion rays per hitting sample; 0: no ao plane */
  float   ao_radius;    /* finite, > 0: the radius R of the probe ball, world units */
  int32_t n_lights;     /* 0..DT_OCCL_MAX_LIGHTS */
  int32_t lights[DT_OCCL_MAX_LIGHTS]; /* indices into the scene's lights, each 0 <= l < the scene's n_lights */
} dt_occlusion_params;
typedef struct dt_occlusion {   /* each plane optional; all on one side */
  float* ao;      /* 1 per pixel, entry q            (needs ao_rays > 0) */
  float* light;   /* n_lights per pixel, entry n_lights*q + j (needs n_lights > 0) */
} dt_occlusion;
void dt_occlusion_params_default(dt_occlusion_params* p);
int  dt_render_occlusion(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                         int32_t n_samples, const dt_occlusion_params* params, const dt_occlusion* out,
                         int32_t out_on_device, void* stream, dt_stats* stats);
/* The two probe generators for one hit (csrc/dt_occl.h, one definition for host and kernel), for tests and
 * callers: dir of AO probe r (0..15) from the fixNorm'ed normal n, and of the probe of slot j (0..7) towards
 * `light` from p. No device work. DT_OK; a null argument or an index outside its range: DT_E_INVALID.
 * (p is not read by the AO rule; it is part of the signature for symmetry and must not be null.) */
int dt_occlusion_ao_ray(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, int32_t r, float ao_radius,
                        const double p[3], const double n[3], double dir[3]);
int dt_occlusion_light_ray(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, int32_t j,
                           const dt_light_desc* light, const double p[3], double dir[3]);

/* ---- occlusion queries at surface points: ambient occlusion and light visibility for baking ----
 * No reference counterpart. dt_render_occlusion asks "how exposed is this surface?" at the camera's own first
 * hits, dt_rays_occluded for rays the caller builds one by one; this call asks it at surface points the
 * caller supplies (the texels of a lightmap, probes), with the probes generated on the device: per point 24
 * bytes of position and 24 of normal go in, one float per plane entry comes out.
 *
 * Samples and RNG counter: point i (0 <= i < n_points, n_points < 2^32) takes the samples s = 0 ..
 * n_samples-1. The RNG counter is dt_render_occlusion's with pixel = (uint32_t)i and sample = s, the key
 * (g->seed, (uint32_t)frame), the purposes P_AO = 6 and P_OLIGHT = 7; DT_OCCL_TRIES is unchanged.
 *
 * Probes: with p = point[3i..3i+2] and n = normal[3i..3i+2], sample s of point i has the ao_rays probes
 * dt_occlusion_ao_ray(seed, frame, i, s, r, ao_radius, p, n), r = 0 .. ao_rays-1, and per light slot j the probe
 * dt_occlusion_light_ray(seed, frame, i, s, j, light, p): the rules of dt_render_occlusion, unchanged (one
 * definition, csrc/dt_occl.h). n is the caller's normal as given: it is not normalised and fixNorm is not
 * applied (the AO ball rests on the surface only for a unit n that points away from it). Each probe is answered exactly as dt_rays_occluded(start = p, dir, skip_shape)
 * answers it, with skip_shape = -1 for an AO probe and L.shape_index for a probe towards light L; its
 * void-ray rule applies: a probe with a zero (or non-finite) dir is not traced and counts as not occluded.
 *
 * Sums and outputs: with V the unoccluded AO probes of point i and V_j the unoccluded probes towards slot j,
 *   ao[i] = (float)((double)V / ((double)n_samples * (double)ao_rays)),
 *   light[n_lights*i + j] = (float)((double)V_j / (double)n_samples).
 * The sums are integers, so the outputs do not depend on the order of the work.
 *
 * A point is VOID if point or normal has a non-finite component. A void point is never probed, writes 0 to
 * each of its outputs and counts no probes; its neighbours are unaffected.
 *
 * point, normal and the planes of out are all host (on_device=0: staged through temporaries, as
 * dt_rays_occluded stages its arrays) or all device (1). The call is synchronous, with a launch record,
 * counters and events of its own; it neither reads nor rebuilds the scene's primary-ray lists, and a render
 * of the scene afterwards is unaffected. g: as for the ray queries, only what traversal reads and the seed
 * matter; the camera is not read.
 * stats (optional): shadow_rays = the probes tested (the non-void ones), kernel_ms; everything else 0. A
 * plane that is not wanted (NULL while ao_rays > 0 or n_lights > 0) costs no probes.
 *
 * Errors, with a dt_last_error starting "dt_points_occlusion: " and naming the argument, all before any
 * device work: DT_E_INVALID for a null scene, globals, point, normal, params or out, n_points < 0 or
 * n_points >= 2^32, n_samples outside 1..DT_POCCL_MAX_SAMPLES, and dt_render_occlusion's rules: ao_rays outside
 * 0..DT_OCCL_MAX_AO_RAYS, n_lights outside 0..DT_OCCL_MAX_LIGHTS, a non-finite or non-positive ao_radius
 * while ao_rays > 0, a light index outside the scene, out->ao given with ao_rays == 0, out->light given with
 * n_lights == 0, every plane NULL; DT_E_UNSUPPORTED for a scene with a RectPrismWithCylinder.
 * n_points == 0: DT_OK, nothing is launched.
 *
 * The walk is the renders' wave-uniform one, as for dt_rays_occluded: 64 consecutive points share a wave,
 * which visits the union of its probes' nodes, one walk per probe index (a light slot skips one shape for the
 * whole wave, so no grouping by skip_shape is needed). Points that are neighbours in the arrays should be
 * neighbours in space (README.md). */
#define DT_POCCL_MAX_SAMPLES 1024
int dt_points_occlusion(const dt_scene* s, const dt_globals* g, int32_t frame, int64_t n_points,
                        const double* point, const double* normal,   /* 3 doubles per point each */
                        int32_t n_samples,                           /* 1..DT_POCCL_MAX_SAMPLES */
                        const dt_occlusion_params* params, const dt_occlusion* out,
                        int32_t on_device, void* stream, dt_stats* stats);

/* The baking mode whose probes pass through glass. Points, samples, the RNG counter, the probe generators, void
 * points, sums, sides, synchrony and errors are dt_points_occlusion's (prefix "dt_points_occlusion_glass: ");
 * dt_occlusion_params and dt_occlusion are unchanged. The differences:
 *   each probe is answered by dt_rays_transmittance's rule (start = p, dir, the same skip_shape) in the place of
 *     dt_rays_occluded's, and is UNOCCLUDED iff 0 <= panes <= max_panes (a void probe: panes 0, unoccluded);
 *   panes (optional) takes two more planes, indexed like ao and light: with S the integer sum of `panes` over
 *     the unoccluded AO probes of point i and S_j that over the unoccluded probes towards slot j,
 *       ao_panes[i] = (float)((double)S / ((double)n_samples * (double)ao_rays)),
 *       light_panes[n_lights*i + j] = (float)((double)S_j / (double)n_samples):
 *     the mean number of panes crossed per probe, the denominators of ao and light. A void point writes 0.
 * A row of probes runs iff one of its two planes is wanted (ao or ao_panes; light or light_panes): a plane that
 * is not wanted costs nothing. out must still want a plane of its own, by dt_points_occlusion's rule.
 * With max_panes = 0 a probe is unoccluded iff nothing counts, which is dt_rays_occluded's answer: the ao and
 * light planes equal dt_points_occlusion's bit for bit.
 * Additional DT_E_INVALID: max_panes outside 0..DT_TRANSMIT_MAX_PANES, panes->ao_panes given with ao_rays == 0,
 * panes->light_panes given with n_lights == 0.
 * Not covered: dt_render_occlusion (the camera-sample planes) keeps the wall rule. */
typedef struct dt_occlusion_panes {   /* each plane optional; on the side of out */
  float* ao_panes;      /* 1 per point            (needs ao_rays > 0) */
  float* light_panes;   /* n_lights per point, entry n_lights*i + j (needs n_lights > 0) */
} dt_occlusion_panes;
int dt_points_occlusion_glass(const dt_scene* s, const dt_globals* g, int32_t frame, int64_t n_points,
                              const double* point, const double* normal, int32_t n_samples,
                              const dt_occlusion_params* params, int32_t max_panes /* 0..DT_TRANSMIT_MAX_PANES */,
                              const dt_occlusion* out, const dt_occlusion_panes* panes /* optional */,
                              int32_t on_device, void* stream, dt_stats* stats);

/* ---- irradiance queries at surface points: direct light and one gather bounce, for light baking ----
 * No reference counterpart. dt_points_occlusion returns fractions of unoccluded probes; this call turns the same
 * probes into light: per point the cosine-weighted visibility of each chosen light, its sum with the lights'
 * colours, and one diffuse bounce gathered over the hemisphere. No recursion, no glossy cascade, no libm beyond
 * the square root of `normalized`.
 *
 * Points, samples, RNG key and counter (pixel = (uint32_t)i, sample = s), void points, host/device sides,
 * staging and synchrony are dt_points_occlusion's. n = normal[3i..3i+2] is taken as given: no fixNorm, no
 * normalisation. A void point is never probed, counts no probes and writes 0 to every plane entry of its own.
 *
 * Cosine (dt_irradiance_cosine; csrc/dt_irr.h, one definition for host and kernel): for a normal n and a
 * direction dir,
 *   c(n, dir) = dmax(0.0, dot(n, normalized(dir)))       (csrc/dt_math.h: dot = (x*x' + y*y') + z*z',
 *                                                         normalized = dir / sqrt(dot(dir, dir)), dmax = std::max)
 * and c = 0.0 for a void dir (a non-finite component, or all zero).
 *
 * Direct: the probe of slot j (light L = light[j] of the scene) of sample s of point i is
 * dt_occlusion_light_ray(seed, frame, i, s, j, L, p), unchanged (purpose P_OLIGHT = 7), answered exactly as
 * dt_rays_occluded(start = p, dir, skip_shape = L.shape_index) answers it, its void-ray rule included: its
 * visibility is the probe behind dt_points_occlusion's light plane. With
 *   C_j = the f64 sum over s = 0 .. n_samples-1, ascending, from 0.0, of (unoccluded ? c(n, dir) : 0.0),
 *   direct[n_lights*i + j] = (float)(C_j / (double)n_samples),
 *   direct_rgb[3i + k]     = (float)(the f64 sum over j ascending, from 0.0, of
 *                                    L_j.color[k] * (C_j / (double)n_samples)).
 * There is no distance falloff (the render's lights have none), and the render's division by the number of
 * lights that contribute (rayColor's `hits`) is NOT applied: the planes are sums over the chosen slots.
 *
 * Gather (gather_rays = K > 0): probe r = 0 .. K-1 of sample s (dt_irradiance_gather_ray):
 *   ball = v(P_GATHER = 8, base = r)            the ball point of dt_render_occlusion, under a purpose of its own
 *   u = normalized(ball),  dir = n + u,  start = p + 1e-3*dir      (each operation one rounded f64 one)
 * which is cosine-weighted about a unit n. The probe is VOID if ball is the zero vector or dir is void
 * (dt_irradiance_gather_ray then gives dir = 0 and start = p); a void probe is not traced, contributes nothing
 * and still counts in the denominators. Otherwise it is answered exactly as dt_trace_rays(start, dir) answers
 * it: shape, q = point, nq = the fixNorm'ed normal, a = albedo (the base colour, texture and checker included).
 *   a miss:                         counts towards sky, contributes 0 light
 *   a shape with DT_F_LIGHT:        contributes a, and runs no light loop
 *   any other shape:                per slot j one probe from q by the light-probe rule of dt_render_occlusion
 *     under the purpose P_GLIGHT = 9 and the generalised slot r*DT_OCCL_MAX_LIGHTS + j in the place of j (the
 *     words at sub = slot*16, the ball at base = slot), dir2 = T - q, answered as
 *     dt_rays_occluded(q, dir2, L_j.shape_index);
 *       E[k] = the f64 sum over j ascending, from 0.0, of L_j.color[k] * (unoccluded ? c(nq, dir2) : 0.0)
 *     and the contribution is a[k] * E[k].
 * With S[k] the f64 sum of the contributions over s ascending, then r ascending, from 0.0, and M the number
 * of probes that missed,
 *   indirect_rgb[3i + k] = (float)(S[k] / ((double)n_samples * (double)gather_rays)),
 *   sky[i]               = (float)((double)M / ((double)n_samples * (double)gather_rays)).
 * The estimator needs no pi: the cosine density of the probes cancels the Lambertian 1/pi. All sums are f64 per
 * point in a fixed order, so every plane is specified bit for bit.
 *
 * Limits: one bounce only; a mirror or a pane of glass met by a gather probe is shaded as diffuse with its base
 * colour; no probe passes through glass (a glass shape occludes, as in the light loop's shadow test); a light's
 * own shape shadows nothing of that light, but a baked emitter still shadows itself against its own light's
 * probes from behind its surface, as in dt_points_occlusion.
 *
 * A plane that is not wanted costs nothing: the direct probes run iff direct or direct_rgb is given, the gather
 * probes iff indirect_rgb or sky is, their light probes (and the hit's attributes) iff indirect_rgb is.
 * stats (optional): shadow_rays = the shadow probes tested (the non-void ones, direct and from gather hits),
 * rays = the gather probes traced (the non-void ones), kernel_ms; everything else 0.
 *
 * Errors, with a dt_last_error starting "dt_points_irradiance: " and naming the argument, all before any
 * device work: DT_E_INVALID for a null scene, globals, point, normal, params or out, n_points < 0 or
 * n_points >= 2^32, n_samples outside 1..DT_POCCL_MAX_SAMPLES, n_lights outside 0..DT_OCCL_MAX_LIGHTS,
 * gather_rays outside 0..DT_OCCL_MAX_AO_RAYS, out->direct or out->direct_rgb given with n_lights == 0,
 * out->indirect_rgb given with gather_rays == 0 or with n_lights == 0, out->sky given with gather_rays == 0,
 * every plane NULL, a light index outside the scene; DT_E_UNSUPPORTED for a scene with a
 * RectPrismWithCylinder. n_points == 0: DT_OK, nothing is launched.
 *
 * The walks are dt_points_occlusion's wave-uniform ones, 64 consecutive points per wave: one shadow walk per
 * (slot, sample), then per (sample, gather probe) one closest-hit walk and one shadow walk per slot. Points
 * that are neighbours in the arrays should be neighbours in space (README.md). */
typedef struct dt_irradiance_params {
  int32_t n_lights;                    /* 0..DT_OCCL_MAX_LIGHTS */
  int32_t light[DT_OCCL_MAX_LIGHTS];   /* scene light indices, slot order */
  int32_t gather_rays;                 /* 0..DT_OCCL_MAX_AO_RAYS gather probes per sample */
} dt_irradiance_params;
typedef struct dt_irradiance {         /* each plane optional, not all NULL; all on one side */
  float* direct;       /* n_lights per point: entry n_lights*i + j, cosine-weighted visibility of slot j */
  float* direct_rgb;   /* 3 per point: sum over slots of colour_j * that mean */
  float* indirect_rgb; /* 3 per point (needs gather_rays > 0 and n_lights > 0) */
  float* sky;          /* 1 per point (needs gather_rays > 0): share of gather probes that hit nothing */
} dt_irradiance;
int dt_points_irradiance(const dt_scene* s, const dt_globals* g, int32_t frame, int64_t n_points,
                         const double* point, const double* normal,   /* 3 doubles per point each */
                         int32_t n_samples,                           /* 1..DT_POCCL_MAX_SAMPLES */
                         const dt_irradiance_params* params, const dt_irradiance* out,
                         int32_t on_device, void* stream, dt_stats* stats);
/* The gather probe r (0..DT_OCCL_MAX_AO_RAYS-1) of one sample and the cosine weight (csrc/dt_irr.h), for tests
 * and callers. No device work. DT_OK; a null argument or r outside its range: DT_E_INVALID. A void gather
 * probe gives dir = (0, 0, 0) and start = p. */
int dt_irradiance_gather_ray(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, int32_t r,
                             const double p[3], const double n[3], double start[3], double dir[3]);
int dt_irradiance_cosine(const double n[3], const double dir[3], double* c);

/* ---- mutual visibility between two point sets: which of these targets can each of those sources see? ----
 * No reference counterpart. dt_rays_occluded answers segments the caller builds one by one (48 bytes in and one
 * out per pair); this call answers all n_a x n_b pairs of two point sets with the segments built on the device:
 * 24 bytes per point go in, one bit per pair comes out, with the per-source and per-target counts and a
 * cosine-weighted sum. Line of sight and coverage (sensors against targets), potentially-visible sets,
 * deterministic area-light quadrature, the form-factor matrix of a radiosity solve.
 * a holds 3 doubles per source (n_a of them), b 3 per target (n_b); n_a and n_b below 2^31.
 *
 * Pair (i, j) is the segment start = a[3i..3i+2], dir = b[3j..3j+2] - start (component-wise, each one rounded
 * f64 subtraction). It is VISIBLE iff dt_rays_occluded(start, dir, skip_shape = skip_b ? skip_b[j] : -1) would
 * write 0 for it: the same gather along dir from start + 1e-3*dir, the same intersectShadow(sn, start + 1e-3*sn,
 * (float)|dir|) on every gathered shape but the skip shape, tree walks only. skip_b[j] is the shape target j is
 * or lies on (a light, a sensor; -1: none); there is no skip shape on the source's side, and the 1e-3 offset is
 * applied at the source only, so visibility is not exactly symmetric in a and b.
 *
 * A source or a target is VOID if its point has a non-finite component and, when out->weight_a is wanted, also
 * if its normal has one. A void source is never probed and writes 0 to its row of bits, its count_a and its
 * weight_a; a void target is never probed, has bit 0 in every row and count_b 0. Neighbours are unaffected.
 * A pair of two live points whose dir is a void ray by dt_rays_occluded's rule (all zero: a[i] == b[j]; or, by
 * overflow of the subtraction, non-finite) is not traced and counts as VISIBLE, as that call reports it: bit 1,
 * counted in count_a and count_b, weight 0.
 *
 * Weight (out->weight_a; needs normal_a and normal_b, taken as given: no fixNorm, no normalisation): with
 *   ca = dt_irradiance_cosine(normal_a[i], dir),  cb = dt_irradiance_cosine(normal_b[j], -dir),
 *   dd = dot(dir, dir) = (x*x + y*y) + z*z                                  (csrc/dt_math.h's order),
 *   w_ij = 0.0 for a pair that is not visible or whose dir is void, else ca*cb (falloff 0) or (ca*cb)/dd (1),
 * weight_a[i] is a sum in a FIXED order, so that the device may split the targets among workgroups:
 *   1. per tile of DT_PVIS_TILE consecutive targets (tile t: j = t*DT_PVIS_TILE .. min(n_b, (t+1)*DT_PVIS_TILE)-1)
 *      the f64 sum of w_ij in ascending j, from 0.0, every j of the tile adding its term (a 0.0 included);
 *   2. then the f64 sum of the tile sums in ascending t, from 0.0.
 * Every plane is so specified bit for bit. There is no pi and no area in the weight: callers scale. There is no
 * weight_b (it would need a sum across lanes): swap the sets.
 *
 * a, b, skip_b, the normals and the planes of out are all host (on_device=0: staged through temporaries, as
 * dt_points_occlusion stages its arrays) or all device (1). The call is synchronous, with a launch record,
 * counters and events of its own; it neither reads nor rebuilds the scene's primary-ray lists, and a render of
 * the scene afterwards is unaffected. g: as for the ray queries, only what traversal reads matters.
 * stats (optional): shadow_rays = the pairs traced (both points live, dir not void), kernel_ms; everything else
 * 0. A plane that is not wanted costs nothing: no cosine is evaluated without weight_a.
 *
 * Errors, with a dt_last_error starting "dt_points_visibility: " and naming the argument, all before any device
 * work: DT_E_INVALID for a null scene, globals, a, b, params or out, every plane NULL, n_a < 0 or n_b < 0, n_a or
 * n_b >= 2^31, out->weight_a given without both normals, falloff outside 0..1; DT_E_UNSUPPORTED for a scene with
 * a RectPrismWithCylinder. n_a == 0 or n_b == 0: DT_OK, nothing is launched, and every plane that has entries
 * (count_a with n_b == 0, count_b with n_a == 0, weight_a) is zeroed.
 *
 * The walk is the renders' wave-uniform one. A work item is 64 consecutive sources (a wave, one source per
 * lane) against DT_PVIS_TILE consecutive targets, one walk per target: the 64 segments of a walk end in one
 * point and skip one shape, so no grouping by skip shape is needed. Keep both arrays spatially ordered: sources
 * that are neighbours in a should be neighbours in space (README.md). bits needs n_a * ceil(n_b/32) words. */
#define DT_PVIS_TILE 256        /* targets per work item; a multiple of 32 */
typedef struct dt_visibility_params {
  const int32_t* skip_b;     /* optional, n_b entries: the shape target j is (a light, a sensor); treated per pair
                                exactly as dt_rays_occluded treats skip_shape */
  const double*  normal_a;   /* optional, 3 per source; required iff out->weight_a */
  const double*  normal_b;   /* optional, 3 per target; required iff out->weight_a */
  int32_t        falloff;    /* 0: weight = ca*cb; 1: weight = (ca*cb)/dd */
} dt_visibility_params;
typedef struct dt_visibility {   /* each plane optional, not all NULL; all on one side */
  uint32_t* bits;      /* n_a rows of W = ceil(n_b/32) words: bit (j & 31) of word j >> 5 of row i = pair (i,j) visible;
                          the unused high bits of a row's last word are 0 */
  int32_t*  count_a;   /* n_a: visible targets per source */
  int32_t*  count_b;   /* n_b: sources that see target j */
  double*   weight_a;  /* n_a: the weighted sum above */
} dt_visibility;
void dt_visibility_params_default(dt_visibility_params* p);   /* no skip shapes, no normals, falloff 0 */
int  dt_points_visibility(const dt_scene* s, const dt_globals* g, int64_t n_a, const double* a, int64_t n_b,
                          const double* b, const dt_visibility_params* params, const dt_visibility* out,
                          int32_t on_device, void* stream, dt_stats* stats);

/* ---- feature-guided denoising of previews: an edge-avoiding a-trous filter ----
 * No reference counterpart. The consumer of the feature buffers: (preview, albedo, normal, depth) ->
 * a clean preview, by the edge-avoiding a-trous wavelet filter of Dammertz et al. 2010, demodulated by
 * the first-hit albedo. Whole frames only, DT_OUT_IMAGE indexing, W = xRes, H = yRes: pixel slot
 * q = r*W + x with r the buffer row (a tile share or a slab lacks its neighbours and is not accepted:
 * gather the frame first). colour C[3q+k] is what dt_render / dt_resolve give (0..255); A, N (3 per
 * pixel) and Z (1 per pixel) are the albedo, normal and depth planes of dt_render_features. Coverage is
 * not read: A and N are premultiplied by it, which is what separates silhouette pixels.
 *
 * All arithmetic is IEEE f32, every operation below one rounded operation (no contraction), the same
 * on the host and on the device. Constants, computed on the host:
 *   isn = 1.0f/(sn*sn)   isa = 1.0f/(sa*sa)           sn, sz, sc, sa: sigma_normal, _depth, _colour, _albedo
 *   isc_l = 1.0f/((sc*2^-l)*(sc*2^-l))                the colour width halves per level
 *   isz_l = 1.0f/((sz*2^l)*(sz*2^l))                  the depth width grows with the step
 * Prepare, per pixel p:
 *   d[k] = demodulate ? fmaxf(A_p[k], 0.0625f) : 1.0f     E0_p[k] = C_p[k] / d[k]
 *   rz_p = 1.0f / (Z_p*Z_p + 1e-6f)
 * Level l = 0 .. levels-1, step s = 1 << l, pixel p = (r, x): taps j = -2..2 (outer), i = -2..2 (inner),
 * q = (r + j*s, x + i*s); a tap outside the image is skipped (no clamping, no mirroring):
 *   h  = K[|i|] * K[|j|]                     K = {0.375, 0.25, 0.0625}
 *   dn = N_p - N_q ; xn = ((dn0*dn0 + dn1*dn1) + dn2*dn2) * isn
 *   da = A_p - A_q ; xa = (same shape) * isa
 *   de = E_p - E_q ; xc = (same shape) * isc_l          (E: this level's input)
 *   dz = Z_p - Z_q ; xz = ((dz*dz) * rz_p) * isz_l
 *   R(x) = t*t with t = fmaxf(0.0f, 1.0f - x)           (fmaxf drops a NaN: weight 0)
 *   w  = (h * (R(xn) * R(xz))) * (R(xa) * R(xc))
 *   if (w > 0) { S[k] = S[k] + w * E_q[k] (k = 0,1,2) ; Wt = Wt + w }       S, Wt from 0
 *   E'_p[k] = Wt > 0 ? S[k] / Wt : E_p[k]
 * Finish: out[3p+k] = fminf(fmaxf(E_L[k] * d[k], 0.0f), 255.0f). A pixel whose input colour has a NaN
 * channel is copied to out unchanged (all three channels); by R it never contributes to a neighbour.
 * The edge-stopping function is a compact polynomial, not exp: no libm on either side, so the output
 * is specified bit for bit. Limits: first-hit guides only (a mirror's or a glass pane's reflection is
 * filtered by the colour term alone); one colour width for every pixel (dt_denoise_var below takes the
 * width per pixel from the adaptive sampler's variance).
 *
 * levels: 1..6. Each sigma > 0; +inf disables its term. dt_denoise_params_default: levels 5,
 * demodulate 1 and the sigmas chosen in BASELINE.md. */
typedef struct dt_denoise_params {
  int32_t levels;        /* 1..6 */
  int32_t demodulate;    /* 0 or 1 */
  float   sigma_normal;  /* edge-stopping width on the normal */
  float   sigma_depth;   /* ... on the relative depth */
  float   sigma_colour;  /* ... on the (demodulated) colour */
  float   sigma_albedo;  /* ... on the albedo */
} dt_denoise_params;

void    dt_denoise_params_default(dt_denoise_params* p);
/* the floats of scratch dt_denoise needs for an xRes x yRes frame (the ping-pong buffers of E and the
 * packed guides; the layout is the implementation's). < 0: xRes or yRes < 1, or p given and invalid. */
int64_t dt_denoise_workspace_floats(int32_t xRes, int32_t yRes, const dt_denoise_params* p);
/* feat needs albedo, normal and depth; its other planes are ignored. colour, the planes, out and work
 * all on one side: host (on_device=0: a plain loop) or device (1: kernels on `stream`, enqueue only;
 * with kernel_ms they are timed with HIP events and the call synchronises). out: 3*xRes*yRes floats,
 * not aliasing colour or work; nothing outside them is written. work: caller-owned,
 * dt_denoise_workspace_floats floats; nothing in it survives a call. No scene, globals or tiles: any
 * whole-frame image, a frame gathered from several ranks included. DT_E_INVALID before any device work,
 * with a dt_last_error naming the argument: a null argument or a missing plane, xRes or yRes < 1, levels
 * outside 1..6, demodulate not 0 or 1, a sigma that is <= 0 or NaN, aliasing. */
int     dt_denoise(int32_t xRes, int32_t yRes, const float* colour, const dt_features* feat,
                   const dt_denoise_params* p, float* out, float* work, int32_t on_device,
                   void* stream, float* kernel_ms);

/* ---- variance-guided preview denoising: the colour width from the adaptive sampler's sums ----
 * No reference counterpart. dt_variance turns the three buffers of dt_render_window_adaptive into a
 * plane: the variance of the mean of every channel's unclamped sample colours, in grey levels squared of
 * the 0..255 output. variance holds dt_accum_doubles(g, tiles) floats and is indexed like the
 * accumulator, so like the colour image, for DT_OUT_IMAGE and DT_OUT_SLAB alike (dt_unpack_slabs gathers
 * the planes of several ranks as it gathers their colours). Element i = 3q+k, n = (double)count[q], f64:
 *   n < 2 : variance[i] = 0.0f                              (no estimate: unowned pixel, 1-sample frame)
 *   else  : d = accum2[i] - (accum[i] * accum[i]) / n       (dt_adapt_converged's d, the same order)
 *           v = fmax(d, 0.0) / (n * (n - 1.0))              (fmax drops a NaN: 0)
 *           variance[i] = (float)(v * 65025.0)
 * One function on both sides, no contraction: host loop and kernel give the same bits. All four buffers
 * on one side: host (on_device=0) or device (1: one kernel on `stream`, enqueue only). A null pointer or
 * invalid g / tiles: DT_E_INVALID with a dt_last_error message, before any device work. */
int dt_variance(const dt_globals* g, const dt_tiles* tiles, const double* accum, const double* accum2,
                const uint32_t* count, float* variance, int32_t on_device, void* stream);

/* dt_denoise_var: dt_denoise's filter with the colour width of every pixel scaled by the standard
 * deviation of its own noise, and that variance filtered along with the colour (the scheme of SVGF,
 * Schied et al. 2017). Whole frames, DT_OUT_IMAGE indexing, C, A, N, Z as for dt_denoise; Vc[3q+k] is the
 * variance plane dt_variance gives. All arithmetic is IEEE f32, every operation below one rounded
 * operation (no contraction, no libm), the same on the host and on the device. Everything not restated
 * here is dt_denoise's. Constants, computed on the host:
 *   isn, isa, isz_l as in dt_denoise      sv2 = sv*sv, sv = sigma_variance      vf = variance_floor
 *   (the colour width does not halve per level: the variance it scales with shrinks as the filter proceeds)
 * Prepare, per pixel p: d[k], E0_p, rz_p as in dt_denoise, and one scalar, the variance of the
 * demodulated colour vector:
 *   x = ((Vc_p[0]/(d[0]*d[0])) + (Vc_p[1]/(d[1]*d[1]))) + (Vc_p[2]/(d[2]*d[2]))
 *   V0_p = fminf(fmaxf(x, 0.0f), 1e12f)        (a NaN or negative x: 0; the cap keeps w*w*V finite)
 * Level l, pixel p = (r, x), before the taps: the 3x3 prefiltered variance, step 1 at every level:
 *   sg = 0, gw = 0;  for b = -1..1 (outer, rows), a = -1..1 (inner), q = (r+b, x+a), a q outside the
 *   image skipped:   g = G[|a|] * G[|b|], G = {0.5, 0.25};   sg = sg + g * V_q;   gw = gw + g
 *   vbar_p = sg / gw          cv_p = 1.0f / (sv2 * (vbar_p + vf))
 * Taps: dt_denoise's 25 taps, order and skip rule; xn, xa, xz unchanged;
 *   xc = ((de0*de0 + de1*de1) + de2*de2) * cv_p
 *   w  = (h * (R(xn) * R(xz))) * (R(xa) * R(xc))
 *   if (w > 0) { S[k] = S[k] + w * E_q[k] ; Wt = Wt + w ; SV = SV + (w*w) * V_q }      S, Wt, SV from 0
 *   Wt > 0:  E'_p = S / Wt,  V'_p = SV / (Wt*Wt);     otherwise E'_p = E_p, V'_p = V_p
 * Finish and the NaN-colour pass-through: dt_denoise's. Two consequences: with sigma_variance = +inf,
 * cv = 0 and R(xc) = 1, and the output is dt_denoise's with sigma_colour = +inf and the same other
 * parameters, bit for bit; where cv_p * |E_p - E_q|^2 >= 1 the tap's weight is exactly 0.
 * Limits: first-hit guides only, as dt_denoise; the variance is the sampler's estimate from the samples
 * taken so far (0 below two samples, where only variance_floor sets the width); one frame alone (dt_reproject
 * below carries the samples of earlier frames over, and its out_var is a variance plane this filter takes).
 *
 * levels: 1..6. Each sigma > 0; +inf disables its term. variance_floor: finite, > 0.
 * dt_denoise_var_params_default: levels 5, demodulate 1 and the values chosen in BASELINE.md. */
typedef struct dt_denoise_var_params {
  int32_t levels;          /* 1..6 */
  int32_t demodulate;      /* 0 or 1 */
  float   sigma_normal;    /* edge-stopping widths on the guides, as dt_denoise_params */
  float   sigma_depth;
  float   sigma_albedo;
  float   sigma_variance;  /* colour width in standard deviations of the pixel's own noise; > 0, +inf disables */
  float   variance_floor;  /* added to the variance, demodulated grey levels squared; finite, > 0 */
  float   _pad;
} dt_denoise_var_params;

void    dt_denoise_var_params_default(dt_denoise_var_params* p);
/* as dt_denoise_workspace_floats (the same size: the variance travels in the fourth float of E's records) */
int64_t dt_denoise_var_workspace_floats(int32_t xRes, int32_t yRes, const dt_denoise_var_params* p);
/* dt_denoise's contract throughout: sides, workspace, kernel_ms, enqueue only on the device; out must not
 * alias colour, variance or work. variance: 3*xRes*yRes floats on the side of colour. DT_E_INVALID before
 * any device work, with a dt_last_error starting "dt_denoise_var: " and naming the argument: a null
 * argument or a missing plane, xRes or yRes < 1, levels outside 1..6, demodulate not 0 or 1, a sigma that
 * is <= 0 or NaN, a variance_floor that is <= 0, infinite or NaN, aliasing. */
int     dt_denoise_var(int32_t xRes, int32_t yRes, const float* colour, const float* variance,
                       const dt_features* feat, const dt_denoise_var_params* p, float* out, float* work,
                       int32_t on_device, void* stream, float* kernel_ms);

/* ---- temporal reuse for animation previews: reproject and accumulate frames ----
 * No reference counterpart. The third leg of the SVGF scheme (Schied et al. 2017) beside dt_denoise_var: the
 * previous frames' samples of the same surfaces, found by reprojecting every pixel's first hit into the
 * previous frame's camera, are blended with the current preview.
 *
 * dt_camera: the render's camera as a record. dt_camera_get fills it with exactly the values the renders
 * take from g (the functions of host_flatten.cpp that fill the device parameters: camera() for X, Y, Z from
 * eye, lookingAt and up, near_plane() for l, r, b, t from fov, aspect and near_plane). Host only; no scene,
 * no device. A null argument, xRes or yRes < 1: DT_E_INVALID; a degenerate gaze: DT_E_INVALID with the
 * renders' message ("Gaze direction can't be equal to up vector"). */
typedef struct dt_camera {
  double  eye[3], X[3], Y[3], Z[3];              /* the eye and the camera's right, up and backward unit vectors */
  float   l, r, b, t, near_plane, focal_length;  /* the near-plane window; rays are focal_length * dir (below) */
  int32_t xRes, yRes;
} dt_camera;

int dt_camera_get(const dt_globals* g, dt_camera* out);

/* dt_reproject: one call per frame. Whole frames only, DT_OUT_IMAGE indexing, W = xRes, H = yRes of both
 * cameras: render pixel (x, y) has slot q = (H-1-y)*W + x. Current frame: camera cur, colour C (3 per pixel,
 * 0..255, what dt_render / dt_resolve give), feat with the planes A (albedo), N (normal), Z (depth) of
 * dt_render_features and optionally shape; optionally the variance plane Vc (3 per pixel, dt_variance's).
 * Previous frame: camera prev, prev_feat with its A', N', Z' and optionally shape' (coverage is not
 * read), and the history record hist_in that the previous call wrote. A history record is three
 * caller-owned planes: colour (3 per pixel, demodulated), var (3 per pixel, present iff Vc is) and len (1 per
 * pixel: the number of frames in the pixel's history, a float). Outputs: out (3 per pixel: the accumulated
 * colour, remodulated and clamped to 0..255), the new history record hist_out, and out_var (3 per pixel,
 * present iff Vc is: the variance of out in dt_variance's units, a plane dt_denoise_var takes unchanged).
 * prev == NULL with prev_feat == NULL and hist_in == NULL: there is no history (the first frame of a
 * sequence, step 8 for every pixel). No output may alias an input or another output: the call gathers from
 * neighbours, and the caller ping-pongs two history records.
 *
 * All arithmetic is IEEE f32, every operation below one rounded operation (no contraction; sqrtf and /
 * correctly rounded; floorf exact; no other libm), the same on the host and on the device;
 * tests/temporal_ref.py restates it in numpy. dot(u, v) = (u0*v0 + u1*v1) + u2*v2. The cameras' eye, X, Y, Z
 * are converted to f32 once, on the host, before any pixel; primed names are prev's. Host constants:
 * nt2 = normal_tol * normal_tol, at2 = albedo_tol * albedo_tol. Per pixel p = (x, y), slot q:
 *  1 demodulate   d[k] = demodulate ? fmaxf(A_p[k], 0.0625f) : 1.0f      E_p[k] = C_p[k] / d[k]
 *                 Ve_p[k] = Vc_p[k] / (d[k]*d[k])
 *  2 direction    camera_ray's, from the pixel's corner:  a = l + ((r-l) * (float)x) / (float)W
 *                 b = b_ + ((t-b_) * (float)y) / (float)H  (b_: the record's b)
 *                 dir[k] = (a*X[k] + b*Y[k]) - near_plane*Z[k]
 *  3 world point  Z_p > 0:  s = Z_p / sqrtf(dot(dir, dir))   Pw[k] = eye[k] + s*dir[k]   v[k] = Pw[k] - eye'[k]
 *                           dq = sqrtf(dot(v, v))      (the depth plane is the mean distance from the lens,
 *                           whose samples are symmetric about eye: the pinhole point through its centre)
 *                 otherwise (sky, nothing hit; a NaN depth too):  v = dir, the pixel is a sky pixel
 *  4 project      zc = -dot(v, Z')       a' = (near_plane' * dot(v, X')) / zc      b' likewise with Y'
 *                 fx = ((a' - l') * (float)W) / (r' - l')      fy = ((b' - b_') * (float)H) / (t' - b_')
 *                 (an integer fx is a pixel: rays leave pixel corners). History is sought iff
 *                 zc > 0 and -1 < fx and fx < (float)W and -1 < fy and fy < (float)H   (false for a NaN;
 *                 decided before any conversion to int)
 *  5 taps         x0 = floorf(fx), tx = fx - x0, y0 = floorf(fy), ty = fy - y0; four taps in the order
 *                 (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with the weights
 *                 (1-tx)*(1-ty), tx*(1-ty), (1-tx)*ty, tx*ty. Tap (u, w_) has slot q' = (H-1-w_)*W + u in the
 *                 previous frame's planes. It is valid iff its weight w > 0, it lies inside the image,
 *                 hist_len[q'] > 0, no channel of hist_colour[q'] is a NaN,
 *                   depth:  fabsf(Z'[q'] - dq) <= depth_tol * dq;  for a sky pixel Z'[q'] == 0 instead
 *                   normal: dot(n, n) <= nt2 with n = N_p - N'[q']  (the premultiplied world-space normals
 *                           compare across cameras)
 *                   albedo: dot(m, m) <= at2 with m = A_p - A'[q']  (demodulation cannot carry a history across
 *                           an albedo edge where the colour is clamped at 255, the albedo is below the 0.0625
 *                           floor, or the surface is an emitter or a mirror; depth, normal and shape do
 *                           not see a texture's edge, or an emitter's edge under depth of field)
 *                   shape:  shape[q] == shape'[q'], when both shape planes are given
 *                 (a NaN guide fails its comparison: such a tap is not valid)
 *  6 gather       over the valid taps in tap order, all sums from 0:  Wt = Wt + w   S[k] = S[k] + w*hist_colour[k]
 *                 SL = SL + w*hist_len   SV[k] = SV[k] + w*hist_var[k];  with Wt > 0:
 *                 E_h = S / Wt   len_h = SL / Wt   V_h = SV / Wt    (the conservative form: interpolated
 *                 taps are not independent, so the variance is interpolated, not reduced)
 *  7 blend        n = fminf(len_h + 1.0f, max_history)      alpha = fmaxf(alpha_min, 1.0f / n)
 *                 E_out = E_h + alpha*(E_p - E_h)           u = 1.0f - alpha
 *                 V_out = (u*u)*V_h + (alpha*alpha)*Ve_p    len_out = n
 *                 out = fminf(fmaxf(E_out*d, 0.0f), 255.0f)  out_var = V_out*(d*d)
 *  8 no history   (no prev, history not sought, or Wt == 0): out = C_p bit for bit, E_out = E_p,
 *                 V_out = Ve_p, out_var = Vc_p bit for bit, len_out = 1
 *  9 NaN colour   a pixel whose C_p has a NaN channel is copied through as in 8 with len_out = 0: by the
 *                 rule on hist_len it is never anybody's history (dt_denoise's rule for such pixels)
 * hist_out holds E_out, V_out and len_out. With +inf a tolerance switches its test off for every tap whose
 * guides are numbers. Limits: a static world is assumed (there are no per-object motion vectors: a moving
 * shape is handled only by the rejection tests); first-hit guides, so a reflection is reprojected as if it
 * were painted on the mirror; the world point is the pinhole point, also under depth of field; whole
 * frames only (a tile share lacks the pixels its taps land on).
 *
 * dt_temporal_params_default: demodulate 1 and the values chosen in BASELINE.md. */
typedef struct dt_temporal_params {
  int32_t demodulate;    /* 0 or 1 */
  float   alpha_min;     /* the least weight of the current frame, in (0, 1] */
  float   max_history;   /* the cap on the history length, >= 1 */
  float   depth_tol;     /* relative depth difference a tap may have; >= 0, +inf: no depth test */
  float   normal_tol;    /* length of the normal difference a tap may have; >= 0, +inf: no normal test */
  float   albedo_tol;    /* length of the albedo difference a tap may have; >= 0, +inf: no albedo test */
} dt_temporal_params;

typedef struct dt_history {   /* caller-owned planes, all on the side of the call */
  float* colour;   /* 3 per pixel: the accumulated colour, demodulated */
  float* var;      /* 3 per pixel: its variance; present iff the call has a variance plane */
  float* len;      /* 1 per pixel: frames accumulated (0: a NaN-colour pixel) */
} dt_history;

void dt_temporal_params_default(dt_temporal_params* p);
/* Every plane on one side: host (on_device=0: a plain loop) or device (1: one kernel on `stream`, enqueue
 * only; with kernel_ms it is timed with HIP events and the call synchronises). Nothing outside the outputs
 * is written. DT_E_INVALID before any device work, with a dt_last_error starting "dt_reproject: " and naming
 * the argument: a null argument or a missing plane (feat's albedo, normal, depth; prev_feat's albedo, normal, depth;
 * a history record's colour and len, and its var iff variance is given; out_var iff variance is given),
 * prev, prev_feat and hist_in not all given or all NULL, a camera of another size than cur, xRes or
 * yRes < 1, demodulate not 0 or 1, alpha_min outside (0, 1], max_history < 1 or NaN, a tolerance that
 * is < 0 or NaN, aliasing. */
int dt_reproject(const dt_camera* cur, const float* colour, const float* variance, const dt_features* feat,
                 const dt_camera* prev, const dt_features* prev_feat, const dt_history* hist_in,
                 const dt_temporal_params* p, float* out, float* out_var, const dt_history* hist_out,
                 int32_t on_device, void* stream, float* kernel_ms);

/* ---- guided upsampling of previews: low-resolution lighting, full-resolution guides ----
 * No reference counterpart. Mixed-resolution preview: the lighting is traced at 1/s of the resolution in
 * each axis (1/s^2 of the rays), the guides (dt_render_features: albedo, normal, depth) at full
 * resolution, and dt_upsample reconstructs the full-resolution image by joint-bilateral upsampling
 * (Kopf et al. 2007) of the low-resolution colour demodulated by its albedo, steered by the
 * full-resolution guides and remodulated by the full-resolution albedo, which puts texture and checker
 * detail back at full sharpness. The camera makes the pixel correspondence exact: rays leave pixel
 * corners at l + (r-l)*x/W and `aspect` is a global of its own, so with W = s*w, H = s*h the
 * low-resolution pixel (x, y) covers exactly the full-resolution pixels s*x..s*x+s-1 by s*y..s*y+s-1,
 * and in buffer rows (DT_OUT_IMAGE indexing, rows flipped) full-resolution row R lies in low-resolution
 * row R div s.
 *
 * Whole frames only, DT_OUT_IMAGE indexing. W = xRes, H = yRes, s = factor, w = W/s, h = H/s. Primes mark
 * the low-resolution planes: C' (3 per pixel, what dt_render / dt_resolve / dt_denoise give at w x h),
 * A', N' (3 per pixel), Z' (1 per pixel) of feat_lo at w x h; A, N, Z of feat_hi at W x H. Coverage is not
 * read. All arithmetic is IEEE f32, every operation below one rounded operation (no contraction, no libm
 * beyond floorf, fabsf, fminf, fmaxf), the same on the host and on the device.
 *   dot(u,u) = (u0*u0 + u1*u1) + u2*u2
 * Constants, computed on the host:
 *   isn = 1.0f/(sn*sn)   isa = 1.0f/(sa*sa)   isz = 1.0f/(sz*sz)   fs = (float)s
 *                                                       sn, sz, sa: sigma_normal, _depth, _albedo
 * Low-resolution pixel q (computed per tap, nothing is stored):
 *   d'[k]   = demodulate ? fmaxf(A'_q[k], 0.0625f) : 1.0f
 *   E'_q[k] = C'_q[k] / d'[k]
 *   q is bad if any channel of C'_q is NaN
 * Full-resolution pixel p = (R, X), slot R*W + X:
 *   d[k] = demodulate ? fmaxf(A_p[k], 0.0625f) : 1.0f
 *   rz = 1.0f / (Z_p*Z_p + 1e-6f)
 *   xc = X / s ; rc = R / s                              (integer division)
 *   fx = ((float)X + 0.5f) / fs - 0.5f ; fy = ((float)R + 0.5f) / fs - 0.5f
 * Taps j = -1..1 (outer, rows), i = -1..1 (inner), q = (rc+j, xc+i); a tap outside the low-resolution
 * image is skipped (no clamping), a bad tap is skipped:
 *   T(t) = fmaxf(0.0f, 1.0f - fabsf(t) * 0.5f)           (a tent of half-width 2 low-resolution pixels)
 *   hsp  = T(fx - (float)(xc+i)) * T(fy - (float)(rc+j))
 *   xn = dot(N_p - N'_q) * isn
 *   xa = dot(A_p - A'_q) * isa
 *   dz = Z_p - Z'_q ; xz = ((dz*dz) * rz) * isz
 *   R(x) = t*t with t = fmaxf(0.0f, 1.0f - x)            (fmaxf drops a NaN: weight 0)
 *   w  = (hsp * (R(xn) * R(xz))) * R(xa)
 *   if (w > 0) { S[k] = S[k] + w * E'_q[k] (k = 0,1,2) ; Wt = Wt + w }       S, Wt from 0
 * Result:
 *   E[k] = Wt > 0 ? S[k] / Wt : E'_(rc,xc)[k]            (the fallback: the nearest low-resolution pixel)
 *   out[3p+k] = fminf(fmaxf(E[k] * d[k], 0.0f), 255.0f)
 *   if Wt == 0 and (rc, xc) is bad: out[3p+k] = C'_(rc,xc)[k], all three channels unchanged
 * Limits: the guides are first-hit only, so the contents of a mirror or a glass pane are upsampled by the
 * spatial term alone; the lighting keeps its low-resolution detail, so shadow edges and specular
 * highlights stay soft; whole frames only (a tile share or a slab lacks its neighbours).
 *
 * factor: 2, 3 or 4. Each sigma > 0; +inf disables its term. dt_upsample_params_default: factor 2,
 * demodulate 1 and the sigmas chosen in BASELINE.md. */
typedef struct dt_upsample_params {
  int32_t factor;        /* s: 2, 3 or 4 */
  int32_t demodulate;    /* 0 or 1 */
  float   sigma_normal;  /* > 0, +inf disables the term */
  float   sigma_depth;
  float   sigma_albedo;
  float   _pad;
} dt_upsample_params;

void dt_upsample_params_default(dt_upsample_params* p);
/* xRes, yRes: the full resolution W, H. colour_lo: 3*w*h floats; feat_lo, feat_hi need albedo, normal and
 * depth (at w x h and W x H), their other planes are ignored; out: 3*W*H floats. All on one side: host
 * (on_device=0: a plain loop) or device (1: one kernel on `stream`, enqueue only; with kernel_ms it is
 * timed with HIP events and the call synchronises). No workspace: E' is computed per tap. out must not
 * alias an input; nothing outside it is written. DT_E_INVALID before any device work, with a
 * dt_last_error starting "dt_upsample: " and naming the argument: a null argument or a missing plane,
 * xRes or yRes < 1, a factor outside 2..4, xRes or yRes not a multiple of the factor, demodulate not 0 or
 * 1, a sigma that is <= 0 or NaN, aliasing. */
int  dt_upsample(int32_t xRes, int32_t yRes, const float* colour_lo, const dt_features* feat_lo,
                 const dt_features* feat_hi, const dt_upsample_params* p, float* out, int32_t on_device,
                 void* stream, float* kernel_ms);

/* renderImageCloud (render_final_project.cpp:1224-1279). Sets eye/up/lookingAt as the
 * reference does (1227-1229) on a local copy; g is not modified. */
int dt_render_sky(const dt_globals* g, float frame, const dt_tiles* tiles, float* out,
                  int32_t out_on_device, void* stream, dt_stats* stats);

/* Scatter a gathered set of per-rank slabs (rank-major, each dt_slab_floats_max floats)
 * into the full ppmOut image (host or device, same side as inputs). */
int dt_unpack_slabs(const dt_globals* g, const dt_tiles* tiles, int32_t world,
                    const float* slabs, float* image, int32_t on_device, void* stream);

/* ---- host scene builders (scene.h) ---------------------------------------- */
/* name: "final" (buildFinal scene.h:605), "spheres" (buildSceneSpheres 4399),
 * "dof" (buildSceneDOF 4422), "hw4" (buildSceneHW4 4451), "prismcyl"
 * (BuildScenePrismCylinder 3227, the `./render prismcyl` mode, cpp:1711-1723).
 * Mutates g exactly as the reference builder mutates its globals (Q23, fresh-process
 * semantics: call dt_globals_default first for a fresh frame).
 * data_dir holds textures/<name>.rgb and bones_<motion>.bin. */
int  dt_build_scene(const char* name, float frame, dt_globals* g, const char* data_dir,
                    dt_scene_desc** out);
void dt_scene_desc_free(dt_scene_desc* d);

/* skeleton.cpp/motion.cpp/displaySkeleton.cpp forward kinematics: the 30 bone-cylinder
 * endpoints buildFinal places (scene.h:637-658) for each posture id in frames[]
 * (out: n_frames * n_bones * 6 doubles, left xyz + right xyz). out == NULL only reports
 * the bone and posture counts. Used by tools/gen_bones.py to make the data table. */
int dt_mocap_bone_table(const char* asf, const char* amc, const int32_t* frames, int32_t n_frames,
                        double* out, int32_t* n_bones, int32_t* n_postures);

/* test hook: the OBJ ingest of finalBuildModels (loadObj, objHelper.h:6-85) on one file. counts =
 * {vertices, texcoords, triangles}; with capacities >= those, v gets 3 floats per vertex, vt 2 per
 * texcoord and faces 6 int32 per triangle (3 vertex + 3 texcoord indices, 0-based, -1: none).
 * Null arrays only report the counts. */
int dt_debug_load_obj(const char* path, float* v, int64_t cap_v, float* vt, int64_t cap_vt, int32_t* faces,
                      int64_t cap_faces, int64_t counts[3]);

/* writePPM (helpers.h:174-195): float -> unsigned char truncation */
int dt_write_ppm(const char* filename, int32_t xRes, int32_t yRes, const float* values);
/* the same pixels as an 8-bit RGB PNG (the output surface beside PPM) */
int dt_write_png(const char* filename, int32_t xRes, int32_t yRes, const float* values);

#ifdef __cplusplus
}
#endif
#endif /* DT_H */
