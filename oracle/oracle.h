/*
 * oracle.h — TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain C, gcc, -ffp-contract=off) of the reference's per-pixel
 * render loop. It is the parity checker for the HIP path and the CPU baseline leg of
 * bench.py; nothing in distraytracer_amd/ links or calls it. Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline may load it.
 *
 * Pinning status:
 *   - value noise (noise.h:25-136) is pinned bit-for-bit against the reference's own
 *     noise.h compiled as-is (oracle/ref/noise_harness.cpp -> oracle/_ref/libref_noise.so)
 *     and against the hand-derived anchors of SURVEY §8c.
 *   - geometry.cpp, as far as this file restates it (intersect / intersectShadow / intersectCap /
 *     getNorm / getBounds / getUV of the classes behind dt_shape_type, fixNorm, getBarycentricCoords3D,
 *     segmentIntersect's verdict, CheckerCylinder's objM, BoundingVolume), is pinned bit-for-bit against
 *     the reference's own geometry.cpp,
 *     compiled unmodified against the Eigen-API shim oracle/ref/eigen_shim
 *     (oracle/ref/geom_harness.cpp -> oracle/_ref/libref_geom.so -> tests/golden/geom_ref.npz,
 *     tests/test_oracle_geom.py). The shim and this file share their Eigen conventions (dot's summation
 *     order, normalized() of a zero vector): the program logic is pinned, Eigen's internals are not.
 *     Not compared (no restatement here, or no reference answer): intersectMax, buildCOB on its own,
 *     shortestLine's coefficients, lineIntersect, RectPrism / RectPrismWithHoles, and
 *     RectPrismWithCylinder::getNorm where the reference throws or answers from a stale lastHit.
 *   - render_final_project.cpp and helpers.h: rayColor and generateBVH are pinned ray by ray against the
 *     reference's own, included unmodified by oracle/ref/shade_harness.cpp (-> oracle/_ref/libref_shade_cr.so
 *     -> tests/golden/shade_ref.npz, tests/test_oracle_shade.py); its glossy, rectangle-light and sphere-light
 *     sampling and in_motion against a draw-tape build fed or_sample_color_log's draws
 *     (-> tests/golden/shade_sampling_ref.npz, tests/test_oracle_shade_sampling.py). Not pinned: the
 *     motion-blur re-trace, DoF and jitter generation (renderImage).
 *
 * RNG: the reference draws from random_device-seeded mt19937 (F7) and cannot be
 * reproduced; oracle and device share the counter-based stream documented in
 * DESIGN.md §RNG (Philox4x32-10).
 */
#ifndef DT_ORACLE_H
#define DT_ORACLE_H

#include "../include/dt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* noise.h */
double or_noise3d(int i, int x, int y, int z);
double or_smoothed3d(int i, int x, int y, int z);
double or_interpolated_noise3d(int i, double x, double y, double z);
double or_value_noise3d(double x, double y, double z);

/* render_final_project.cpp:146-192 */
void or_sky_color(const dt_globals* g, const double ray[3], double out[3]);
void or_cloud_color(const dt_globals* g, const double ray[3], const double origin[3],
                    float frame, double out[3]);

/* counter RNG (shared definition with the device path) */
void or_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
double or_u01(uint32_t w0, uint32_t w1);
double or_u32_01(uint32_t w);   /* area-light draws: one word per float */

/* renderImageCloud (cpp:1224-1279) on a pixel window / tile set */
int or_render_sky(const dt_globals* g, float frame, const dt_tiles* tiles, float* out,
                  int nthreads);

/* generateBVH (helpers.h:330-472) over all shapes */
int or_bvh(const dt_scene_desc* d, const dt_globals* g, dt_bvh_node* nodes, int cap,
           int* indices, int index_cap, int* n_nodes, int* n_indices);

/* renderImage pixel loop (cpp:965-1222) on a pixel window / tile set */
int or_render(const dt_scene_desc* d, const dt_globals* g, int frame, const dt_tiles* tiles,
              float* out, int nthreads, dt_stats* stats);

/* or_render, also adding the include/dt_work.h event counts of the reference's loop (every box
 * its gathers test, every intersect / intersectShadow call, light, BRDF, texel, sky march) into
 * work[DT_WK_N] (zeroed by the caller) */
int or_render_work(const dt_scene_desc* d, const dt_globals* g, int frame, const dt_tiles* tiles,
                   float* out, int nthreads, dt_stats* stats, uint64_t* work);

/* the intersection micro-benchmark's closest hits (include/dt.h dt_intersect_primary numbering) */
int or_primary_hit(const dt_scene_desc* d, const dt_globals* g, int frame, long long first, long long n,
                   int* shape, float* t, int nthreads);

/* the start and direction (n x 3 doubles each) of the rays or_primary_hit and dt_intersect_primary trace */
int or_primary_ray(const dt_globals* g, int frame, long long first, long long n, double* start, double* dir);

/* Test-only entry points to the geometry.cpp restatement (tests/test_oracle_geom.py). A shape is
 * (d, si): d->shapes[si], with d->holes for a RectPrismWithCylinder. They wrap the static functions
 * the render loop calls. *t / *inside keep the caller's value where the reference's method leaves its
 * reference parameter unwritten. */
int  or_shape_intersect(const dt_scene_desc* d, int si, const double ray[3], const double start[3], float* t,
                        int* inside, int* hole);
int  or_shape_color_after_hit(const dt_scene_desc* d, int si, const double ray[3], const double start[3],
                              double color[3]);
int  or_shape_shadow(const dt_scene_desc* d, int si, const double ray[3], const double start[3], float t_max);
int  or_shape_intersect_cap(const dt_scene_desc* d, int si, const double ray[3], const double start[3], float* t,
                            int* inside);
int  or_shape_norm(const dt_scene_desc* d, int si, const double p[3], int hole, double out[3]);
int  or_shape_uv(const dt_scene_desc* d, int si, const double p[3], double uv[2]);
void or_shape_bounds(const dt_scene_desc* d, int si, double lb[3], double ub[3]);
void or_checker_cyl_objM(const dt_scene_desc* d, int si, double out[16]);
int  or_box_intersect(const dt_scene_desc* d, int si, int leaf, const double ray[3], const double inv_ray[3],
                      const double start[3], double lb[3], double ub[3]);
void or_fix_norm(const double ray[3], const double nrm[3], double out[3]);
void or_barycentric3d(const double p[3], const double A[3], const double B[3], const double C[3], double out[3]);
int  or_segment_intersect(const double A[3], const double B[3], const double ray[3], const double origin[3]);

/* one rayColor call tree for a single pixel-sample (debug / unit tests) */
int or_sample_color(const dt_scene_desc* d, const dt_globals* g, int frame, int x, int y,
                    int sample, double out_color[3], int* out_hit);

/* or_sample_color, also returning what the reference's rayColor would have to be told to answer the same ray
 * (tests/test_oracle_shade_sampling.py): the uniform values the primary ray_color call tree consumed, in
 * consumption order, each as the double handed to the arithmetic (or_u32_01 for rect_sample's and the glossy
 * sample's two, or_u01 for the sphere light's two per attempt), and in_motion as that call left it. The DoF
 * and blur-time draws happen outside rayColor and are not logged, nor are the blur passes' own draws.
 * *n_draws counts every draw; draws[0 .. cap-1] receives the first cap of them (draws may be NULL). */
int or_sample_color_log(const dt_scene_desc* d, const dt_globals* g, int frame, int x, int y, int sample,
                        double out_color[3], int* out_hit, int* out_in_motion, double* draws, int cap,
                        int* n_draws);

#ifdef __cplusplus
}
#endif
#endif
