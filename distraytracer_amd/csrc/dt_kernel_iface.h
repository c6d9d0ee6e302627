// dt_kernel_iface.h — every extern "C" symbol the kernel units (dt_kernels.hip and one .hip per auxiliary
// kernel family) export to the host library, declared once and
// included by both sides (tests/test_kernel_iface.py): a definition that disagrees with it does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

extern "C" size_t dt_launch_size(void);
extern "C" size_t dt_scene_struct_offset(void);
extern "C" size_t dt_scene_struct_size(void);
extern "C" size_t dt_params_struct_offset(void);
extern "C" hipError_t dt_launch_sky(const void* dev_launch, float* out, int64_t n_threads, hipStream_t stream);
extern "C" hipError_t dt_launch_sky_miss(const void* dev_launch, float* out, int64_t n_px, hipStream_t stream);
extern "C" hipError_t dt_launch_chunk_sum(const void* dev_launch, float* out, int64_t n_px, hipStream_t stream);
extern "C" hipError_t dt_launch_unpack(const void* dev_launch, int world, int64_t slab_floats, const float* slabs,
                                       float* image, hipStream_t stream);
extern "C" hipError_t dt_launch_normalize(const double* in, double* out, int64_t n, hipStream_t stream);
extern "C" hipError_t dt_launch_vdiv(const double* in, const double* den, double* out, unsigned long long* fallback,
                                     int64_t n, hipStream_t stream);
extern "C" hipError_t dt_launch_vnorm(const double* in, double* out, unsigned long long* fallback, int64_t n,
                                      hipStream_t stream);
// The trace-kernel builds, named once (dt_kernels.hip DT_TRACE_KERNEL, Makefile TRACE_BUILDS, in its
// order): per wave count (4, then 5) room, mesh, full (still frames), tunnel, blur (motion-blur frames)
// and sky; then the work-sharing and the RectPrismWithCylinder build. Each exists in three modes: the
// product build <k>, its window build <k>_win (DT_WINDOW, Makefile WIN_OBJ) and its adaptive window
// build <k>_awin (DT_WINDOW=2, AWIN_OBJ). The declarations here and dt_api.cpp's table g_builds come from this list.
#define DT_TRACE_BUILDS(X)                                                                               \
  X(dt_trace_kernel) X(dt_trace_kernel_mesh) X(dt_trace_kernel_full) X(dt_trace_kernel_tunnel)           \
  X(dt_trace_kernel_blur) X(dt_trace_kernel_sky) X(dt_trace_kernel_w5) X(dt_trace_kernel_w5_mesh)        \
  X(dt_trace_kernel_w5_full) X(dt_trace_kernel_w5_tunnel) X(dt_trace_kernel_w5_blur)                     \
  X(dt_trace_kernel_w5_sky) X(dt_trace_kernel_dn) X(dt_trace_kernel_rpc)
#define DT_TRACE_DECL(k)                                                                               \
  extern "C" hipError_t k##_launch(const void* dev_launch, float* out, int grid, hipStream_t stream); \
  extern "C" const void* k##_ptr(void);                                                                \
  extern "C" int k##_traits(void);
#define DT_TRACE_DECL3(k) DT_TRACE_DECL(k) DT_TRACE_DECL(k##_win) DT_TRACE_DECL(k##_awin)
DT_TRACE_BUILDS(DT_TRACE_DECL3)
#undef DT_TRACE_DECL3
#undef DT_TRACE_DECL
extern "C" hipError_t dt_launch_resolve(const double* accum, float* out, int64_t n_px, int n_samples,
                                        unsigned long long* nan_px, hipStream_t stream);
extern "C" hipError_t dt_launch_resolve_adaptive(const double* accum, const uint32_t* count, float* out, int64_t n_px,
                                                 unsigned long long* nan_px, hipStream_t stream);
extern "C" int64_t dt_adapt_select_blocks(int64_t n_items);
extern "C" hipError_t dt_launch_adapt_select(const void* dev_launch, int64_t n_items, hipStream_t stream);
extern "C" hipError_t dt_launch_isect(const void* dev_launch, int64_t first, int64_t n, int32_t* hit_shape, float* hit_t,
                                      int grid, hipStream_t stream);
extern "C" const void* dt_isect_kernel_ptr(void);
extern "C" hipError_t dt_launch_features(const void* dev_launch, int n_samples, float* albedo, float* normal, float* depth,
                                         float* coverage, int32_t* shape, int grid, hipStream_t stream);
extern "C" const void* dt_features_kernel_ptr(void);
extern "C" hipError_t dt_launch_features_path(const void* dev_launch, int n_samples, int max_bounces, float* albedo,
                                              float* normal, float* depth, float* coverage, int32_t* shape,
                                              float* bounces, int grid, hipStream_t stream);
extern "C" const void* dt_features_path_kernel_ptr(void);
extern "C" hipError_t dt_launch_rayq(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                     int32_t* shape, float* t, double* point, double* normal, double* albedo, int grid,
                                     hipStream_t stream);
extern "C" hipError_t dt_launch_rayq_occl(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                          const int32_t* skip_shape, uint8_t* occluded, int grid, hipStream_t stream);
extern "C" const void* dt_rayq_kernel_ptr(void);
extern "C" const void* dt_rayq_occl_kernel_ptr(void);
extern "C" hipError_t dt_launch_rayq_multi(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                           int k, int32_t* count, int32_t* shape, float* t, double* point,
                                           double* normal, double* albedo, int grid, hipStream_t stream);
extern "C" const void* dt_rayq_multi_kernel_ptr(int k);
extern "C" hipError_t dt_launch_mattes(const void* dev_launch, int n_samples, const int32_t* gmap, int layers, int32_t* id,
                                       float* weight, int32_t* distinct, unsigned long long* overflow, int grid,
                                       hipStream_t stream);
extern "C" const void* dt_mattes_kernel_ptr(void);
extern "C" hipError_t dt_launch_occlusion(const void* dev_launch, int n_samples, int ao_rays, float ao_radius, int n_lights,
                                          const void* lights, float* ao, float* light, int grid, hipStream_t stream);
extern "C" const void* dt_occlusion_kernel_ptr(void);
extern "C" hipError_t dt_launch_points_occl(const void* dev_launch, uint32_t seed, int32_t frame, int64_t n,
                                            const double* point, const double* normal, int n_samples, int ao_rays,
                                            float ao_radius, int n_lights, const void* lights, float* ao, float* light,
                                            int grid, hipStream_t stream);
extern "C" const void* dt_points_occl_kernel_ptr(void);
extern "C" hipError_t dt_launch_rayq_transmit(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                              const int32_t* skip_shape, int k, int32_t* panes, int32_t* pane_shape,
                                              int grid, hipStream_t stream);
extern "C" const void* dt_rayq_transmit_kernel_ptr(int k);
extern "C" hipError_t dt_launch_points_occl_glass(const void* dev_launch, uint32_t seed, int32_t frame, int64_t n,
                                                  const double* point, const double* normal, int n_samples,
                                                  int ao_rays, float ao_radius, int n_lights, const void* lights,
                                                  int max_panes, float* ao, float* light, float* ao_panes,
                                                  float* light_panes, int grid, hipStream_t stream);
extern "C" const void* dt_points_occl_glass_kernel_ptr(void);
extern "C" hipError_t dt_launch_points_irr(const void* dev_launch, uint32_t seed, int32_t frame, int64_t n,
                                           const double* point, const double* normal, int n_samples, int n_lights,
                                           const void* lights, int gather_rays, float* direct, float* direct_rgb,
                                           float* indirect_rgb, float* sky, int grid, hipStream_t stream);
extern "C" const void* dt_points_irr_kernel_ptr(void);
// partial: n_tiles * n_a doubles the weight reduction reads (null with weight_a: no cosines, no second kernel)
extern "C" hipError_t dt_launch_points_vis(const void* dev_launch, int64_t n_a, const double* a, int64_t n_b,
                                           const double* b, const int32_t* skip_b, const double* normal_a,
                                           const double* normal_b, int falloff, uint32_t* bits, int32_t* count_a,
                                           int32_t* count_b, double* partial, double* weight_a, int grid,
                                           hipStream_t stream);
extern "C" const void* dt_points_vis_kernel_ptr(void);
// planes: include/dt.h dt_ray_paths holding the device side of every plane (null: not wanted)
struct dt_ray_paths;
extern "C" hipError_t dt_launch_rayq_path(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                          int max_bounces, const struct dt_ray_paths* planes, int grid,
                                          hipStream_t stream);
extern "C" const void* dt_rayq_path_kernel_ptr(void);
extern "C" hipError_t dt_launch_camera_rays(const void* dev_launch, int sample_begin, int ns, int64_t n_rows,
                                            double* start, double* dir, hipStream_t stream);
