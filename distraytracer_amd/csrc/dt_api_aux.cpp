// dt_api_aux.cpp — the C-ABI entry points (include/dt.h) over the auxiliary kernels (the Makefile's AUX_BUILDS),
// all through AuxLaunch. The scene and render path is dt_api.cpp; what the two share is dt_api_internal.h.
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>

#include "dt_api_internal.h"
#include "dt_guide.h"
#include "dt_irr.h"
#include "dt_occl.h"

using namespace dth;

// a persistent kernel's resident waves, looked up once per kernel; callers may run on several threads
static int resident_waves(const void* kernel_fn)
{
  static std::mutex lock;
  static std::map<const void*, int> cache;
  std::lock_guard<std::mutex> hold(lock);
  int& resident = cache[kernel_fn];
  if (!resident) resident = max_resident_waves(kernel_fn, 64);
  return resident;
}

// the pixels a launch over P's items produces: the owned tiles' pixels inside the window (pixel_of's `valid`)
static uint64_t owned_pixels(const dtd::DParams& P)
{
  uint64_t pixels = 0;
  for (int64_t slot = 0; slot < P.n_owned_tiles; ++slot) {
    const int64_t t = dtd::tile_of(slot, P.rank, P.world);
    if (t >= P.n_tiles) continue;
    const int ty = (int)(t / P.tiles_x), tx = (int)(t - (int64_t)ty * P.tiles_x);
    const int xa = P.x0 + tx * P.tw, ya = P.y0 + ty * P.th;
    const int xb = xa + P.tw < P.x1 ? xa + P.tw : P.x1, yb = ya + P.th < P.y1 ? ya + P.th : P.y1;
    if (xb > xa && yb > ya) pixels += (uint64_t)(xb - xa) * (uint64_t)(yb - ya);
  }
  return pixels;
}

// One synchronous launch of an auxiliary kernel. The launch record, the counters and the two events are
// the call's own, so it may run beside renders of the same scene on other streams. The caller checks its
// arguments and calls prepare_render; then begin(), plane() per array, run() with the kernel's launch
// wrapper. Everything is released on every return path, after the stream's work that may use it; the
// record's host bytes live as long.
struct AuxLaunch {
  hipStream_t st;
  void* launch = nullptr;                     // the launch record on the device
  unsigned long long* counters = nullptr;     // device: ST_N counters, the queue word, begin()'s `extra` words
  std::vector<unsigned long long> h;          // ... as run() read them back
  float kernel_ms = 0;

  explicit AuxLaunch(void* stream) : st((hipStream_t)stream) {}
  AuxLaunch(const AuxLaunch&) = delete;
  ~AuxLaunch()
  {
    if (!bufs.empty()) (void)hipStreamSynchronize(st);
    for (void* b : bufs) (void)hipFree(b);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }

  // The scene on the device and the record of (scene, P) with zeroed counters of the call's own.
  // primary_lists: the launch shoots P's camera rays and shares the scene's primary-ray lists; without
  // them (rays that are not the camera's) the lists are neither read nor rebuilt. sc null (dt_camera_rays: a
  // kernel that reads the record's parameters only): the record of P with a zeroed scene, and counters
  // nobody adds to.
  int begin(dt_scene* sc, dtd::DParams& P, bool primary_lists, int extra = 0)
  {
    if (int rc = sc ? scene_upload(sc) : DT_OK) return rc;
    if (sc && primary_lists) {
      if (int rc = update_primary_lists(sc, P, true)) return rc;
    } else if (sc) {
      P.pl_block = P.pl_nbx = P.pl_nby = P.pl_bump = 0;
    }
    h.assign(ST_N + 1 + extra, 0);
    void* d = nullptr;
    if (int rc = alloc(dt_launch_size(), &launch)) return rc;
    if (int rc = alloc(h.size() * sizeof(h[0]), &d)) return rc;
    counters = (unsigned long long*)d;
    HIPCHK(hipMemsetAsync(counters, 0, h.size() * sizeof(h[0]), st));
    record.assign(dt_launch_size(), 0);
    if (sc) {
      HScene hs;
      fill_hscene(sc, hs);
      if (!primary_lists) hs.pl_cells = hs.pl_list = nullptr;
      hs.stats = counters;
      hs.queue = hs.stats + ST_N;
      memcpy(record.data() + dt_scene_struct_offset(), &hs, sizeof(hs));
    }
    memcpy(record.data() + dt_params_struct_offset(), &P, sizeof(P));
    HIPCHK(hipMemcpyAsync(launch, record.data(), record.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    return DT_OK;
  }

  // The device side of one of the caller's arrays: p itself when it is null or on the device, else a
  // temporary of `bytes`, holding p's bytes first (copy_in) and copied back to p by run() (copy_out).
  int plane(const void* p, size_t bytes, bool on_device, bool copy_in, bool copy_out, void** dev)
  {
    *dev = const_cast<void*>(p);
    if (!p || on_device) return DT_OK;
    if (int rc = alloc(bytes, dev)) return rc;
    if (copy_in) HIPCHK(hipMemcpyAsync(*dev, p, bytes, hipMemcpyHostToDevice, st));
    if (copy_out) back.push_back({const_cast<void*>(p), *dev, bytes});
    return DT_OK;
  }

  // a device temporary of the launch's own, released with it (contents undefined)
  int scratch(size_t bytes, void** dev) { return alloc(bytes, dev); }

  // the two 3 n double arrays a query reads (rays: start and dir; points: point and normal)
  int plane_pair(const double* a, const double* b, size_t n, bool on_device, const double** da, const double** db)
  {
    if (int rc = plane(a, 3 * n * sizeof(double), on_device, true, false, (void**)da)) return rc;
    return plane(b, 3 * n * sizeof(double), on_device, true, false, (void**)db);
  }

  // The launch, launch_fn(grid) being the kernel's launch wrapper: a persistent grid over `work` items or waves,
  // the kernel's resident waves at the most, one block at the least (kernel_fn null: the wrapper sizes its own).
  // Then the staged arrays and the counters back, the stream drained, the kernel's time.
  template <class Launch>
  int run(const void* kernel_fn, int64_t work, Launch launch_fn)
  {
    int grid = 0;
    if (kernel_fn) {
      const int resident = resident_waves(kernel_fn);
      grid = (int)(work < resident ? work : resident);
      if (grid < 1) grid = 1;
    }
    HIPCHK(hipEventRecord(e0, st));
    const hipError_t launched = launch_fn(grid);
    if (launched != hipSuccess)
      return fail(DT_E_NO_DEVICE, std::string("auxiliary kernel launch: ") + hipGetErrorString(launched));
    HIPCHK(hipEventRecord(e1, st));
    for (const Back& b : back) HIPCHK(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h.data(), counters, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipEventElapsedTime(&kernel_ms, e0, e1));
    return DT_OK;
  }

  // what a call reports in dt_stats (null: nothing). Pixel planes: P's owned pixels, a camera ray per sample
  void pixel_stats(dt_stats* stats, const dtd::DParams& P, int32_t n_samples) const
  {
    if (!stats) return;
    memset(stats, 0, sizeof(*stats));
    stats->pixels = owned_pixels(P);
    stats->samples = stats->pixels * (uint64_t)n_samples;
    stats->rays = stats->samples;
    stats->kernel_ms = kernel_ms;
  }
  // closest-hit queries (the caller zeroed stats)
  void hit_stats(dt_stats* stats) const
  {
    if (!stats) return;
    stats->rays = h[ST_RAYS];
    stats->tex_fetches = h[ST_TEX];
    stats->uv_out_of_range = h[ST_UV];
    stats->prism_norm_fallback = h[ST_PRISM];
    stats->kernel_ms = kernel_ms;
  }
  // shadow-ray queries (the caller zeroed stats)
  void shadow_stats(dt_stats* stats) const
  {
    if (!stats) return;
    stats->shadow_rays = h[ST_SHADOW];
    stats->kernel_ms = kernel_ms;
  }

 private:
  struct Back {
    void *host, *dev;
    size_t bytes;
  };
  std::vector<void*> bufs;
  std::vector<Back> back;
  std::vector<uint8_t> record;   // the launch record's host bytes
  hipEvent_t e0 = nullptr, e1 = nullptr;

  int alloc(size_t bytes, void** dev)
  {
    HIPCHK(hipMalloc(dev, bytes));
    bufs.push_back(*dev);
    return DT_OK;
  }
};

// prepare_render for the whole image on one rank
static int prepare_whole(const dt_scene* sc, const dt_globals* g, int32_t frame, dtd::DParams& P)
{
  std::vector<float> zs;
  dt_tiles whole;
  memset(&whole, 0, sizeof(whole));
  whole.world = 1;
  return prepare_render(sc, g, frame, &whole, P, zs);
}

// The front of the ray and point queries, around the call's own checks: its pointers (a, b: the 3 n doubles) ...
static int query_pointers(const std::string& who, const dt_scene* sc, const dt_globals* g, const char* a_name,
                          const double* a, const char* b_name, const double* b)
{
  if (!sc) return fail(DT_E_INVALID, who + "null scene");
  if (!g) return fail(DT_E_INVALID, who + "null globals");
  if (!a) return fail(DT_E_INVALID, who + "null " + a_name);
  if (!b) return fail(DT_E_INVALID, who + "null " + b_name);
  return DT_OK;
}

// ... and, after every argument check, the RectPrismWithCylinder rule, the zeroed stats and n == 0 (*done)
static int query_ready(const std::string& who, const dt_scene* sc, int64_t n, dt_stats* stats, bool* done)
{
  *done = true;
  if (sc->no_cull) return fail(DT_E_UNSUPPORTED, who + "scenes with a RectPrismWithCylinder");
  if (stats) memset(stats, 0, sizeof(*stats));
  *done = n == 0;
  return DT_OK;
}

extern "C" {

// Intersection micro-benchmark: dt_isect_kernel over rays first_ray .. first_ray+n_rays-1
// of the globals' camera.
int dt_intersect_primary(const dt_scene* sc_c, const dt_globals* g, int32_t frame, int64_t first_ray, int64_t n_rays,
                         int32_t* hit_shape, float* hit_t, int32_t out_on_device, void* stream, float* kernel_ms)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  if (!sc || !g || !hit_shape || !hit_t) return fail(DT_E_INVALID, "null argument");
  if (first_ray < 0 || n_rays < 0) return fail(DT_E_INVALID, "negative ray range");
  if (sc->no_cull) return fail(DT_E_UNSUPPORTED, "dt_intersect_primary: scenes with a RectPrismWithCylinder");
  if (n_rays == 0) {
    if (kernel_ms) *kernel_ms = 0;
    return DT_OK;
  }
  dtd::DParams P;
  if (int rc = prepare_whole(sc, g, frame, P)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, true)) return rc;
  void *dshape = nullptr, *dt_ = nullptr;
  if (int rc = aux.plane(hit_shape, (size_t)n_rays * sizeof(int32_t), out_on_device, false, true, &dshape)) return rc;
  if (int rc = aux.plane(hit_t, (size_t)n_rays * sizeof(float), out_on_device, false, true, &dt_)) return rc;
  if (int rc = aux.run(dt_isect_kernel_ptr(), (n_rays + 63) / 64, [&](int grid) {
        return dt_launch_isect(aux.launch, first_ray, n_rays, (int32_t*)dshape, (float*)dt_, grid, aux.st);
      }))
    return rc;
  if (kernel_ms) *kernel_ms = aux.kernel_ms;
  return DT_OK;
}

// Camera rays as arrays: dt_camera_rays_kernel over the rows of (g, tiles, the sample range). The camera is
// fill_params' (the renders'), no scene is involved: the launch record holds the parameters alone.
static int camera_rays_check(const char* who, const dt_globals* g, const dt_tiles* tiles, int32_t sample_begin,
                             int32_t sample_end, int32_t frame, dtd::DParams& P, int64_t& n_rows)
{
  const std::string w = std::string(who) + ": ";
  if (!g) return fail(DT_E_INVALID, w + "null globals");
  if (!(0 <= sample_begin && sample_begin < sample_end && sample_end - sample_begin <= DT_CAMERA_RAYS_MAX_SAMPLES))
    return fail(DT_E_INVALID, w + "samples [" + std::to_string(sample_begin) + "," + std::to_string(sample_end) +
                                  "): need 0 <= sample_begin < sample_end, at most " +
                                  std::to_string(DT_CAMERA_RAYS_MAX_SAMPLES) + " samples");
  std::string err;
  if (int rc = fill_params(*g, frame, tiles, P, err)) return fail(rc, w + "globals or tiles: " + err);
  const int64_t slots = P.layout == DT_OUT_SLAB ? P.n_owned_tiles * P.tw * P.th : (int64_t)P.xRes * P.yRes;
  n_rows = slots * (sample_end - sample_begin);
  return DT_OK;
}

int64_t dt_camera_rays_rows(const dt_globals* g, const dt_tiles* tiles, int32_t sample_begin, int32_t sample_end)
{
  dtd::DParams P;
  int64_t n_rows = 0;
  if (camera_rays_check("dt_camera_rays_rows", g, tiles, sample_begin, sample_end, 0, P, n_rows)) return -1;
  return n_rows;
}

int dt_camera_rays(const dt_globals* g, int32_t frame, const dt_tiles* tiles, int32_t sample_begin, int32_t sample_end,
                   double* start, double* dir, int32_t on_device, void* stream, float* kernel_ms)
{
  if (g && !start) return fail(DT_E_INVALID, "dt_camera_rays: null start");
  if (g && !dir) return fail(DT_E_INVALID, "dt_camera_rays: null dir");
  dtd::DParams P;
  int64_t n_rows = 0;
  if (int rc = camera_rays_check("dt_camera_rays", g, tiles, sample_begin, sample_end, frame, P, n_rows)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(nullptr, P, false)) return rc;
  // host arrays are staged through device copies of the caller's arrays: unowned rows go back as they came
  void *dstart = nullptr, *ddir = nullptr;
  const size_t bytes = (size_t)n_rows * 3 * sizeof(double);
  if (int rc = aux.plane(start, bytes, on_device, true, true, &dstart)) return rc;
  if (int rc = aux.plane(dir, bytes, on_device, true, true, &ddir)) return rc;
  if (int rc = aux.run(nullptr, 0, [&](int) {
        return dt_launch_camera_rays(aux.launch, sample_begin, sample_end - sample_begin, n_rows, (double*)dstart,
                                     (double*)ddir, aux.st);
      }))
    return rc;
  if (kernel_ms) *kernel_ms = aux.kernel_ms;
  return DT_OK;
}

// First-hit feature buffers: dt_features_kernel over the samples 0 .. n_samples-1 of every owned pixel.
// It shares only the scene's primary-ray lists. Every argument check comes before the scene is looked at.
// Specular-path feature buffers (dt_render_features_path, `path`): the same call with
// dt_features_path_kernel, max_bounces and one more plane; its errors carry its own prefix.
static int render_features_common(bool path, const dt_scene* sc_c, const dt_globals* g, int32_t frame,
                                  const dt_tiles* tiles, int32_t n_samples, int32_t max_bounces, const dt_features* out,
                                  float* bounces, int32_t out_on_device, void* stream, dt_stats* stats)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  const std::string who = path ? "dt_render_features_path: " : "dt_render_features: ";
  if (!sc) return fail(DT_E_INVALID, who + "null scene");
  if (!g) return fail(DT_E_INVALID, who + "null globals");
  if (!out) return fail(DT_E_INVALID, who + "null planes");
  if (!out->albedo && !out->normal && !out->depth && !out->coverage && !out->shape && !bounces)
    return fail(DT_E_INVALID, who + "no plane wanted (every pointer is null)");
  if (int rc = dt_window_check(g, 0, n_samples)) return path ? fail(rc, who + "n_samples: " + dt_last_error()) : rc;
  if (path && (max_bounces < 0 || max_bounces > DT_GUIDE_MAX_BOUNCES))
    return fail(DT_E_INVALID, who + "max_bounces must be in 0.." + std::to_string(DT_GUIDE_MAX_BOUNCES) + ", got " +
                                  std::to_string(max_bounces));
  if (sc->no_cull) return fail(DT_E_UNSUPPORTED, who + "scenes with a RectPrismWithCylinder");
  dtd::DParams P;
  std::vector<float> zs;
  if (int rc = prepare_render(sc, g, frame, tiles, P, zs)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, true)) return rc;
  // the planes' lengths (dt_accum_doubles). Host planes are staged through device copies of the caller's
  // arrays: the entries of pixels this rank does not own go back as they came
  const size_t n3 = P.layout == DT_OUT_SLAB ? (size_t)(P.n_owned_tiles * P.tw * P.th * 3) : (size_t)3 * P.xRes * P.yRes;
  const size_t n1 = n3 / 3;
  void* host[6] = {out->albedo, out->normal, out->depth, out->coverage, out->shape, bounces};
  void* dev[6];
  const size_t bytes[6] = {n3 * sizeof(float), n3 * sizeof(float), n1 * sizeof(float),
                           n1 * sizeof(float), n1 * sizeof(int32_t), n1 * sizeof(float)};
  for (int k = 0; k < 6; ++k)
    if (int rc = aux.plane(host[k], bytes[k], out_on_device, true, true, &dev[k])) return rc;
  const void* kernel = path ? dt_features_path_kernel_ptr() : dt_features_kernel_ptr();
  if (int rc = aux.run(kernel, P.n_items, [&](int grid) {
        return path ? dt_launch_features_path(aux.launch, n_samples, max_bounces, (float*)dev[0], (float*)dev[1],
                                              (float*)dev[2], (float*)dev[3], (int32_t*)dev[4], (float*)dev[5], grid,
                                              aux.st)
                    : dt_launch_features(aux.launch, n_samples, (float*)dev[0], (float*)dev[1], (float*)dev[2],
                                         (float*)dev[3], (int32_t*)dev[4], grid, aux.st);
      }))
    return rc;
  aux.pixel_stats(stats, P, n_samples);
  if (stats) {
    if (path) stats->rays = aux.h[ST_RAYS];   // path: the segments traced
    if (path) stats->reflect_errors = aux.h[ST_REFL];
    stats->tex_fetches = aux.h[ST_TEX];
    stats->uv_out_of_range = aux.h[ST_UV];
    stats->prism_norm_fallback = aux.h[ST_PRISM];
  }
  return DT_OK;
}

int dt_render_features(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles, int32_t n_samples,
                       const dt_features* out, int32_t out_on_device, void* stream, dt_stats* stats)
{
  return render_features_common(false, s, g, frame, tiles, n_samples, 0, out, nullptr, out_on_device, stream, stats);
}

int dt_render_features_path(const dt_scene* s, const dt_globals* g, int32_t frame, const dt_tiles* tiles,
                            int32_t n_samples, int32_t max_bounces, const dt_features* out, float* bounces,
                            int32_t out_on_device, void* stream, dt_stats* stats)
{
  return render_features_common(true, s, g, frame, tiles, n_samples, max_bounces, out, bounces, out_on_device, stream,
                                stats);
}

// The bounce rule of dt_render_features_path for one hit (dt_guide.h), for tests and callers.
int dt_guide_bounce(const dt_globals* g, int32_t material, uint32_t flags, int32_t inside, const double in[3],
                    const double n[3], const double p[3], double next_dir[3], double next_start[3])
{
  if (!g || !in || !n || !p || !next_dir || !next_start) return fail(DT_E_INVALID, "dt_guide_bounce: null argument");
  dtm::V3 nd = dtm::v3(0, 0, 0), ns = dtm::v3(0, 0, 0);
  bool refl_err = false;
  const int rc = dtd::guide_bounce(g->reflect, g->nogloss, g->refr_air, g->refr_glass, material, flags, inside,
                                   dtm::v3a(in), dtm::v3a(n), dtm::v3a(p), nd, ns, refl_err);
  if (rc != dtd::DT_GUIDE_STOP) {
    next_dir[0] = nd.x; next_dir[1] = nd.y; next_dir[2] = nd.z;
    next_start[0] = ns.x; next_start[1] = ns.y; next_start[2] = ns.z;
  }
  return rc;
}

// Object mattes: dt_mattes_kernel over the samples 0 .. n_samples-1 of every owned pixel. As
// dt_render_features it shares only the scene's primary-ray lists. Every argument check, the map's
// entries included, comes before any device work.
int dt_render_mattes(const dt_scene* sc_c, const dt_globals* g, int32_t frame, const dt_tiles* tiles, int32_t n_samples,
                     const int32_t* group_of_shape, int32_t n_shapes, int32_t layers, const dt_mattes* out,
                     int32_t out_on_device, void* stream, dt_stats* stats, uint64_t* overflow_pixels)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  if (!sc) return fail(DT_E_INVALID, "dt_render_mattes: null scene");
  if (!g) return fail(DT_E_INVALID, "dt_render_mattes: null globals");
  if (!out) return fail(DT_E_INVALID, "dt_render_mattes: null out");
  if (!out->id && !out->weight && !out->distinct)
    return fail(DT_E_INVALID, "dt_render_mattes: out wants no plane (every pointer is null)");
  if (int rc = dt_window_check(g, 0, n_samples))
    return fail(rc, std::string("dt_render_mattes: n_samples: ") + dt_last_error());
  if (layers < 1 || layers > DT_MATTE_MAX_LAYERS)
    return fail(DT_E_INVALID, "dt_render_mattes: layers " + std::to_string(layers) + " outside 1.." +
                                  std::to_string(DT_MATTE_MAX_LAYERS));
  if (n_shapes < 0) return fail(DT_E_INVALID, "dt_render_mattes: n_shapes " + std::to_string(n_shapes) + " is negative");
  if (group_of_shape)
    for (int32_t i = 0; i < n_shapes; ++i)
      if (group_of_shape[i] < 0)
        return fail(DT_E_INVALID, "dt_render_mattes: group_of_shape[" + std::to_string(i) + "] is negative");
  // (the scene is looked at only from here on)
  if ((size_t)n_shapes != sc->flat.hdr.size())
    return fail(DT_E_INVALID, "dt_render_mattes: n_shapes " + std::to_string(n_shapes) + ", the scene has " +
                                  std::to_string(sc->flat.hdr.size()) + " shapes");
  if (sc->no_cull) return fail(DT_E_UNSUPPORTED, "dt_render_mattes: scenes with a RectPrismWithCylinder");
  dtd::DParams P;
  std::vector<float> zs;
  if (int rc = prepare_render(sc, g, frame, tiles, P, zs)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, true, /*extra: the overflow count*/ 1)) return rc;
  void* map = nullptr;
  if (n_shapes > 0)
    if (int rc = aux.plane(group_of_shape, (size_t)n_shapes * sizeof(int32_t), false, true, false, &map)) return rc;
  // the planes, staged as dt_render_features stages its own
  const size_t n1 = P.layout == DT_OUT_SLAB ? (size_t)(P.n_owned_tiles * P.tw * P.th) : (size_t)P.xRes * P.yRes;
  void* host[3] = {out->id, out->weight, out->distinct};
  void* dev[3];
  const size_t bytes[3] = {n1 * layers * sizeof(int32_t), n1 * layers * sizeof(float), n1 * sizeof(int32_t)};
  for (int k = 0; k < 3; ++k)
    if (int rc = aux.plane(host[k], bytes[k], out_on_device, true, true, &dev[k])) return rc;
  if (int rc = aux.run(dt_mattes_kernel_ptr(), P.n_items, [&](int grid) {
        return dt_launch_mattes(aux.launch, n_samples, (const int32_t*)map, layers, (int32_t*)dev[0], (float*)dev[1],
                                (int32_t*)dev[2], aux.counters + ST_N + 1, grid, aux.st);
      }))
    return rc;
  if (overflow_pixels) *overflow_pixels = aux.h[ST_N + 1];
  aux.pixel_stats(stats, P, n_samples);
  return DT_OK;
}

// Ray queries (dt_trace_rays, dt_rays_occluded): dt_rayq_kernel / dt_rayq_occl_kernel over rays the caller
// hands over. A query takes only the traversal parameters from g (prepare_render at frame 0; the camera it
// fills in is not read): it neither reads nor rebuilds the scene's primary-ray lists, and a render afterwards
// finds the scene as it was.
// dt_trace_rays_multi (`multi`) is the same call with dt_rayq_multi_kernel in the smallest list capacity that
// holds k (dt_rayq_multi_kernel_ptr picks it, as the launch wrapper does), k entries per ray and plane, and
// the counts. host: the caller's planes (count, shape, t, point, normal, albedo).
static int trace_rays_common(bool multi, const dt_scene* sc_c, const dt_globals* g, int64_t n_rays, const double* start,
                             const double* dir, int32_t k, bool have_out, void* const host[6], int32_t on_device,
                             void* stream, dt_stats* stats)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  const std::string who = multi ? "dt_trace_rays_multi: " : "dt_trace_rays: ";
  if (int rc = query_pointers(who, sc, g, "start", start, "dir", dir)) return rc;
  if (!have_out) return fail(DT_E_INVALID, who + "null out");
  if (!host[0] && !host[1] && !host[2] && !host[3] && !host[4] && !host[5])
    return fail(DT_E_INVALID, who + "out wants no plane (every pointer is null)");
  if (n_rays < 0) return fail(DT_E_INVALID, who + "n_rays < 0");
  if (multi && (k < 1 || k > DT_MULTIHIT_MAX))
    return fail(DT_E_INVALID, who + "k = " + std::to_string(k) + " outside 1.." + std::to_string(DT_MULTIHIT_MAX));
  bool done;
  if (int rc = query_ready(who, sc, n_rays, stats, &done); rc || done) return rc;
  dtd::DParams P;
  if (int rc = prepare_whole(sc, g, 0, P)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, false)) return rc;
  const size_t n = (size_t)n_rays, nk = n * (size_t)k;
  const double *dstart = nullptr, *ddir = nullptr;
  if (int rc = aux.plane_pair(start, dir, n, on_device, &dstart, &ddir)) return rc;
  void* dev[6];
  const size_t bytes[6] = {n * sizeof(int32_t),      nk * sizeof(int32_t),     nk * sizeof(float),
                           3 * nk * sizeof(double),  3 * nk * sizeof(double),  3 * nk * sizeof(double)};
  for (int p = 0; p < 6; ++p)
    if (int rc = aux.plane(host[p], bytes[p], on_device, false, true, &dev[p])) return rc;
  const void* kernel = multi ? dt_rayq_multi_kernel_ptr(k) : dt_rayq_kernel_ptr();
  if (int rc = aux.run(kernel, (n_rays + 63) / 64, [&](int grid) {
        return multi ? dt_launch_rayq_multi(aux.launch, n_rays, dstart, ddir, k, (int32_t*)dev[0], (int32_t*)dev[1],
                                            (float*)dev[2], (double*)dev[3], (double*)dev[4], (double*)dev[5], grid,
                                            aux.st)
                     : dt_launch_rayq(aux.launch, n_rays, dstart, ddir, (int32_t*)dev[1], (float*)dev[2],
                                      (double*)dev[3], (double*)dev[4], (double*)dev[5], grid, aux.st);
      }))
    return rc;
  aux.hit_stats(stats);
  return DT_OK;
}

int dt_trace_rays(const dt_scene* s, const dt_globals* g, int64_t n_rays, const double* start, const double* dir,
                  const dt_ray_hits* out, int32_t on_device, void* stream, dt_stats* stats)
{
  void* const host[6] = {nullptr, out ? out->shape : nullptr, out ? out->t : nullptr, out ? out->point : nullptr,
                         out ? out->normal : nullptr, out ? out->albedo : nullptr};
  return trace_rays_common(false, s, g, n_rays, start, dir, 1, out != nullptr, host, on_device, stream, stats);
}

int dt_trace_rays_multi(const dt_scene* s, const dt_globals* g, int64_t n_rays, const double* start, const double* dir,
                        int32_t k, const dt_ray_multihits* out, int32_t on_device, void* stream, dt_stats* stats)
{
  void* const host[6] = {out ? out->count : nullptr, out ? out->shape : nullptr, out ? out->t : nullptr,
                         out ? out->point : nullptr, out ? out->normal : nullptr, out ? out->albedo : nullptr};
  return trace_rays_common(true, s, g, n_rays, start, dir, k, out != nullptr, host, on_device, stream, stats);
}

int dt_rays_occluded(const dt_scene* sc_c, const dt_globals* g, int64_t n_rays, const double* start, const double* dir,
                     const int32_t* skip_shape, uint8_t* occluded, int32_t on_device, void* stream, dt_stats* stats)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  const std::string who = "dt_rays_occluded: ";
  if (int rc = query_pointers(who, sc, g, "start", start, "dir", dir)) return rc;
  if (!occluded) return fail(DT_E_INVALID, who + "null occluded");
  if (n_rays < 0) return fail(DT_E_INVALID, who + "n_rays < 0");
  bool done;
  if (int rc = query_ready(who, sc, n_rays, stats, &done); rc || done) return rc;
  dtd::DParams P;
  if (int rc = prepare_whole(sc, g, 0, P)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, false)) return rc;
  const size_t n = (size_t)n_rays;
  const double *dstart = nullptr, *ddir = nullptr;
  void *dskip = nullptr, *docc = nullptr;
  if (int rc = aux.plane_pair(start, dir, n, on_device, &dstart, &ddir)) return rc;
  if (int rc = aux.plane(skip_shape, n * sizeof(int32_t), on_device, true, false, &dskip)) return rc;
  if (int rc = aux.plane(occluded, n, on_device, false, true, &docc)) return rc;
  if (int rc = aux.run(dt_rayq_occl_kernel_ptr(), (n_rays + 63) / 64, [&](int grid) {
        return dt_launch_rayq_occl(aux.launch, n_rays, dstart, ddir, (const int32_t*)dskip, (uint8_t*)docc, grid, aux.st);
      }))
    return rc;
  aux.shadow_stats(stats);
  return DT_OK;
}

// dt_rays_transmittance: dt_rayq_transmit_kernel in the smallest list capacity that holds the pane ids wanted
// (none without out->pane_shape; dt_rayq_transmit_kernel_ptr picks it, as the launch wrapper does)
int dt_rays_transmittance(const dt_scene* sc_c, const dt_globals* g, int64_t n_rays, const double* start,
                          const double* dir, const int32_t* skip_shape, int32_t k, const dt_ray_transmittance* out,
                          int32_t on_device, void* stream, dt_stats* stats)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  const std::string who = "dt_rays_transmittance: ";
  if (int rc = query_pointers(who, sc, g, "start", start, "dir", dir)) return rc;
  if (!out) return fail(DT_E_INVALID, who + "null out");
  if (!out->panes && !out->pane_shape) return fail(DT_E_INVALID, who + "out wants no plane (every pointer is null)");
  if (n_rays < 0) return fail(DT_E_INVALID, who + "n_rays < 0");
  if (k < 0 || k > DT_TRANSMIT_MAX_PANES)
    return fail(DT_E_INVALID, who + "k = " + std::to_string(k) + " outside 0.." + std::to_string(DT_TRANSMIT_MAX_PANES));
  if (out->pane_shape && k == 0) return fail(DT_E_INVALID, who + "out->pane_shape given with k == 0");
  bool done;
  if (int rc = query_ready(who, sc, n_rays, stats, &done); rc || done) return rc;
  dtd::DParams P;
  if (int rc = prepare_whole(sc, g, 0, P)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, false)) return rc;
  const size_t n = (size_t)n_rays;
  const double *dstart = nullptr, *ddir = nullptr;
  void *dskip = nullptr, *dpanes = nullptr, *dshape = nullptr;
  if (int rc = aux.plane_pair(start, dir, n, on_device, &dstart, &ddir)) return rc;
  if (int rc = aux.plane(skip_shape, n * sizeof(int32_t), on_device, true, false, &dskip)) return rc;
  if (int rc = aux.plane(out->panes, n * sizeof(int32_t), on_device, false, true, &dpanes)) return rc;
  if (int rc = aux.plane(out->pane_shape, n * (size_t)k * sizeof(int32_t), on_device, false, true, &dshape)) return rc;
  if (int rc = aux.run(dt_rayq_transmit_kernel_ptr(out->pane_shape ? k : 0), (n_rays + 63) / 64, [&](int grid) {
        return dt_launch_rayq_transmit(aux.launch, n_rays, dstart, ddir, (const int32_t*)dskip, k, (int32_t*)dpanes,
                                       (int32_t*)dshape, grid, aux.st);
      }))
    return rc;
  aux.shadow_stats(stats);
  return DT_OK;
}

// dt_trace_rays_path: dt_rayq_path_kernel over the caller's rays, a ray query as dt_trace_rays is one; the
// per-segment planes hold max_bounces + 1 entries per ray. The kernel takes the planes' device side in a
// dt_ray_paths of its own.
int dt_trace_rays_path(const dt_scene* sc_c, const dt_globals* g, int64_t n_rays, const double* start, const double* dir,
                       int32_t max_bounces, const dt_ray_paths* out, int32_t on_device, void* stream, dt_stats* stats)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  const std::string who = "dt_trace_rays_path: ";
  if (int rc = query_pointers(who, sc, g, "start", start, "dir", dir)) return rc;
  if (!out) return fail(DT_E_INVALID, who + "null out");
  void* const host[11] = {out->end,    out->segments, out->shape,      out->length,   out->point,    out->normal,
                          out->albedo, out->last_start, out->last_dir, out->seg_shape, out->seg_point};
  bool wanted = false;
  for (void* p : host) wanted = wanted || p;
  if (!wanted) return fail(DT_E_INVALID, who + "out wants no plane (every pointer is null)");
  if (n_rays < 0) return fail(DT_E_INVALID, who + "n_rays < 0");
  if (max_bounces < 0 || max_bounces > DT_RAY_PATH_MAX_BOUNCES)
    return fail(DT_E_INVALID, who + "max_bounces must be in 0.." + std::to_string(DT_RAY_PATH_MAX_BOUNCES) + ", got " +
                                  std::to_string(max_bounces));
  bool done;
  if (int rc = query_ready(who, sc, n_rays, stats, &done); rc || done) return rc;
  dtd::DParams P;
  if (int rc = prepare_whole(sc, g, 0, P)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, false)) return rc;
  const size_t n = (size_t)n_rays, ns = n * (size_t)(max_bounces + 1);
  const double *dstart = nullptr, *ddir = nullptr;
  if (int rc = aux.plane_pair(start, dir, n, on_device, &dstart, &ddir)) return rc;
  const size_t i32 = sizeof(int32_t), f64 = sizeof(double);
  const size_t bytes[11] = {n * i32,     n * i32,     n * i32,     n * f64,  3 * n * f64,  3 * n * f64,
                            3 * n * f64, 3 * n * f64, 3 * n * f64, ns * i32, 3 * ns * f64};
  void* dev[11];
  for (int p = 0; p < 11; ++p)
    if (int rc = aux.plane(host[p], bytes[p], on_device, false, true, &dev[p])) return rc;
  const dt_ray_paths planes = {(int32_t*)dev[0], (int32_t*)dev[1], (int32_t*)dev[2], (double*)dev[3],
                               (double*)dev[4],  (double*)dev[5],  (double*)dev[6],  (double*)dev[7],
                               (double*)dev[8],  (int32_t*)dev[9], (double*)dev[10]};
  if (int rc = aux.run(dt_rayq_path_kernel_ptr(), (n_rays + 63) / 64, [&](int grid) {
        return dt_launch_rayq_path(aux.launch, n_rays, dstart, ddir, max_bounces, &planes, grid, aux.st);
      }))
    return rc;
  aux.hit_stats(stats);
  if (stats) stats->reflect_errors = aux.h[ST_REFL];
  return DT_OK;
}

// Occlusion feature buffers: dt_occlusion_kernel over the samples 0 .. n_samples-1 of every owned pixel. As
// dt_render_features it shares only the scene's primary-ray lists. Every argument check, the light indices
// included, comes before any device work. The lights' records (dt_occl.h OcclLight, from the scene's flattened
// lights) travel with the launch.
void dt_occlusion_params_default(dt_occlusion_params* p)
{
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->ao_rays = 4;
  p->ao_radius = 1.0f;   // one world unit (include/dt.h: a choice, not a measurement)
}

// The rules dt_render_occlusion and dt_points_occlusion share for params and out (both non-null), under the
// caller's prefix: the counts and the radius, planes given without their count, every plane NULL, then (the
// scene is looked at only from there on) the light indices and the RectPrismWithCylinder rule.
static int check_occlusion(const std::string& who, const dt_scene* sc, const dt_occlusion_params* params,
                           const dt_occlusion* out)
{
  if (params->ao_rays < 0 || params->ao_rays > DT_OCCL_MAX_AO_RAYS)
    return fail(DT_E_INVALID, who + "ao_rays " + std::to_string(params->ao_rays) + " outside 0.." +
                                  std::to_string(DT_OCCL_MAX_AO_RAYS));
  if (params->n_lights < 0 || params->n_lights > DT_OCCL_MAX_LIGHTS)
    return fail(DT_E_INVALID, who + "n_lights " + std::to_string(params->n_lights) + " outside 0.." +
                                  std::to_string(DT_OCCL_MAX_LIGHTS));
  if (params->ao_rays > 0 && !(std::isfinite(params->ao_radius) && params->ao_radius > 0))
    return fail(DT_E_INVALID, who + "ao_radius must be finite and > 0");
  if (out->ao && params->ao_rays == 0) return fail(DT_E_INVALID, who + "out->ao given with ao_rays == 0");
  if (out->light && params->n_lights == 0) return fail(DT_E_INVALID, who + "out->light given with n_lights == 0");
  if (!out->ao && !out->light) return fail(DT_E_INVALID, who + "out wants no plane (every pointer is null)");
  // (the scene is looked at only from here on)
  const int32_t scene_lights = (int32_t)sc->flat.lights.size();
  for (int32_t j = 0; j < params->n_lights; ++j)
    if (params->lights[j] < 0 || params->lights[j] >= scene_lights)
      return fail(DT_E_INVALID, who + "lights[" + std::to_string(j) + "] = " + std::to_string(params->lights[j]) +
                                    ", the scene has " + std::to_string(scene_lights) + " lights");
  if (sc->no_cull) return fail(DT_E_UNSUPPORTED, who + "scenes with a RectPrismWithCylinder");
  return DT_OK;
}

// the chosen lights' records (dt_occl.h OcclLight) in the caller's recs, which the copy reads until the
// stream is drained, and their device copy (null without lights)
static int occlusion_lights(AuxLaunch& aux, const dt_scene* sc, const dt_occlusion_params* params, int n_lights,
                            dtd::OcclLight recs[DT_OCCL_MAX_LIGHTS], void** dlights)
{
  memset(recs, 0, sizeof(dtd::OcclLight) * DT_OCCL_MAX_LIGHTS);
  for (int j = 0; j < n_lights; ++j) {
    const dtd::DLight& L = sc->flat.lights[params->lights[j]];
    dtd::OcclLight& o = recs[j];
    o.type = L.type;
    o.shape_index = L.shape_index;
    o.radius = L.radius;
    for (int k = 0; k < 3; ++k) { o.center[k] = L.center[k]; o.A[k] = L.A[k]; o.B[k] = L.B[k]; o.D[k] = L.D[k]; }
  }
  *dlights = nullptr;
  if (n_lights <= 0) return DT_OK;
  return aux.plane(recs, sizeof(dtd::OcclLight) * DT_OCCL_MAX_LIGHTS, false, true, false, dlights);
}

int dt_render_occlusion(const dt_scene* sc_c, const dt_globals* g, int32_t frame, const dt_tiles* tiles, int32_t n_samples,
                        const dt_occlusion_params* params, const dt_occlusion* out, int32_t out_on_device, void* stream,
                        dt_stats* stats)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  const std::string who = "dt_render_occlusion: ";
  if (!sc) return fail(DT_E_INVALID, who + "null scene");
  if (!g) return fail(DT_E_INVALID, who + "null globals");
  if (!params) return fail(DT_E_INVALID, who + "null params");
  if (!out) return fail(DT_E_INVALID, who + "null out");
  if (int rc = dt_window_check(g, 0, n_samples)) return fail(rc, who + "n_samples: " + dt_last_error());
  if (int rc = check_occlusion(who, sc, params, out)) return rc;
  // a plane that is not wanted costs no probes
  const int ao_rays = out->ao ? params->ao_rays : 0, n_lights = out->light ? params->n_lights : 0;
  dtd::DParams P;
  std::vector<float> zs;
  if (int rc = prepare_render(sc, g, frame, tiles, P, zs)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, true)) return rc;
  dtd::OcclLight recs[DT_OCCL_MAX_LIGHTS];
  void* dlights = nullptr;
  if (int rc = occlusion_lights(aux, sc, params, n_lights, recs, &dlights)) return rc;
  // the planes, staged as dt_render_features stages its own
  const size_t n1 = P.layout == DT_OUT_SLAB ? (size_t)(P.n_owned_tiles * P.tw * P.th) : (size_t)P.xRes * P.yRes;
  void *dao = nullptr, *dlight = nullptr;
  if (int rc = aux.plane(out->ao, n1 * sizeof(float), out_on_device, true, true, &dao)) return rc;
  if (int rc = aux.plane(out->light, n1 * (size_t)params->n_lights * sizeof(float), out_on_device, true, true, &dlight))
    return rc;
  if (int rc = aux.run(dt_occlusion_kernel_ptr(), P.n_items, [&](int grid) {
        return dt_launch_occlusion(aux.launch, n_samples, ao_rays, params->ao_radius, n_lights, dlights, (float*)dao,
                                   (float*)dlight, grid, aux.st);
      }))
    return rc;
  aux.pixel_stats(stats, P, n_samples);
  if (stats) {
    stats->shadow_rays = aux.h[ST_SHADOW];
    stats->prism_norm_fallback = aux.h[ST_PRISM];
  }
  return DT_OK;
}

// Occlusion queries at surface points: dt_points_occl_kernel over the caller's points, one lane per point. As a
// ray query it takes only the traversal parameters from g (prepare_whole at frame 0, as dt_rays_occluded, so
// that a probe is answered as that call answers it); the RNG key (g->seed, frame) travels as kernel
// arguments. It neither reads nor rebuilds the primary-ray lists.
//
// dt_points_occlusion_glass is the same call with dt_points_occl_glass_kernel (glass: max_panes and the optional
// pane planes; a row of probes runs for either of its two planes).
static int points_occlusion_common(bool glass, const dt_scene* sc_c, const dt_globals* g, int32_t frame, int64_t n_points,
                                   const double* point, const double* normal, int32_t n_samples,
                                   const dt_occlusion_params* params, int32_t max_panes, const dt_occlusion* out,
                                   const dt_occlusion_panes* panes, int32_t on_device, void* stream, dt_stats* stats)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  const std::string who = glass ? "dt_points_occlusion_glass: " : "dt_points_occlusion: ";
  if (int rc = query_pointers(who, sc, g, "point", point, "normal", normal)) return rc;
  if (!params) return fail(DT_E_INVALID, who + "null params");
  if (!out) return fail(DT_E_INVALID, who + "null out");
  if (n_points < 0) return fail(DT_E_INVALID, who + "n_points < 0");
  if (n_points >= (int64_t)1 << 32) return fail(DT_E_INVALID, who + "n_points >= 2^32 (a point is the RNG counter's pixel)");
  if (n_samples < 1 || n_samples > DT_POCCL_MAX_SAMPLES)
    return fail(DT_E_INVALID, who + "n_samples " + std::to_string(n_samples) + " outside 1.." +
                                  std::to_string(DT_POCCL_MAX_SAMPLES));
  if (glass) {
    if (max_panes < 0 || max_panes > DT_TRANSMIT_MAX_PANES)
      return fail(DT_E_INVALID, who + "max_panes " + std::to_string(max_panes) + " outside 0.." +
                                    std::to_string(DT_TRANSMIT_MAX_PANES));
    if (panes && panes->ao_panes && params->ao_rays == 0)
      return fail(DT_E_INVALID, who + "panes->ao_panes given with ao_rays == 0");
    if (panes && panes->light_panes && params->n_lights == 0)
      return fail(DT_E_INVALID, who + "panes->light_panes given with n_lights == 0");
  }
  if (int rc = check_occlusion(who, sc, params, out)) return rc;
  bool done;
  if (int rc = query_ready(who, sc, n_points, stats, &done); rc || done) return rc;
  // a plane that is not wanted costs no probes
  float* const ao_panes = glass && panes ? panes->ao_panes : nullptr;
  float* const light_panes = glass && panes ? panes->light_panes : nullptr;
  const int ao_rays = (out->ao || ao_panes) ? params->ao_rays : 0;
  const int n_lights = (out->light || light_panes) ? params->n_lights : 0;
  dtd::DParams P;
  if (int rc = prepare_whole(sc, g, 0, P)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, false)) return rc;
  dtd::OcclLight recs[DT_OCCL_MAX_LIGHTS];
  void* dlights = nullptr;
  if (int rc = occlusion_lights(aux, sc, params, n_lights, recs, &dlights)) return rc;
  const size_t n = (size_t)n_points;
  const double *dpoint = nullptr, *dnormal = nullptr;
  void *dao = nullptr, *dlight = nullptr, *daop = nullptr, *dlp = nullptr;
  if (int rc = aux.plane_pair(point, normal, n, on_device, &dpoint, &dnormal)) return rc;
  if (int rc = aux.plane(out->ao, n * sizeof(float), on_device, false, true, &dao)) return rc;
  if (int rc = aux.plane(out->light, n * (size_t)params->n_lights * sizeof(float), on_device, false, true, &dlight))
    return rc;
  if (int rc = aux.plane(ao_panes, n * sizeof(float), on_device, false, true, &daop)) return rc;
  if (int rc = aux.plane(light_panes, n * (size_t)params->n_lights * sizeof(float), on_device, false, true, &dlp))
    return rc;
  const void* kernel = glass ? dt_points_occl_glass_kernel_ptr() : dt_points_occl_kernel_ptr();
  if (int rc = aux.run(kernel, (n_points + 63) / 64, [&](int grid) {
        return glass ? dt_launch_points_occl_glass(aux.launch, (uint32_t)g->seed, frame, n_points, dpoint, dnormal,
                                                   n_samples, ao_rays, params->ao_radius, n_lights, dlights, max_panes,
                                                   (float*)dao, (float*)dlight, (float*)daop, (float*)dlp, grid, aux.st)
                     : dt_launch_points_occl(aux.launch, (uint32_t)g->seed, frame, n_points, dpoint, dnormal, n_samples,
                                             ao_rays, params->ao_radius, n_lights, dlights, (float*)dao, (float*)dlight,
                                             grid, aux.st);
      }))
    return rc;
  aux.shadow_stats(stats);
  return DT_OK;
}

int dt_points_occlusion(const dt_scene* s, const dt_globals* g, int32_t frame, int64_t n_points, const double* point,
                        const double* normal, int32_t n_samples, const dt_occlusion_params* params,
                        const dt_occlusion* out, int32_t on_device, void* stream, dt_stats* stats)
{
  return points_occlusion_common(false, s, g, frame, n_points, point, normal, n_samples, params, 0, out, nullptr,
                                 on_device, stream, stats);
}

int dt_points_occlusion_glass(const dt_scene* s, const dt_globals* g, int32_t frame, int64_t n_points, const double* point,
                              const double* normal, int32_t n_samples, const dt_occlusion_params* params,
                              int32_t max_panes, const dt_occlusion* out, const dt_occlusion_panes* panes,
                              int32_t on_device, void* stream, dt_stats* stats)
{
  return points_occlusion_common(true, s, g, frame, n_points, point, normal, n_samples, params, max_panes, out, panes,
                                 on_device, stream, stats);
}

// The two probe generators of dt_render_occlusion for one hit (dt_occl.h), for tests and callers.
int dt_occlusion_ao_ray(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, int32_t r, float ao_radius,
                        const double p[3], const double n[3], double dir[3])
{
  if (!p || !n || !dir) return fail(DT_E_INVALID, "dt_occlusion_ao_ray: null argument");
  if (r < 0 || r >= DT_OCCL_MAX_AO_RAYS)
    return fail(DT_E_INVALID, "dt_occlusion_ao_ray: r " + std::to_string(r) + " outside 0.." +
                                  std::to_string(DT_OCCL_MAX_AO_RAYS - 1));
  const dtm::V3 d = dtd::occl_ao_dir(seed, frame, pixel, sample, r, ao_radius, dtm::v3a(n));
  dir[0] = d.x; dir[1] = d.y; dir[2] = d.z;
  return DT_OK;
}

int dt_occlusion_light_ray(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, int32_t j,
                           const dt_light_desc* light, const double p[3], double dir[3])
{
  if (!light || !p || !dir) return fail(DT_E_INVALID, "dt_occlusion_light_ray: null argument");
  if (j < 0 || j >= DT_OCCL_MAX_LIGHTS)
    return fail(DT_E_INVALID, "dt_occlusion_light_ray: j " + std::to_string(j) + " outside 0.." +
                                  std::to_string(DT_OCCL_MAX_LIGHTS - 1));
  dtd::OcclLight o;
  memset(&o, 0, sizeof(o));
  o.type = light->type;
  o.shape_index = light->shape_index;
  o.radius = (double)light->radius;
  for (int k = 0; k < 3; ++k) { o.center[k] = light->center[k]; o.A[k] = light->A[k]; o.B[k] = light->B[k]; o.D[k] = light->D[k]; }
  const dtm::V3 d = dtd::occl_light_dir(seed, frame, pixel, sample, j, o, dtm::v3a(p));
  dir[0] = d.x; dir[1] = d.y; dir[2] = d.z;
  return DT_OK;
}

// Irradiance queries at surface points: dt_points_irr_kernel over the caller's points, one lane per point. The
// front, the traversal parameters, the RNG key and the staging are dt_points_occlusion's; the lights' records
// (dt_irr.h IrrLight: the probe's OcclLight and the light's colour) travel with the launch. Every argument
// check comes before any device work.
int dt_points_irradiance(const dt_scene* sc_c, const dt_globals* g, int32_t frame, int64_t n_points, const double* point,
                         const double* normal, int32_t n_samples, const dt_irradiance_params* params,
                         const dt_irradiance* out, int32_t on_device, void* stream, dt_stats* stats)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  const std::string who = "dt_points_irradiance: ";
  if (int rc = query_pointers(who, sc, g, "point", point, "normal", normal)) return rc;
  if (!params) return fail(DT_E_INVALID, who + "null params");
  if (!out) return fail(DT_E_INVALID, who + "null out");
  if (n_points < 0) return fail(DT_E_INVALID, who + "n_points < 0");
  if (n_points >= (int64_t)1 << 32) return fail(DT_E_INVALID, who + "n_points >= 2^32 (a point is the RNG counter's pixel)");
  if (n_samples < 1 || n_samples > DT_POCCL_MAX_SAMPLES)
    return fail(DT_E_INVALID, who + "n_samples " + std::to_string(n_samples) + " outside 1.." +
                                  std::to_string(DT_POCCL_MAX_SAMPLES));
  if (params->n_lights < 0 || params->n_lights > DT_OCCL_MAX_LIGHTS)
    return fail(DT_E_INVALID, who + "n_lights " + std::to_string(params->n_lights) + " outside 0.." +
                                  std::to_string(DT_OCCL_MAX_LIGHTS));
  if (params->gather_rays < 0 || params->gather_rays > DT_OCCL_MAX_AO_RAYS)
    return fail(DT_E_INVALID, who + "gather_rays " + std::to_string(params->gather_rays) + " outside 0.." +
                                  std::to_string(DT_OCCL_MAX_AO_RAYS));
  if (out->direct && params->n_lights == 0) return fail(DT_E_INVALID, who + "out->direct given with n_lights == 0");
  if (out->direct_rgb && params->n_lights == 0)
    return fail(DT_E_INVALID, who + "out->direct_rgb given with n_lights == 0");
  if (out->indirect_rgb && params->gather_rays == 0)
    return fail(DT_E_INVALID, who + "out->indirect_rgb given with gather_rays == 0");
  if (out->indirect_rgb && params->n_lights == 0)
    return fail(DT_E_INVALID, who + "out->indirect_rgb given with n_lights == 0");
  if (out->sky && params->gather_rays == 0) return fail(DT_E_INVALID, who + "out->sky given with gather_rays == 0");
  if (!out->direct && !out->direct_rgb && !out->indirect_rgb && !out->sky)
    return fail(DT_E_INVALID, who + "out wants no plane (every pointer is null)");
  // (the scene is looked at only from here on)
  const int32_t scene_lights = (int32_t)sc->flat.lights.size();
  for (int32_t j = 0; j < params->n_lights; ++j)
    if (params->light[j] < 0 || params->light[j] >= scene_lights)
      return fail(DT_E_INVALID, who + "light[" + std::to_string(j) + "] = " + std::to_string(params->light[j]) +
                                    ", the scene has " + std::to_string(scene_lights) + " lights");
  bool done;
  if (int rc = query_ready(who, sc, n_points, stats, &done); rc || done) return rc;
  dtd::DParams P;
  if (int rc = prepare_whole(sc, g, 0, P)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, false)) return rc;
  // the chosen lights' records, which the copy reads until the stream is drained
  dtd::IrrLight recs[DT_OCCL_MAX_LIGHTS];
  memset(recs, 0, sizeof(recs));
  for (int j = 0; j < params->n_lights; ++j) {
    const dtd::DLight& L = sc->flat.lights[params->light[j]];
    dtd::IrrLight& o = recs[j];
    o.L.type = L.type;
    o.L.shape_index = L.shape_index;
    o.L.radius = L.radius;
    for (int k = 0; k < 3; ++k) {
      o.L.center[k] = L.center[k]; o.L.A[k] = L.A[k]; o.L.B[k] = L.B[k]; o.L.D[k] = L.D[k];
      o.color[k] = L.color[k];
    }
  }
  void* dlights = nullptr;
  if (params->n_lights > 0)
    if (int rc = aux.plane(recs, sizeof(recs), false, true, false, &dlights)) return rc;
  const size_t n = (size_t)n_points;
  const double *dpoint = nullptr, *dnormal = nullptr;
  if (int rc = aux.plane_pair(point, normal, n, on_device, &dpoint, &dnormal)) return rc;
  void* host[4] = {out->direct, out->direct_rgb, out->indirect_rgb, out->sky};
  void* dev[4];
  const size_t bytes[4] = {n * (size_t)params->n_lights * sizeof(float), 3 * n * sizeof(float), 3 * n * sizeof(float),
                           n * sizeof(float)};
  for (int k = 0; k < 4; ++k)
    if (int rc = aux.plane(host[k], bytes[k], on_device, false, true, &dev[k])) return rc;
  if (int rc = aux.run(dt_points_irr_kernel_ptr(), (n_points + 63) / 64, [&](int grid) {
        return dt_launch_points_irr(aux.launch, (uint32_t)g->seed, frame, n_points, dpoint, dnormal, n_samples,
                                    params->n_lights, dlights, params->gather_rays, (float*)dev[0], (float*)dev[1],
                                    (float*)dev[2], (float*)dev[3], grid, aux.st);
      }))
    return rc;
  aux.shadow_stats(stats);
  if (stats) stats->rays = aux.h[ST_RAYS];   // the gather probes traced, as dt_trace_rays counts its rays
  return DT_OK;
}

// The gather probe and the cosine weight of dt_points_irradiance for one point (dt_irr.h), for tests and callers.
int dt_irradiance_gather_ray(uint32_t seed, int32_t frame, uint32_t pixel, uint32_t sample, int32_t r, const double p[3],
                             const double n[3], double start[3], double dir[3])
{
  if (!p || !n || !start || !dir) return fail(DT_E_INVALID, "dt_irradiance_gather_ray: null argument");
  if (r < 0 || r >= DT_OCCL_MAX_AO_RAYS)
    return fail(DT_E_INVALID, "dt_irradiance_gather_ray: r " + std::to_string(r) + " outside 0.." +
                                  std::to_string(DT_OCCL_MAX_AO_RAYS - 1));
  dtm::V3 s, d;
  dtd::irr_gather_ray(seed, frame, pixel, sample, r, dtm::v3a(p), dtm::v3a(n), s, d);
  start[0] = s.x; start[1] = s.y; start[2] = s.z;
  dir[0] = d.x; dir[1] = d.y; dir[2] = d.z;
  return DT_OK;
}

int dt_irradiance_cosine(const double n[3], const double dir[3], double* c)
{
  if (!n || !dir || !c) return fail(DT_E_INVALID, "dt_irradiance_cosine: null argument");
  *c = dtd::irr_cosine(dtm::v3a(n), dtm::v3a(dir));
  return DT_OK;
}

// Mutual visibility of two point sets: dt_points_vis_kernel over (waves of 64 sources) x (tiles of DT_PVIS_TILE
// targets), then dt_points_vis_sum_kernel when weight_a is wanted. As a ray query it takes only the traversal
// parameters from g (prepare_whole at frame 0, as dt_rays_occluded, so that a pair is answered as that call
// answers it) and neither reads nor rebuilds the primary-ray lists. Every argument check comes before any
// device work. The two count planes are zeroed on the stream before the launch (the kernel adds to them); the
// tiles' partial weight sums live in a temporary of the launch's own.
void dt_visibility_params_default(dt_visibility_params* p)
{
  if (p) memset(p, 0, sizeof(*p));
}

int dt_points_visibility(const dt_scene* sc_c, const dt_globals* g, int64_t n_a, const double* a, int64_t n_b,
                         const double* b, const dt_visibility_params* params, const dt_visibility* out,
                         int32_t on_device, void* stream, dt_stats* stats)
{
  dt_scene* sc = const_cast<dt_scene*>(sc_c);
  const std::string who = "dt_points_visibility: ";
  if (int rc = query_pointers(who, sc, g, "a", a, "b", b)) return rc;
  if (!params) return fail(DT_E_INVALID, who + "null params");
  if (!out) return fail(DT_E_INVALID, who + "null out");
  if (!out->bits && !out->count_a && !out->count_b && !out->weight_a)
    return fail(DT_E_INVALID, who + "out wants no plane (every pointer is null)");
  if (n_a < 0) return fail(DT_E_INVALID, who + "n_a < 0");
  if (n_b < 0) return fail(DT_E_INVALID, who + "n_b < 0");
  if (n_a >= (int64_t)1 << 31) return fail(DT_E_INVALID, who + "n_a >= 2^31");
  if (n_b >= (int64_t)1 << 31) return fail(DT_E_INVALID, who + "n_b >= 2^31");
  if (out->weight_a && !params->normal_a) return fail(DT_E_INVALID, who + "out->weight_a given without params->normal_a");
  if (out->weight_a && !params->normal_b) return fail(DT_E_INVALID, who + "out->weight_a given without params->normal_b");
  if (params->falloff < 0 || params->falloff > 1)
    return fail(DT_E_INVALID, who + "falloff " + std::to_string(params->falloff) + " outside 0..1");
  const size_t na = (size_t)n_a, nb = (size_t)n_b, words = (nb + 31) / 32;
  const size_t n_tiles = (nb + DT_PVIS_TILE - 1) / DT_PVIS_TILE;
  bool done;
  if (int rc = query_ready(who, sc, (n_a && n_b) ? 1 : 0, stats, &done)) return rc;
  void* const host[4] = {out->bits, out->count_a, out->count_b, out->weight_a};
  const size_t bytes[4] = {na * words * sizeof(uint32_t), na * sizeof(int32_t), nb * sizeof(int32_t), na * sizeof(double)};
  if (done) {   // no pair: the planes that have entries are zeros
    hipStream_t st = (hipStream_t)stream;
    bool any = false;
    for (int k = 0; k < 4; ++k) {
      if (!host[k] || !bytes[k]) continue;
      if (on_device) {
        HIPCHK(hipMemsetAsync(host[k], 0, bytes[k], st));
        any = true;
      } else {
        memset(host[k], 0, bytes[k]);
      }
    }
    if (any) HIPCHK(hipStreamSynchronize(st));
    return DT_OK;
  }
  dtd::DParams P;
  if (int rc = prepare_whole(sc, g, 0, P)) return rc;
  AuxLaunch aux(stream);
  if (int rc = aux.begin(sc, P, false)) return rc;
  const double *da = nullptr, *db = nullptr, *dna = nullptr, *dnb = nullptr;
  void* dskip = nullptr;
  if (int rc = aux.plane(a, 3 * na * sizeof(double), on_device, true, false, (void**)&da)) return rc;
  if (int rc = aux.plane(b, 3 * nb * sizeof(double), on_device, true, false, (void**)&db)) return rc;
  if (int rc = aux.plane(params->skip_b, nb * sizeof(int32_t), on_device, true, false, &dskip)) return rc;
  if (out->weight_a) {   // the normals are read for the weight alone
    if (int rc = aux.plane(params->normal_a, 3 * na * sizeof(double), on_device, true, false, (void**)&dna)) return rc;
    if (int rc = aux.plane(params->normal_b, 3 * nb * sizeof(double), on_device, true, false, (void**)&dnb)) return rc;
  }
  void* dev[4];
  for (int k = 0; k < 4; ++k)
    if (int rc = aux.plane(host[k], bytes[k], on_device, false, true, &dev[k])) return rc;
  for (int k = 1; k <= 2; ++k)
    if (dev[k]) HIPCHK(hipMemsetAsync(dev[k], 0, bytes[k], aux.st));
  void* partial = nullptr;
  if (out->weight_a)
    if (int rc = aux.scratch(n_tiles * na * sizeof(double), &partial)) return rc;
  const int64_t items = (int64_t)((na + 63) / 64) * (int64_t)n_tiles;
  if (int rc = aux.run(dt_points_vis_kernel_ptr(), items, [&](int grid) {
        return dt_launch_points_vis(aux.launch, n_a, da, n_b, db, (const int32_t*)dskip, dna, dnb, params->falloff,
                                    (uint32_t*)dev[0], (int32_t*)dev[1], (int32_t*)dev[2], (double*)partial,
                                    (double*)dev[3], grid, aux.st);
      }))
    return rc;
  aux.shadow_stats(stats);
  return DT_OK;
}

}  // extern "C"
