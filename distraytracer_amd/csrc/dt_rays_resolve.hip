// dt_rays_resolve -- per-ray rows (the row order of dt_camera_rays) reduced to per-pixel planes: per owned pixel
// and component the f64 sum of its n_samples rows in ascending row order, divided by n_samples or by the number
// of rows that count, cast to float. No reference counterpart. The specification is the comment block of
// dt_rays_resolve in include/dt.h; tests/camera_rays_ref.py restates it in numpy, and the host loop, the kernel
// and that restatement agree bit for bit: the element is one function (rr::element, dt_rays_resolve.h) that
// the host loop and the kernel both call.
//
// The kernel is a lane per output element (pixel and component), each lane walking its pixel's rows: the
// lanes of a pixel read one row's `width` doubles side by side, a wave reads 64 / width pixels' rows, n_samples
// * width * 8 bytes apart, and walks each of those runs to its end, so every cache line it touches is used
// whole over the walk. Its stores are 256 contiguous bytes per wave. The summation order is the contract; an
// LDS-staged shape (a wave copying its pixels' rows in with whole-line loads first) was not built.
//
// A translation unit of its own, compiled once for both libraries: dt_kernels.hip's objects stay as they are.
// The error prefix, the 1-D grid and the (untimed) launch are dt_post.h's.
#include "dt_post.h"
#include "dt_rays_resolve.h"
#include "host_internal.h"

namespace {

__global__ __launch_bounds__(256) void dt_rays_resolve_kernel(rr::Args a)
{
  const int64_t n = a.n_slots * a.width;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) rr::element(a, e);
}

constexpr post::Fail rr_fail{"dt_rays_resolve"};

}  // namespace

extern "C" int dt_rays_resolve(const dt_globals* g, const dt_tiles* tiles, int32_t n_samples, int32_t width,
                               const double* values, const int32_t* shape, int32_t mode, float* out, float* coverage,
                               int32_t on_device, void* stream)
{
  if (!g) return rr_fail("null globals");
  if (!values) return rr_fail("null values");
  if (!out) return rr_fail("null out");
  if (n_samples < 1 || n_samples > DT_CAMERA_RAYS_MAX_SAMPLES)
    return rr_fail("n_samples " + std::to_string(n_samples) + " outside 1.." + std::to_string(DT_CAMERA_RAYS_MAX_SAMPLES));
  if (width < 1 || width > 3) return rr_fail("width " + std::to_string(width) + " outside 1..3");
  if (mode != DT_RESOLVE_MEAN && mode != DT_RESOLVE_HIT_MEAN) return rr_fail("mode " + std::to_string(mode) + " unknown");
  dtd::DParams P;
  std::string err;
  if (dth::fill_sky_params(*g, 0.0f, tiles, P, err)) return rr_fail("globals or tiles: " + err);
  rr::Args a;
  a.n_slots = P.layout == DT_OUT_SLAB ? P.n_owned_tiles * P.tw * P.th : (int64_t)P.xRes * P.yRes;
  a.n = n_samples; a.width = width; a.mode = mode;
  a.xRes = P.xRes; a.yRes = P.yRes; a.x0 = P.x0; a.y0 = P.y0; a.x1 = P.x1; a.y1 = P.y1;
  a.tw = P.tw; a.th = P.th; a.rank = P.rank; a.world = P.world; a.layout = P.layout; a.tiles_x = P.tiles_x;
  a.n_owned_tiles = P.n_owned_tiles; a.n_tiles = P.n_tiles;
  a.values = values; a.shape = shape; a.out = out; a.coverage = coverage;
  if (!on_device) {
    rr::host_loop(a);
    return DT_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  return post::launch(st, nullptr, rr_fail.who, [&] {   // untimed: nothing waits
    hipLaunchKernelGGL(dt_rays_resolve_kernel, post::linear_grid(a.n_slots * a.width, 1 << 20), dim3(256), 0, st, a);
    return hipGetLastError();
  });
}
