// dt_camera_rays.hip — the render's camera rays as arrays (dt_camera_rays).
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_device.h"

// Camera rays as arrays (include/dt.h dt_camera_rays; the CPU oracle's or_primary_ray is its counterpart): for
// the samples sample_begin .. sample_begin+ns-1 of every owned pixel the ray the trace kernel starts from --
// its RNG pixel, sample and key, and camera_ray itself -- written out as 3 doubles of start (the eye sample)
// and 3 of dir (the unnormalised ray through the focal point). No scene: only Lp->P is read.
// One ray per lane, rows in ascending order: row i is sample sample_begin + i % ns of output slot i / ns
// (dtd::slot_pixel), so a wave's 64 rows are 1536 contiguous bytes of each array in both layouts, whole
// cache lines but for the wave's two ends. The rows of slots the tile share does not own are not written.
// Below 2^32 rows (wave-uniform) the slot comes from a 32-bit division.
extern "C" __global__ void __launch_bounds__(256)
dt_camera_rays_kernel(const DLaunch* __restrict__ Lp, int sample_begin, int ns, int64_t n_rows,
                      double* __restrict__ start, double* __restrict__ dir)
{
  const DParams& P = Lp->P;
  Ctx c;
  c.S = &Lp->S;
  c.P = &P;
  c.rng.k0 = P.seed;
  c.rng.k1 = (uint32_t)P.frame;
  const bool small = n_rows <= 0xffffffffll;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * 256) {
    const int64_t q = small ? (int64_t)((uint32_t)i / (uint32_t)ns) : i / ns;
    const int s = (int)(i - q * ns);
    int x, y;
    if (!dtd::slot_pixel(P, q, x, y)) continue;
    c.rng.pixel = (uint32_t)(y * P.xRes + x);
    c.rng.sample = (uint32_t)(sample_begin + s);
    V3 eye_sample, ray0;
    camera_ray(c, P, x, y, eye_sample, ray0);
    start[3 * i] = eye_sample.x; start[3 * i + 1] = eye_sample.y; start[3 * i + 2] = eye_sample.z;
    dir[3 * i] = ray0.x; dir[3 * i + 1] = ray0.y; dir[3 * i + 2] = ray0.z;
  }
}
extern "C" hipError_t dt_launch_camera_rays(const void* dev_launch, int sample_begin, int ns, int64_t n_rows,
                                            double* start, double* dir, hipStream_t stream)
{
  int64_t blocks = (n_rows + 255) / 256;
  if (blocks > (1 << 22)) blocks = 1 << 22;   // grid-stride past that
  hipLaunchKernelGGL(dt_camera_rays_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const DLaunch*)dev_launch,
                     sample_begin, ns, n_rows, start, dir);
  return hipGetLastError();
}
