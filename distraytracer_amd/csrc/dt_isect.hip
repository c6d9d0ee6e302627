// dt_isect.hip — the intersection micro-benchmark.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_aux_wave.h"

// Intersection micro-benchmark (2^24 primary rays of the C3 camera): rayColor's first
// step for the camera's primary rays (getDOFSamples + getPerspEyeRay, cpp:195-210 / 1044-1072; the
// BVH gather and closest hit, cpp:491-538), taken exactly as the trace kernel takes it for a root
// ray -- the pixel block's primary list when the wave's rays share a block, else the fast tree --
// one ray per lane. Ray r (pixel-major, DT_ISECT_RPP rays per pixel): q = r / RPP, pixel q mod W*H
// (raster order), sample r mod RPP + RPP * (q div W*H). Out: the hit shape (-1: none) and its t
// (FLT_MAX: none), as oracle/oracle.c or_primary_hit.
#define DT_ISECT_RPP 8
extern "C" __global__ void __launch_bounds__(64)
dt_isect_kernel(const DLaunch* __restrict__ Lp, int64_t first, int64_t n, int32_t* __restrict__ hit_shape,
                float* __restrict__ hit_t)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  Counters cnt = aux_counters(wc_lds, lane);
  Ctx c;
  c.S = &S;
  c.P = &P;
  c.rng.k0 = P.seed;
  c.rng.k1 = (uint32_t)P.frame;
  const int64_t npx = (int64_t)P.xRes * P.yRes;
  const bool lists = P.pl_block > 0 && P.n_fnodes > 0 && (P.ftree_mode & 1);
  for (int64_t base = (int64_t)blockIdx.x * DT_WAVE; base < n; base += (int64_t)gridDim.x * DT_WAVE) {
    const int64_t i = base + lane;
    const bool act = i < n;
    const int64_t r = first + i;
    const int64_t q = r / DT_ISECT_RPP;
    const int64_t p = q % npx;
    const int x = (int)(p % P.xRes), y = (int)(p / P.xRes);
    c.rng.pixel = (uint32_t)(y * P.xRes + x);
    c.rng.sample = (uint32_t)(r % DT_ISECT_RPP + DT_ISECT_RPP * (q / npx));
    V3 eye_sample = v3a(P.eye), ray0 = v3(0, 0, 0);
    if (act) camera_ray(c, P, x, y, eye_sample, ray0);
    int pblock = -1;
    if (lists) {
      const int blk = (y / P.pl_block) * P.pl_nbx + x / P.pl_block;
      const int b0 = uni(blk);
      if (!__ballot(act && blk != b0)) pblock = b0;
    }
    HitRec h;
    const bool any = closest_hit(S, P, act, ray0, eye_sample, 0.0f, h, cnt, pblock);
    if (act) {
      const bool hit = any && h.shape >= 0;
      hit_shape[i] = hit ? h.shape : -1;
      hit_t[i] = hit ? h.t_min : FLT_MAX;
    }
  }
  if (lane == 0) atomicAdd(S.stats + ST_WNODES, (unsigned long long)cnt.wnodes);
}
extern "C" hipError_t dt_launch_isect(const void* dev_launch, int64_t first, int64_t n, int32_t* hit_shape, float* hit_t,
                                      int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(dt_isect_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, first, n, hit_shape,
                     hit_t);
  return hipGetLastError();
}
extern "C" const void* dt_isect_kernel_ptr(void) { return (const void*)dt_isect_kernel; }
