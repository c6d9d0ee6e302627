// dt_repro.hip — the reproducer of the called-function defect (tools/call_repro, tests/test_codegen.py;
// DESIGN.md §8). Never part of libdt.so.
#include "dt_kernel_iface.h"
#include "dt_device.h"

// The sky of dt_sky_miss_kernel (cpp:1074-1092,
// cloudColor of mcam * focalPoint per pixel) through cloud_color_lane inlined and through the same
// function behind a real call, on the same pixels, for the called-function defect
__device__ __noinline__ V3 cloud_color_lane_call(const DParams& P, const float* __restrict__ zs, V3 ray)
{
  return cloud_color_lane(P, zs, ray);
}
template <bool CALL>
__device__ __forceinline__ void repro_sky(const DParams* __restrict__ Pp, const float* __restrict__ zs, int x0, int y0,
                                          int w, int n, double* __restrict__ out)
{
  const DParams& P = *Pp;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) {
    const int x = x0 + q % w, y = y0 + q / w;
    const V3 eye = v3a(P.eye), X = v3a(P.X), Y = v3a(P.Y), Z = v3a(P.Z);
    float aa = P.l + (P.r - P.l) * (float)x / (float)P.xRes;
    float bb = P.b + (P.t - P.b) * (float)y / (float)P.yRes;
    V3 rd = sub(add(mul(aa, X), mul(bb, Y)), mul(P.near_plane, Z));
    V3 fp = add(eye, mul(P.focal_length, rd));
    V3 pt;
    pt.x = ((P.sky_m[0][0] * fp.x + P.sky_m[0][1] * fp.y) + P.sky_m[0][2] * fp.z) + P.sky_m[0][3] * 1.0;
    pt.y = ((P.sky_m[1][0] * fp.x + P.sky_m[1][1] * fp.y) + P.sky_m[1][2] * fp.z) + P.sky_m[1][3] * 1.0;
    pt.z = ((P.sky_m[2][0] * fp.x + P.sky_m[2][1] * fp.y) + P.sky_m[2][2] * fp.z) + P.sky_m[2][3] * 1.0;
    const V3 c = CALL ? cloud_color_lane_call(P, zs, pt) : cloud_color_lane(P, zs, pt);
    out[3 * q] = c.x;
    out[3 * q + 1] = c.y;
    out[3 * q + 2] = c.z;
  }
}
extern "C" __global__ void __launch_bounds__(256) dt_repro_inline(const DParams* Pp, const float* zs, int x0, int y0,
                                                                  int w, int n, double* out)
{
  repro_sky<false>(Pp, zs, x0, y0, w, n, out);
}
extern "C" __global__ void __launch_bounds__(256) dt_repro_call(const DParams* Pp, const float* zs, int x0, int y0,
                                                                int w, int n, double* out)
{
  repro_sky<true>(Pp, zs, x0, y0, w, n, out);
}
extern "C" hipError_t dt_repro_launch(int call, const void* Pp, const float* zs, int x0, int y0, int w, int n,
                                      double* out)
{
  if (call)
    hipLaunchKernelGGL(dt_repro_call, dim3((n + 255) / 256), dim3(256), 0, 0, (const DParams*)Pp, zs, x0, y0, w, n, out);
  else
    hipLaunchKernelGGL(dt_repro_inline, dim3((n + 255) / 256), dim3(256), 0, 0, (const DParams*)Pp, zs, x0, y0, w, n, out);
  return hipGetLastError();
}
