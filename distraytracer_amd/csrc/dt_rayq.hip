// dt_rayq.hip — the ray queries of dt_trace_rays and dt_rays_occluded.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_rayq_load.h"
#include "dt_aux_wave.h"
#include "dt_hit_color.h"

// dt_trace_rays: rayColor's gather and closest hit (cpp:491-538) at shift 0, as dt_isect_kernel takes it
// without a primary list (pblock -1: the fast tree; the exact walk for a wave with an axis-parallel ray
// and after an edge-on checkerboard hit), and per hit what dt_features_kernel computes for one sample.
// Every plane is optional; the normal and the colour are computed only for the planes that take them, so
// the counters belong to the planes: prism_norm_fallback to `normal`, tex_fetches and uv_out_of_range
// to `albedo`.
extern "C" __global__ void __launch_bounds__(64)
dt_rayq_kernel(const DLaunch* __restrict__ Lp, int64_t n, const double* __restrict__ start,
               const double* __restrict__ dir, int32_t* __restrict__ shape_out, float* __restrict__ t_out,
               double* __restrict__ point, double* __restrict__ normal, double* __restrict__ albedo)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  Counters cnt = aux_counters(wc_lds, lane);
  unsigned long long traced = 0;   // wave-uniform
  for (int64_t base = (int64_t)blockIdx.x * DT_WAVE; base < n; base += (int64_t)gridDim.x * DT_WAVE) {
    const int64_t i = base + lane;
    const bool in = i < n;
    V3 org, ray;
    const bool act = rayq_load(start, dir, i, in, org, ray);
    const unsigned long long am = __ballot(act);
    traced += (unsigned long long)__popcll(am);
    HitRec h;
    h.t_min = FLT_MAX; h.shape = -1; h.ccol = -1;
    bool hit = false;
    if (am) {
      const bool any = closest_hit(S, P, act, ray, org, 0.0f, h, cnt, /*pblock*/ -1);
      hit = any && act && h.shape >= 0;
    }
    V3 p = v3(0, 0, 0), nrm = v3(0, 0, 0), col = v3(0, 0, 0);
    if (hit && (point || normal || albedo)) {
      const int sid = h.shape;
      const DShapeHdr hd = S.hdr[sid];
      GP g = cas(S.geom) + hd.off;
      const DMat& M = S.mat[sid];
      p = add(org, mul(h.t_min, ray));
      if (normal) {
        nrm = shape_norm(hd.type, hd.flags, g, p, 0.0f, cnt.wc + WC_PRISM, h.ccol);
        const V3 in_dir = normalized(ray);
        if (dot(mul(1e4, in_dir), nrm) >= 0) nrm = mul(-1, nrm);   // fixNorm
      }
      if (albedo) {
        col = hit_color(g, M, h.ccol);
        if (M.flags & DT_F_TEXTURE) {
          double tu = 0, tv = 0;
          const int uvt = shape_uv(hd.type, hd.flags, g, p, 0.0f, tu, tv);
          if (uvt == 2) {
            col = v3a(M.bordercolor);
          } else if (uvt == 1 && M.tex >= 0) {
            col = texel_color(S, M, tu, tv);
            atomicAdd(cnt.wc + WC_TEX, 1u);
          }
          if (uvt != 0 && (tu < 0 || tv < 0 || tu > 1 || tv > 1)) atomicAdd(cnt.wc + WC_UV, 1u);
        }
      }
    }
    if (in) {
      if (shape_out) shape_out[i] = hit ? h.shape : -1;
      if (t_out) t_out[i] = hit ? h.t_min : FLT_MAX;
      if (point) { point[3 * i] = p.x; point[3 * i + 1] = p.y; point[3 * i + 2] = p.z; }
      if (normal) { normal[3 * i] = nrm.x; normal[3 * i + 1] = nrm.y; normal[3 * i + 2] = nrm.z; }
      if (albedo) { albedo[3 * i] = col.x; albedo[3 * i + 1] = col.y; albedo[3 * i + 2] = col.z; }
    }
  }
  __syncthreads();
  const int st_of[WC_N] = {ST_RAYS, ST_SHADOW, ST_TEX, ST_STACK, ST_REFL, ST_GLOSSY, ST_UV, ST_PRISM, ST_SPHL};
  if (lane < WC_N) {
    const unsigned long long v = lane == WC_RAYS ? traced : wc_lds[lane];
    if (v) atomicAdd(S.stats + st_of[lane], v);
  }
}

// dt_rays_occluded: the light loop's shadow test (cpp:806-852) with sray = dir: the gather along dir from
// start + 1e-3 dir, intersectShadow along sn = normalized(dir) from start + 1e-3 sn up to t_max = |dir|, on
// every gathered shape but the lane's skip_shape. Tree walks only: the shadow grid's lists are per light
// and culled by the render's origin box. The walks skip one wave-uniform shape (the light's own, in the
// trace kernel), so the lanes of a wave are served in groups of equal skip_shape, one walk per group:
// one walk for a wave whose rays skip the same shape (or none), as many as it holds distinct values
// otherwise.
extern "C" __global__ void __launch_bounds__(64)
dt_rayq_occl_kernel(const DLaunch* __restrict__ Lp, int64_t n, const double* __restrict__ start,
                    const double* __restrict__ dir, const int32_t* __restrict__ skip_shape,
                    uint8_t* __restrict__ occluded)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  Counters cnt = aux_counters(wc_lds, lane);
  unsigned long long traced = 0;   // wave-uniform
  for (int64_t base = (int64_t)blockIdx.x * DT_WAVE; base < n; base += (int64_t)gridDim.x * DT_WAVE) {
    const int64_t i = base + lane;
    const bool in = i < n;
    V3 org, sray;
    const bool act = rayq_load(start, dir, i, in, org, sray);
    const int skip = (act && skip_shape) ? skip_shape[i] : -1;
    const float t_max = (float)norm(sray);
    const V3 sn = act ? normalized(sray) : v3(1, 0, 0);
    const V3 bstart = add(org, mul(1e-3, sray)), sstart = add(org, mul(1e-3, sn));
    bool occl = false;
    unsigned long long todo = __ballot(act);
    traced += (unsigned long long)__popcll(todo);
    while (todo) {
      const int k0 = __builtin_amdgcn_readlane(skip, (int)__builtin_ctzll(todo));
      const bool mine = inv(todo) && skip == k0;
      todo &= ~__ballot(mine);
      const Walk w = make_walk(P, mine, sray, bstart, 0.0f);
      const bool o = w.inf_wave ? occluded_walk<1>(S, P, w, mine, bstart, sn, sstart, t_max, k0, 0.0f, cnt)
                                : occluded_walk<0>(S, P, w, mine, bstart, sn, sstart, t_max, k0, 0.0f, cnt);
      occl = occl || (mine && o);
    }
    if (in) occluded[i] = occl ? 1 : 0;
  }
  if (lane == 0 && traced) atomicAdd(S.stats + ST_SHADOW, traced);
}

extern "C" hipError_t dt_launch_rayq(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                     int32_t* shape, float* t, double* point, double* normal, double* albedo, int grid,
                                     hipStream_t stream)
{
  hipLaunchKernelGGL(dt_rayq_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n, start, dir, shape, t,
                     point, normal, albedo);
  return hipGetLastError();
}
extern "C" hipError_t dt_launch_rayq_occl(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                          const int32_t* skip_shape, uint8_t* occluded, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(dt_rayq_occl_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n, start, dir,
                     skip_shape, occluded);
  return hipGetLastError();
}
extern "C" const void* dt_rayq_kernel_ptr(void) { return (const void*)dt_rayq_kernel; }
extern "C" const void* dt_rayq_occl_kernel_ptr(void) { return (const void*)dt_rayq_occl_kernel; }
