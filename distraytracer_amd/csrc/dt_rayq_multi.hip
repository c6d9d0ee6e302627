// dt_rayq_multi.hip — the multi-hit ray query of dt_trace_rays_multi.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_rayq_load.h"
#include "dt_hit_color.h"
#include "dt_hitlist.h"

// dt_trace_rays_multi: per ray the k nearest of the shapes dt_trace_rays gathers, each tested on its own
// (multi_hit_walk: the fast tree for finite waves, the reference tree for a wave with an axis-parallel ray),
// in a list of K >= k register slots per lane (K: 1, 2, 4 or 8; the host launches the smallest that holds k),
// of which the first k are written. Then per rank j < k, at wave-uniform control flow, what dt_rayq_kernel
// computes for its one hit, for the lanes with j < count; the other lanes write -1, FLT_MAX and zeros, so
// every element of every wanted plane is written. The walk carries no checker colour per slot (8 more live
// registers at K = 8): where albedo is wanted, a recorded checkerboard is tested once more (t reset) for
// its square.
template <int K>
__global__ void __launch_bounds__(64)
dt_rayq_multi_kernel(const DLaunch* __restrict__ Lp, int64_t n, const double* __restrict__ start,
                     const double* __restrict__ dir, int k, int32_t* __restrict__ count_out,
                     int32_t* __restrict__ shape_out, float* __restrict__ t_out, double* __restrict__ point,
                     double* __restrict__ normal, double* __restrict__ albedo)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  if (lane < WC_N) wc_lds[lane] = 0;
  __syncthreads();
  unsigned int* const wc = wc_lds;
  unsigned long long traced = 0;   // wave-uniform
  for (int64_t base = (int64_t)blockIdx.x * DT_WAVE; base < n; base += (int64_t)gridDim.x * DT_WAVE) {
    const int64_t i = base + lane;
    const bool in = i < n;
    V3 org, ray;
    const bool act = rayq_load(start, dir, i, in, org, ray);
    const unsigned long long am = __ballot(act);
    traced += (unsigned long long)__popcll(am);
    HitList<K> L;
    hitlist_clear(L);
    if (am) {
      const Walk w = make_walk(P, act, ray, org, 0.0f);
      if (w.inf_wave) multi_hit_walk<1>(S, P, w, act, ray, org, L);
      else multi_hit_walk<0>(S, P, w, act, ray, org, L);
    }
    if (in && count_out) {
      int c = 0;
#pragma unroll
      for (int j = 0; j < K; ++j) c += L.t[j] < FLT_MAX ? 1 : 0;
      count_out[i] = c < k ? c : k;
    }
    for (int j = 0; j < k; ++j) {
      float tj;
      int sj;
      hitlist_pop(L, tj, sj);
      const bool hit = act && tj < FLT_MAX;   // j < count
      V3 p = v3(0, 0, 0), nrm = v3(0, 0, 0), col = v3(0, 0, 0);
      if (hit && (point || normal || albedo)) {
        const DShapeHdr hd = S.hdr[sj];
        GP g = cas(S.geom) + hd.off;
        const DMat& M = S.mat[sj];
        p = add(org, mul(tj, ray));
        int ccol = -1;
        if (albedo && (hd.type == DT_SHAPE_CHECKERBOARD || hd.type == DT_SHAPE_CHECKERBOARD_HOLE)) {
          float t2 = FLT_MAX;
          int ins = 0, edge = 0;
          shape_hit(S, sj, hd.type, hd.flags, g, ray, org, 0.0f, t2, ins, ccol, edge);
        }
        if (normal) {
          nrm = shape_norm(hd.type, hd.flags, g, p, 0.0f, wc + WC_PRISM, ccol);
          const V3 in_dir = normalized(ray);
          if (dot(mul(1e4, in_dir), nrm) >= 0) nrm = mul(-1, nrm);   // fixNorm
        }
        if (albedo) {
          col = hit_color(g, M, ccol);
          if (M.flags & DT_F_TEXTURE) {
            double tu = 0, tv = 0;
            const int uvt = shape_uv(hd.type, hd.flags, g, p, 0.0f, tu, tv);
            if (uvt == 2) {
              col = v3a(M.bordercolor);
            } else if (uvt == 1 && M.tex >= 0) {
              col = texel_color(S, M, tu, tv);
              atomicAdd(wc + WC_TEX, 1u);
            }
            if (uvt != 0 && (tu < 0 || tv < 0 || tu > 1 || tv > 1)) atomicAdd(wc + WC_UV, 1u);
          }
        }
      }
      if (in) {
        const int64_t e = (int64_t)k * i + j;
        if (shape_out) shape_out[e] = hit ? sj : -1;
        if (t_out) t_out[e] = hit ? tj : FLT_MAX;
        if (point) { point[3 * e] = p.x; point[3 * e + 1] = p.y; point[3 * e + 2] = p.z; }
        if (normal) { normal[3 * e] = nrm.x; normal[3 * e + 1] = nrm.y; normal[3 * e + 2] = nrm.z; }
        if (albedo) { albedo[3 * e] = col.x; albedo[3 * e + 1] = col.y; albedo[3 * e + 2] = col.z; }
      }
    }
  }
  __syncthreads();
  const int st_of[WC_N] = {ST_RAYS, ST_SHADOW, ST_TEX, ST_STACK, ST_REFL, ST_GLOSSY, ST_UV, ST_PRISM, ST_SPHL};
  if (lane < WC_N) {
    const unsigned long long v = lane == WC_RAYS ? traced : wc_lds[lane];
    if (v) atomicAdd(S.stats + st_of[lane], v);
  }
}

// the list capacity a launch with k takes: the smallest of 1, 2, 4, 8 that holds it
static int rayq_multi_capacity(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

extern "C" hipError_t dt_launch_rayq_multi(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                           int k, int32_t* count, int32_t* shape, float* t, double* point,
                                           double* normal, double* albedo, int grid, hipStream_t stream)
{
#define RAYQ_MULTI_LAUNCH(K)                                                                                            \
  hipLaunchKernelGGL(dt_rayq_multi_kernel<K>, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n, start, \
                     dir, k, count, shape, t, point, normal, albedo)
  switch (rayq_multi_capacity(k)) {
    case 1: RAYQ_MULTI_LAUNCH(1); break;
    case 2: RAYQ_MULTI_LAUNCH(2); break;
    case 4: RAYQ_MULTI_LAUNCH(4); break;
    default: RAYQ_MULTI_LAUNCH(8); break;
  }
#undef RAYQ_MULTI_LAUNCH
  return hipGetLastError();
}
extern "C" const void* dt_rayq_multi_kernel_ptr(int k)
{
  switch (rayq_multi_capacity(k)) {
    case 1: return (const void*)dt_rayq_multi_kernel<1>;
    case 2: return (const void*)dt_rayq_multi_kernel<2>;
    case 4: return (const void*)dt_rayq_multi_kernel<4>;
    default: return (const void*)dt_rayq_multi_kernel<8>;
  }
}
