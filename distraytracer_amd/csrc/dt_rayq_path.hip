// dt_rayq_path.hip — the path ray query of dt_trace_rays_path.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_rayq_load.h"
#include "dt_aux_wave.h"
#include "dt_hit_color.h"
#include "dt_guide.h"

// dt_trace_rays_path: dt_features_path_kernel's chain per caller-supplied ray (include/dt.h): segment 0 is the
// caller's ray as dt_rayq_kernel loads it, every segment goes without a primary list (pblock -1) with the lanes
// still travelling as the mask, and the bounce loop is wave-uniform and capped by max_bounces: lanes whose path
// has ended wait for the others. A lane's path ends as DT_PATH_VOID until a traced segment says otherwise: a
// bounce leaves it so, and the void-ray test before the next segment decides.
// What a lane would have to carry to the end of the loop goes straight to memory instead: a segment's shape and
// point, the last ray and the terminal hit's point, normal and colour are stored where they are known (each lane
// its own row, vector stores), and the entries nobody wrote are filled after the loop. Only the ray, the length
// so far and three integers live across a walk.
extern "C" __global__ void __launch_bounds__(64)
dt_rayq_path_kernel(const DLaunch* __restrict__ Lp, int64_t n, const double* __restrict__ start,
                    const double* __restrict__ dir, int max_bounces, const dt_ray_paths O)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  Counters cnt = aux_counters(wc_lds, lane);
  const int per = max_bounces + 1;   // per-segment entries of a ray
  unsigned long long traced = 0;     // wave-uniform: the segments traced
  for (int64_t base = (int64_t)blockIdx.x * DT_WAVE; base < n; base += (int64_t)gridDim.x * DT_WAVE) {
    const int64_t i = base + lane;
    const bool in = i < n;
    V3 org, ray;
    bool live = rayq_load(start, dir, i, in, org, ray);   // the path is still travelling
    int end = DT_PATH_VOID, segs = 0, end_shape = -1;
    double len = 0;   // the path's length so far
    for (int k = 0; k <= max_bounces && __ballot(live); ++k) {
      if (k > 0) {
        // a void ray is not traced: its path stays DT_PATH_VOID
        live = live && isfinite(org.x) && isfinite(org.y) && isfinite(org.z) && isfinite(ray.x) &&
               isfinite(ray.y) && isfinite(ray.z) && (ray.x != 0 || ray.y != 0 || ray.z != 0);
        if (!live) { org = v3(0, 0, 0); ray = v3(0, 0, 0); }
      }
      const unsigned long long am = __ballot(live);
      if (!am) break;
      traced += (unsigned long long)__popcll(am);
      HitRec h;
      h.t_min = FLT_MAX; h.shape = -1; h.ccol = -1; h.inside = 0;
      const bool any = closest_hit(S, P, live, ray, org, 0.0f, h, cnt, /*pblock*/ -1);
      const bool hit = any && live && h.shape >= 0;
      if (live) {
        const int64_t e = (int64_t)per * i + k;
        segs = k + 1;
        if (!hit) end = DT_PATH_MISS;
        if (O.last_start) { O.last_start[3 * i] = org.x; O.last_start[3 * i + 1] = org.y; O.last_start[3 * i + 2] = org.z; }
        if (O.last_dir) { O.last_dir[3 * i] = ray.x; O.last_dir[3 * i + 1] = ray.y; O.last_dir[3 * i + 2] = ray.z; }
        if (O.seg_shape) O.seg_shape[e] = hit ? h.shape : -1;
        if (O.seg_point && !hit) { O.seg_point[3 * e] = 0; O.seg_point[3 * e + 1] = 0; O.seg_point[3 * e + 2] = 0; }
      }
      int goes_on = 0;   // the lane's path goes on with another segment (a miss ends it)
      if (hit) {
        const int sid = h.shape;
        const DShapeHdr hd = S.hdr[sid];
        GP g = cas(S.geom) + hd.off;
        const DMat& M = S.mat[sid];
        const V3 p = add(org, mul(h.t_min, ray));
        len = len + (double)h.t_min * norm(ray);
        if (O.seg_point) {
          const int64_t e = (int64_t)per * i + k;
          O.seg_point[3 * e] = p.x; O.seg_point[3 * e + 1] = p.y; O.seg_point[3 * e + 2] = p.z;
        }
        V3 nk = v3(0, 0, 0);
        int go = DT_GUIDE_STOP;
        V3 ndir = v3(0, 0, 0), nstart = v3(0, 0, 0);
        if (k < max_bounces || O.normal) {
          nk = shape_norm(hd.type, hd.flags, g, p, 0.0f, cnt.wc + WC_PRISM, h.ccol);
          const V3 in_dir = normalized(ray);
          if (dot(mul(1e4, in_dir), nk) >= 0) nk = mul(-1, nk);   // fixNorm
          if (k < max_bounces) {
            bool refl_err = false;
            go = guide_bounce(P.reflect, P.nogloss, P.refr_air, P.refr_glass, M.material, M.flags, h.inside, in_dir, nk,
                              p, ndir, nstart, refl_err);
            if (refl_err) atomicAdd(cnt.wc + WC_REFL, 1u);
          }
        }
        const bool goes = go != DT_GUIDE_STOP;
        goes_on = goes ? 1 : 0;
        if (goes) {
          ray = ndir;
          org = nstart;
          end = DT_PATH_VOID;   // until the next segment is traced
        }
        if (!goes) {
          end = k < max_bounces ? DT_PATH_SURFACE : DT_PATH_CUT;
          end_shape = sid;
          if (O.point) { O.point[3 * i] = p.x; O.point[3 * i + 1] = p.y; O.point[3 * i + 2] = p.z; }
          if (O.normal) { O.normal[3 * i] = nk.x; O.normal[3 * i + 1] = nk.y; O.normal[3 * i + 2] = nk.z; }
          if (O.albedo) {
            V3 col = hit_color(g, M, h.ccol);
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
            O.albedo[3 * i] = col.x; O.albedo[3 * i + 1] = col.y; O.albedo[3 * i + 2] = col.z;
          }
        }
      }
      // `live` must leave the hit's code as a per-lane VGPR value, not as a lane mask. The lanes that end run a
      // divergent region that holds the wave-uniform branch `if (O.albedo)`. With `live` assigned inside the
      // hit's code (in either arm, or before both), the mask of the lanes that go on reaches the join after that
      // branch on two edges: as ~(ending lanes) on the edge that skips the colour code, and as the constant 0 on
      // the edge through it (gfx950 ISA of this build: `s_xor_b64 m, exec, -1` before the branch, `s_mov_b64 m, 0`
      // after the colour code, `s_and_b64 live, m, exec` at the join). So with albedo wanted, one ending lane
      // stopped the whole wave after that segment. Supposed cause, not proven: the Makefile's
      // -structurizecfg-skip-uniform-regions leaves that uniform branch unstructurized inside a divergent region.
      // dt_features_path_kernel has no uniform branch there. The empty asm keeps the value opaque, so the mask is
      // formed from the VGPR here, after the region. tests/test_gpu_raypath.py case 2 (K >= 1, albedo wanted,
      // paths of mixed lengths in one wave) fails without it.
      asm volatile("" : "+v"(goes_on));
      live = goes_on != 0;
    }
    if (in) {
      if (O.end) O.end[i] = end;
      if (O.segments) O.segments[i] = segs;
      if (O.shape) O.shape[i] = end_shape;
      if (O.length) O.length[i] = len;
      if (end_shape < 0) {   // no terminal hit
        if (O.point) { O.point[3 * i] = 0; O.point[3 * i + 1] = 0; O.point[3 * i + 2] = 0; }
        if (O.normal) { O.normal[3 * i] = 0; O.normal[3 * i + 1] = 0; O.normal[3 * i + 2] = 0; }
        if (O.albedo) { O.albedo[3 * i] = 0; O.albedo[3 * i + 1] = 0; O.albedo[3 * i + 2] = 0; }
      }
      if (segs == 0) {
        if (O.last_start) { O.last_start[3 * i] = 0; O.last_start[3 * i + 1] = 0; O.last_start[3 * i + 2] = 0; }
        if (O.last_dir) { O.last_dir[3 * i] = 0; O.last_dir[3 * i + 1] = 0; O.last_dir[3 * i + 2] = 0; }
      }
      for (int k = segs; k < per; ++k) {   // the segments never traced
        const int64_t e = (int64_t)per * i + k;
        if (O.seg_shape) O.seg_shape[e] = -1;
        if (O.seg_point) { O.seg_point[3 * e] = 0; O.seg_point[3 * e + 1] = 0; O.seg_point[3 * e + 2] = 0; }
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

extern "C" hipError_t dt_launch_rayq_path(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                          int max_bounces, const struct dt_ray_paths* planes, int grid,
                                          hipStream_t stream)
{
  hipLaunchKernelGGL(dt_rayq_path_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n, start, dir,
                     max_bounces, *planes);
  return hipGetLastError();
}
extern "C" const void* dt_rayq_path_kernel_ptr(void) { return (const void*)dt_rayq_path_kernel; }
