// dt_points_irr.hip — the irradiance queries at surface points of dt_points_irradiance.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_aux_wave.h"
#include "dt_hit_color.h"
#include "dt_irr.h"

// Irradiance queries at surface points (include/dt.h dt_points_irradiance; no reference counterpart):
// dt_points_occl_kernel's points, lanes and light probes, each unoccluded probe weighted by the cosine at the
// point (dt_irr.h irr_cosine) and the means combined with the lights' colours, which travel in the launch's
// light records (dt_irr.h IrrLight); then one diffuse gather bounce. Every loop is wave-uniform:
//   the direct rows: per light slot j and sample s one probe (dt_occl.h occl_light_dir, unchanged), answered by
//     make_walk + occluded_walk<0/1> as dt_rayq_occl_kernel answers a ray, the slot's skip shape for the wave;
//   the gather: per (s, r) one closest-hit walk for the wave's gather probes (dt_irr.h irr_gather_ray) with
//     the attributes as dt_rayq_kernel computes them (point, shape_norm + fixNorm, hit_color / texel), and from
//     the lanes' own hits one occluded_walk per light slot (irr_light_dir under OCCL_P_GLIGHT).
// A tail lane, a void point, a void probe, a lane that missed or hit an emitter is an inactive lane of the
// walks it has no part in and stays in the wave. A lane keeps its sums in registers (f64, in the header's
// order) and stores each plane entry once, every store guarded by the plane's pointer; rows and loops whose
// planes are all NULL run no walk: the direct rows for direct or direct_rgb, the gather for indirect_rgb or
// sky, its light loop and attributes for indirect_rgb.
extern "C" __global__ void __launch_bounds__(64)
dt_points_irr_kernel(const DLaunch* __restrict__ Lp, uint32_t seed, int32_t frame, int64_t n,
                     const double* __restrict__ point, const double* __restrict__ normal, int n_samples, int n_lights,
                     const dtd::IrrLight* __restrict__ lights, int gather_rays, float* __restrict__ direct_out,
                     float* __restrict__ direct_rgb_out, float* __restrict__ indirect_rgb_out,
                     float* __restrict__ sky_out)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  Counters cnt = aux_counters(wc_lds, lane);
  const int direct_rows = (direct_out || direct_rgb_out) ? n_lights : 0;
  const int gathers = (indirect_rgb_out || sky_out) ? gather_rays : 0;
  const int gather_lights = indirect_rgb_out ? n_lights : 0;
  unsigned long long shadowed = 0, gathered = 0;   // wave-uniform: the non-void shadow and gather probes
  for (int64_t base = (int64_t)blockIdx.x * DT_WAVE; base < n; base += (int64_t)gridDim.x * DT_WAVE) {
    const int64_t i = base + lane;
    const bool in = i < n;
    V3 p = v3(0, 0, 0), nrm = v3(0, 0, 0);
    bool live = false;
    if (in) {
      const V3 pi = v3(point[3 * i], point[3 * i + 1], point[3 * i + 2]);
      const V3 ni = v3(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
      live = isfinite(pi.x) && isfinite(pi.y) && isfinite(pi.z) && isfinite(ni.x) && isfinite(ni.y) && isfinite(ni.z);
      if (live) {
        p = pi;
        nrm = ni;
      }
    }
    const uint32_t pixel = (uint32_t)i;
    const bool any_live = __ballot(live) != 0;   // wave-uniform: a wave of void points runs no probe loop
    const double den = (double)n_samples;
    V3 D = v3(0, 0, 0);   // direct_rgb's sums over the slots
    for (int j = 0; j < direct_rows; ++j) {
      const dtd::IrrLight L = lights[j];   // wave-uniform
      const int skip = uni(L.L.shape_index);
      double C = 0.0;
      for (int s = 0; any_live && s < n_samples; ++s) {
        V3 sray = v3(0, 0, 0);
        if (live) sray = dtd::occl_light_dir(seed, frame, pixel, (uint32_t)s, j, L.L, p);
        // a void probe (dt_rays_occluded's rule) is an inactive lane, as in dt_rayq_occl_kernel
        const bool act = live && !dtd::irr_void_dir(sray);
        if (!act) sray = v3(0, 0, 0);
        const V3 org = act ? p : v3(0, 0, 0);
        const float t_max = (float)norm(sray);
        const V3 sn = act ? normalized(sray) : v3(1, 0, 0);
        const V3 bstart = add(org, mul(1e-3, sray)), sstart = add(org, mul(1e-3, sn));
        const unsigned long long am = __ballot(act);
        shadowed += (unsigned long long)__popcll(am);
        bool occl = false;
        if (am) {
          const Walk w = make_walk(P, act, sray, bstart, 0.0f);
          const bool o = w.inf_wave ? occluded_walk<1>(S, P, w, act, bstart, sn, sstart, t_max, skip, 0.0f, cnt)
                                    : occluded_walk<0>(S, P, w, act, bstart, sn, sstart, t_max, skip, 0.0f, cnt);
          occl = act && o;
        }
        C = C + (occl ? 0.0 : dtd::irr_cosine(nrm, sray));
      }
      const double mean = C / den;
      if (in && direct_out) direct_out[(int64_t)n_lights * i + j] = live ? (float)mean : 0.0f;
      D = add(D, mul(mean, v3a(L.color)));
    }
    if (in && direct_rgb_out) {
      direct_rgb_out[3 * i] = live ? (float)D.x : 0.0f;
      direct_rgb_out[3 * i + 1] = live ? (float)D.y : 0.0f;
      direct_rgb_out[3 * i + 2] = live ? (float)D.z : 0.0f;
    }
    if (gathers <= 0) continue;   // wave-uniform
    V3 G = v3(0, 0, 0);       // indirect_rgb's sums over (s, r)
    unsigned int missed = 0;  // the gather probes that hit nothing
    for (int t = 0; any_live && t < n_samples * gathers; ++t) {
      const int s = t / gathers, r = t - s * gathers;
      V3 gstart = v3(0, 0, 0), gdir = v3(0, 0, 0);
      bool gl = false;
      if (live) gl = dtd::irr_gather_ray(seed, frame, pixel, (uint32_t)s, r, p, nrm, gstart, gdir);
      if (!gl) {
        gstart = v3(0, 0, 0);
        gdir = v3(0, 0, 0);
      }
      const unsigned long long gm = __ballot(gl);
      gathered += (unsigned long long)__popcll(gm);
      HitRec h;
      h.t_min = FLT_MAX; h.shape = -1; h.ccol = -1;
      bool hit = false;
      if (gm) {
        const bool any = closest_hit(S, P, gl, gdir, gstart, 0.0f, h, cnt, /*pblock*/ -1);
        hit = any && gl && h.shape >= 0;
      }
      if (gl && !hit) ++missed;
      if (!indirect_rgb_out || !__ballot(hit)) continue;   // wave-uniform
      V3 q = v3(0, 0, 0), nq = v3(0, 0, 0), col = v3(0, 0, 0);
      bool shade = false;   // a hit that is no emitter: it runs the light loop
      if (hit) {
        const int sid = h.shape;
        const DShapeHdr hd = S.hdr[sid];
        GP g = cas(S.geom) + hd.off;
        const DMat& M = S.mat[sid];
        q = add(gstart, mul(h.t_min, gdir));
        col = hit_color(g, M, h.ccol);
        if (M.flags & DT_F_TEXTURE) {
          double tu = 0, tv = 0;
          const int uvt = shape_uv(hd.type, hd.flags, g, q, 0.0f, tu, tv);
          if (uvt == 2) col = v3a(M.bordercolor);
          else if (uvt == 1 && M.tex >= 0) col = texel_color(S, M, tu, tv);
        }
        if (M.flags & DT_F_LIGHT) {
          G = add(G, col);
        } else {
          shade = true;
          nq = shape_norm(hd.type, hd.flags, g, q, 0.0f, cnt.wc + WC_PRISM, h.ccol);
          const V3 in_dir = normalized(gdir);
          if (dot(mul(1e4, in_dir), nq) >= 0) nq = mul(-1, nq);   // fixNorm
        }
      }
      if (!__ballot(shade)) continue;   // wave-uniform
      V3 E = v3(0, 0, 0);
      for (int j = 0; j < gather_lights; ++j) {
        const dtd::IrrLight L = lights[j];   // wave-uniform
        const int skip = uni(L.L.shape_index);
        V3 sray = v3(0, 0, 0);
        if (shade)
          sray = dtd::irr_light_dir(seed, frame, pixel, (uint32_t)s, dtd::OCCL_P_GLIGHT, r * DT_OCCL_MAX_LIGHTS + j, L.L, q);
        const bool act = shade && !dtd::irr_void_dir(sray) && isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
        if (!act) sray = v3(0, 0, 0);
        const V3 org = act ? q : v3(0, 0, 0);
        const float t_max = (float)norm(sray);
        const V3 sn = act ? normalized(sray) : v3(1, 0, 0);
        const V3 bstart = add(org, mul(1e-3, sray)), sstart = add(org, mul(1e-3, sn));
        const unsigned long long am = __ballot(act);
        shadowed += (unsigned long long)__popcll(am);
        bool occl = false;
        if (am) {
          const Walk w = make_walk(P, act, sray, bstart, 0.0f);
          const bool o = w.inf_wave ? occluded_walk<1>(S, P, w, act, bstart, sn, sstart, t_max, skip, 0.0f, cnt)
                                    : occluded_walk<0>(S, P, w, act, bstart, sn, sstart, t_max, skip, 0.0f, cnt);
          occl = act && o;
        }
        E = add(E, mul(occl ? 0.0 : dtd::irr_cosine(nq, sray), v3a(L.color)));
      }
      if (shade) G = add(G, cwise(col, E));
    }
    if (in) {
      const double gden = den * (double)gather_rays;
      if (indirect_rgb_out) {
        indirect_rgb_out[3 * i] = live ? (float)(G.x / gden) : 0.0f;
        indirect_rgb_out[3 * i + 1] = live ? (float)(G.y / gden) : 0.0f;
        indirect_rgb_out[3 * i + 2] = live ? (float)(G.z / gden) : 0.0f;
      }
      if (sky_out) sky_out[i] = live ? (float)((double)missed / gden) : 0.0f;
    }
  }
  if (lane == 0) {
    if (shadowed) atomicAdd(S.stats + ST_SHADOW, shadowed);
    if (gathered) atomicAdd(S.stats + ST_RAYS, gathered);
  }
}
extern "C" hipError_t dt_launch_points_irr(const void* dev_launch, uint32_t seed, int32_t frame, int64_t n,
                                           const double* point, const double* normal, int n_samples, int n_lights,
                                           const void* lights, int gather_rays, float* direct, float* direct_rgb,
                                           float* indirect_rgb, float* sky, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(dt_points_irr_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, seed, frame, n,
                     point, normal, n_samples, n_lights, (const dtd::IrrLight*)lights, gather_rays, direct, direct_rgb,
                     indirect_rgb, sky);
  return hipGetLastError();
}
extern "C" const void* dt_points_irr_kernel_ptr(void) { return (const void*)dt_points_irr_kernel; }
