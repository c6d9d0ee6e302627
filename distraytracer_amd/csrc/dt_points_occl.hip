// dt_points_occl.hip — the occlusion queries at surface points, plain and through glass.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_aux_wave.h"
#include "dt_occl.h"
// DT_GLASS_PROBES=1: the unit's second build (Makefile dt_kernels_pocclg): dt_points_occl_glass_kernel, whose
// probes pass through glass; the same source with the transmittance walk in the place of the any-hit walk
#ifndef DT_GLASS_PROBES
#define DT_GLASS_PROBES 0
#endif
#if DT_GLASS_PROBES
#include "dt_panelist.h"
#endif

// Occlusion queries at surface points (include/dt.h dt_points_occlusion; no reference counterpart): the probes
// of dt_occlusion_kernel from points and normals the caller hands over, 3 doubles each, in place of the
// camera's first hits. One point per lane, 64 consecutive points per wave, grid-stride over the waves as
// dt_rayq_occl_kernel; the lane's point is the RNG counter's pixel, its sample loop the counter's sample.
// Probes are generated in registers (dt_occl.h, the one definition) and answered as dt_rayq_occl_kernel
// answers a ray: make_walk + occluded_walk<0/1>, tree walks only, one call site.
// The loops are wave-uniform: row 0 is the AO plane (probe t = sample * ao_rays + r), row 1 + j light slot j
// (probe t = sample), whose skip shape is the light's own, one value for the wave: one walk per probe index,
// never one per lane. A lane counts its own unoccluded probes in a register and stores one float per row
// (integers: no summation order). A tail lane or a void point (a non-finite component) is an inactive lane
// of every walk: it stays in the wave, is never probed, and a void point stores 0.
//
// DT_GLASS_PROBES: the same source as dt_points_occl_glass_kernel (include/dt.h dt_points_occlusion_glass), a build
// of its own; the preprocessor leaves the plain build the tokens it had. There a probe is answered by
// transmit_walk<0/1, 0> (a count, no list): it is unoccluded iff it is not blocked and crosses at most
// max_panes panes; beside its unoccluded probes a lane sums their panes (integers again), for the two optional
// pane planes, and every store is guarded, as a row runs for either of its two planes.
extern "C" __global__ void __launch_bounds__(64)
#if DT_GLASS_PROBES
dt_points_occl_glass_kernel(const DLaunch* __restrict__ Lp, uint32_t seed, int32_t frame, int64_t n,
                            const double* __restrict__ point, const double* __restrict__ normal, int n_samples,
                            int ao_rays, float ao_radius, int n_lights, const dtd::OcclLight* __restrict__ lights,
                            int max_panes, float* __restrict__ ao_out, float* __restrict__ light_out,
                            float* __restrict__ ao_panes_out, float* __restrict__ light_panes_out)
#else
dt_points_occl_kernel(const DLaunch* __restrict__ Lp, uint32_t seed, int32_t frame, int64_t n,
                      const double* __restrict__ point, const double* __restrict__ normal, int n_samples, int ao_rays,
                      float ao_radius, int n_lights, const dtd::OcclLight* __restrict__ lights,
                      float* __restrict__ ao_out, float* __restrict__ light_out)
#endif
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
    for (int row = ao_rays > 0 ? 0 : 1; row <= n_lights; ++row) {
      const int per = row == 0 ? ao_rays : 1;
      const int n_probes = any_live ? n_samples * per : 0;
      dtd::OcclLight L = {};
      int skip = -1;
      if (row > 0) {
        L = lights[row - 1];   // wave-uniform
        skip = uni(L.shape_index);
      }
      unsigned int V = 0;
#if DT_GLASS_PROBES
      unsigned int VP = 0;   // the panes of the unoccluded probes
#endif
      for (int t = 0; t < n_probes; ++t) {
        const int sample = t / per, r = t - sample * per;
        V3 sray = v3(0, 0, 0);
        if (live) {
          if (row == 0) sray = dtd::occl_ao_dir(seed, frame, pixel, (uint32_t)sample, r, ao_radius, nrm);
          else sray = dtd::occl_light_dir(seed, frame, pixel, (uint32_t)sample, row - 1, L, p);
        }
        // a void probe (dt_rays_occluded's rule) is an inactive lane, as in dt_rayq_occl_kernel
        const bool act = live && isfinite(sray.x) && isfinite(sray.y) && isfinite(sray.z) &&
                         (sray.x != 0 || sray.y != 0 || sray.z != 0);
        if (!act) sray = v3(0, 0, 0);
        const V3 org = act ? p : v3(0, 0, 0);
        const float t_max = (float)norm(sray);
        const V3 sn = act ? normalized(sray) : v3(1, 0, 0);
        const V3 bstart = add(org, mul(1e-3, sray)), sstart = add(org, mul(1e-3, sn));
        const unsigned long long am = __ballot(act);
        traced += (unsigned long long)__popcll(am);
        bool occl = false;
#if DT_GLASS_PROBES
        int panes = 0;
        if (am) {
          const Walk w = make_walk(P, act, sray, bstart, 0.0f);
          PaneList<0> none;
          const bool b = w.inf_wave ? transmit_walk<1>(S, P, w, act, bstart, sn, sstart, t_max, skip, panes, none)
                                    : transmit_walk<0>(S, P, w, act, bstart, sn, sstart, t_max, skip, panes, none);
          occl = act && (b || panes > max_panes);
        }
        if (live && !occl) {
          ++V;
          VP += (unsigned int)panes;
        }
#else
        if (am) {
          const Walk w = make_walk(P, act, sray, bstart, 0.0f);
          const bool o = w.inf_wave ? occluded_walk<1>(S, P, w, act, bstart, sn, sstart, t_max, skip, 0.0f, cnt)
                                    : occluded_walk<0>(S, P, w, act, bstart, sn, sstart, t_max, skip, 0.0f, cnt);
          occl = act && o;
        }
        if (live && !occl) ++V;
#endif
      }
#if DT_GLASS_PROBES
      if (in) {
        const double den = row == 0 ? (double)n_samples * (double)ao_rays : (double)n_samples;
        float* const vis = row == 0 ? ao_out : light_out;
        float* const pan = row == 0 ? ao_panes_out : light_panes_out;
        const int64_t e = row == 0 ? i : (int64_t)n_lights * i + (row - 1);
        if (vis) vis[e] = live ? (float)((double)V / den) : 0.0f;
        if (pan) pan[e] = live ? (float)((double)VP / den) : 0.0f;
      }
#else
      if (in) {
        if (row == 0) ao_out[i] = live ? (float)((double)V / ((double)n_samples * (double)ao_rays)) : 0.0f;
        else light_out[(int64_t)n_lights * i + (row - 1)] = live ? (float)((double)V / (double)n_samples) : 0.0f;
      }
#endif
    }
  }
  if (lane == 0 && traced) atomicAdd(S.stats + ST_SHADOW, traced);
}
#if DT_GLASS_PROBES
extern "C" hipError_t dt_launch_points_occl_glass(const void* dev_launch, uint32_t seed, int32_t frame, int64_t n,
                                                  const double* point, const double* normal, int n_samples,
                                                  int ao_rays, float ao_radius, int n_lights, const void* lights,
                                                  int max_panes, float* ao, float* light, float* ao_panes,
                                                  float* light_panes, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(dt_points_occl_glass_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, seed,
                     frame, n, point, normal, n_samples, ao_rays, ao_radius, n_lights, (const dtd::OcclLight*)lights,
                     max_panes, ao, light, ao_panes, light_panes);
  return hipGetLastError();
}
extern "C" const void* dt_points_occl_glass_kernel_ptr(void) { return (const void*)dt_points_occl_glass_kernel; }
#else
extern "C" hipError_t dt_launch_points_occl(const void* dev_launch, uint32_t seed, int32_t frame, int64_t n,
                                            const double* point, const double* normal, int n_samples, int ao_rays,
                                            float ao_radius, int n_lights, const void* lights, float* ao, float* light,
                                            int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(dt_points_occl_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, seed, frame, n,
                     point, normal, n_samples, ao_rays, ao_radius, n_lights, (const dtd::OcclLight*)lights, ao, light);
  return hipGetLastError();
}
extern "C" const void* dt_points_occl_kernel_ptr(void) { return (const void*)dt_points_occl_kernel; }
#endif
