// dt_rayq_load.h — the ray queries' common rules and the load of one caller-supplied ray (the dt_rayq*.hip units).
#pragma once
#include "dt_device.h"

// Ray queries (include/dt.h dt_trace_rays, dt_rays_occluded, dt_trace_rays_multi, dt_rays_transmittance, dt_trace_rays_path; no reference counterpart): rays the caller
// hands over in memory, 3 doubles of start and of direction each, one ray per lane, 64 consecutive rays
// per wave, grid-stride over the waves as dt_isect_kernel. The walks are the wave-uniform ones of the
// trace kernel (node and shape data through scalar loads, the lanes' decisions as masks), so a wave
// visits the union of its lanes' nodes: rays that lie together in memory should lie together in space.
//
// A void ray (a non-finite component, or an all-zero direction) is an inactive lane: it is never traced
// and does not reach make_walk's ballots, so it neither sends its wave down the exact walk nor changes
// a neighbour's answer.
__device__ __forceinline__ bool rayq_load(const double* __restrict__ start, const double* __restrict__ dir, int64_t i,
                                          bool in, V3& org, V3& ray)
{
  org = v3(0, 0, 0);
  ray = v3(0, 0, 0);
  if (!in) return false;
  const V3 o = v3(start[3 * i], start[3 * i + 1], start[3 * i + 2]);
  const V3 d = v3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
  const bool live = isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) &&
                    isfinite(d.z) && (d.x != 0 || d.y != 0 || d.z != 0);
  if (live) {
    org = o;
    ray = d;
  }
  return live;
}
