// dt_rayq_transmit.hip — the transmittance ray query of dt_rays_transmittance.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_rayq_load.h"
#include "dt_panelist.h"

// dt_rays_transmittance: dt_rayq_occl_kernel's rays, groups of equal skip_shape and walks (make_walk, the
// inf_wave split), with transmit_walk in the place of occluded_walk: per ray -1 when a counting shape that is
// not glass blocks it, else the number of counting glass shapes, and the k smallest of their indices from a
// list of K >= k register slots per lane (K: 0, 1, 2, 4 or 8; the host launches the smallest that holds k). A
// lane belongs to one group, so its count and list are written by one walk only. Every element of every
// wanted plane is written: a void ray writes 0 and -1s, a blocked ray -1 and -1s. No workgroup waits on
// another.
template <int K>
__global__ void __launch_bounds__(64)
dt_rayq_transmit_kernel(const DLaunch* __restrict__ Lp, int64_t n, const double* __restrict__ start,
                        const double* __restrict__ dir, const int32_t* __restrict__ skip_shape, int k,
                        int32_t* __restrict__ panes_out, int32_t* __restrict__ pane_shape)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
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
    bool blocked = false;
    int panes = 0;
    PaneList<K> L;
    panelist_clear(L);
    unsigned long long todo = __ballot(act);
    traced += (unsigned long long)__popcll(todo);
    while (todo) {
      const int k0 = __builtin_amdgcn_readlane(skip, (int)__builtin_ctzll(todo));
      const bool mine = inv(todo) && skip == k0;
      todo &= ~__ballot(mine);
      const Walk w = make_walk(P, mine, sray, bstart, 0.0f);
      const bool b = w.inf_wave ? transmit_walk<1>(S, P, w, mine, bstart, sn, sstart, t_max, k0, panes, L)
                                : transmit_walk<0>(S, P, w, mine, bstart, sn, sstart, t_max, k0, panes, L);
      blocked = blocked || (mine && b);
    }
    if (in && panes_out) panes_out[i] = blocked ? -1 : panes;
    if constexpr (K > 0) {
      if (pane_shape) {
        for (int j = 0; j < k; ++j) {   // through slot 0: the runtime trip count indexes nothing
          const int sj = panelist_pop(L);
          if (in) pane_shape[(int64_t)k * i + j] = (!blocked && sj != 0x7fffffff) ? sj : -1;
        }
      }
    }
  }
  if (lane == 0 && traced) atomicAdd(S.stats + ST_SHADOW, traced);
}

// the list capacity a launch with k takes: the smallest of 0, 1, 2, 4, 8 that holds it
static int rayq_transmit_capacity(int k) { return k <= 0 ? 0 : k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

extern "C" hipError_t dt_launch_rayq_transmit(const void* dev_launch, int64_t n, const double* start, const double* dir,
                                              const int32_t* skip_shape, int k, int32_t* panes, int32_t* pane_shape,
                                              int grid, hipStream_t stream)
{
#define RAYQ_TRANSMIT_LAUNCH(K)                                                                                       \
  hipLaunchKernelGGL(dt_rayq_transmit_kernel<K>, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n,    \
                     start, dir, skip_shape, k, panes, pane_shape)
  switch (rayq_transmit_capacity(pane_shape ? k : 0)) {
    case 0: RAYQ_TRANSMIT_LAUNCH(0); break;
    case 1: RAYQ_TRANSMIT_LAUNCH(1); break;
    case 2: RAYQ_TRANSMIT_LAUNCH(2); break;
    case 4: RAYQ_TRANSMIT_LAUNCH(4); break;
    default: RAYQ_TRANSMIT_LAUNCH(8); break;
  }
#undef RAYQ_TRANSMIT_LAUNCH
  return hipGetLastError();
}
extern "C" const void* dt_rayq_transmit_kernel_ptr(int k)
{
  switch (rayq_transmit_capacity(k)) {
    case 0: return (const void*)dt_rayq_transmit_kernel<0>;
    case 1: return (const void*)dt_rayq_transmit_kernel<1>;
    case 2: return (const void*)dt_rayq_transmit_kernel<2>;
    case 4: return (const void*)dt_rayq_transmit_kernel<4>;
    default: return (const void*)dt_rayq_transmit_kernel<8>;
  }
}
