// dt_points_vis.hip — the mutual visibility of two point sets of dt_points_visibility.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_aux_wave.h"
#include "dt_irr.h"

// Mutual visibility of two point sets (include/dt.h dt_points_visibility; no reference counterpart): every pair
// (source i, target j) answered as dt_rayq_occl_kernel answers the ray (a_i, b_j - a_i, skip_b[j]), with the
// segment built in registers as dt_points_occl_kernel builds a probe: make_walk + occluded_walk<0/1>, tree walks
// only, one call site.
// A work item is (a wave of 64 consecutive sources) x (a tile of DT_PVIS_TILE consecutive targets), item =
// wave * n_tiles + tile, grid-stride over the items: few sources against many targets still fill the machine. One
// source per lane, loaded once per item; the target, its normal and its skip shape are wave-uniform loads (the
// skip through uni(), as dt_points_occl_kernel takes a light's shape), so the 64 lanes of a walk aim at one
// point and skip one shape: one walk per target, never one per lane. A void target runs no walk for the wave;
// a tail lane, a void source or a void segment is an inactive lane of its walks and stays in the wave.
// bits: a lane ORs 32 verdicts into a register and stores one word per 32 targets (at the word's end or at the
// tile's; tiles are multiples of 32, so no word is shared between items). count_a: one integer atomicAdd per
// lane and item; count_b: the ballot's popcount added by one lane, as ST_SHADOW is counted; the host zeroed
// both, and integers show no order. weight_a: the lane's f64 sum over the tile in ascending j goes to
// partial[tile * n_a + i]; dt_points_vis_sum_kernel then adds the tiles in ascending order (the header's fixed
// order). The cosines run only with `partial` (out->weight_a); every store is guarded by its plane's pointer.
static_assert(DT_PVIS_TILE % 32 == 0 && DT_PVIS_TILE > 0, "a bits word must not straddle two tiles");
extern "C" __global__ void __launch_bounds__(64)
dt_points_vis_kernel(const DLaunch* __restrict__ Lp, int64_t n_a, const double* __restrict__ a, int64_t n_b,
                     const double* __restrict__ b, const int32_t* __restrict__ skip_b,
                     const double* __restrict__ normal_a, const double* __restrict__ normal_b, int falloff,
                     uint32_t* __restrict__ bits, int32_t* __restrict__ count_a, int32_t* __restrict__ count_b,
                     double* __restrict__ partial)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  Counters cnt = aux_counters(wc_lds, lane);
  const int64_t n_tiles = (n_b + DT_PVIS_TILE - 1) / DT_PVIS_TILE, n_waves = (n_a + DT_WAVE - 1) / DT_WAVE;
  const int64_t words = (n_b + 31) / 32;   // per row of bits
  unsigned long long traced = 0;   // wave-uniform
  for (int64_t item = blockIdx.x; item < n_waves * n_tiles; item += gridDim.x) {
    const int64_t wave = item / n_tiles, tile = item - wave * n_tiles;
    const int64_t i = wave * DT_WAVE + lane;
    const bool in = i < n_a;
    V3 p = v3(0, 0, 0), na = v3(0, 0, 0);
    bool live = false;
    if (in) {
      const V3 pi = v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]);
      live = isfinite(pi.x) && isfinite(pi.y) && isfinite(pi.z);
      if (partial) {
        const V3 ni = v3(normal_a[3 * i], normal_a[3 * i + 1], normal_a[3 * i + 2]);
        live = live && isfinite(ni.x) && isfinite(ni.y) && isfinite(ni.z);
        if (live) na = ni;
      }
      if (live) p = pi;
    }
    const bool any_live = __ballot(live) != 0;   // wave-uniform: a wave of void sources runs no walk
    const int64_t j0 = tile * DT_PVIS_TILE, j1 = j0 + DT_PVIS_TILE < n_b ? j0 + DT_PVIS_TILE : n_b;
    uint32_t word = 0;
    int seen = 0;        // the lane's visible targets of this tile
    double wsum = 0.0;   // ... and their weights, ascending j
    for (int64_t j = j0; j < j1; ++j) {
      // the target: wave-uniform
      const V3 q = v3(b[3 * j], b[3 * j + 1], b[3 * j + 2]);
      bool live_b = any_live && isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
      V3 nb = v3(0, 0, 0);
      if (partial && live_b) {
        nb = v3(normal_b[3 * j], normal_b[3 * j + 1], normal_b[3 * j + 2]);
        live_b = isfinite(nb.x) && isfinite(nb.y) && isfinite(nb.z);
      }
      bool visible = false;
      if (live_b) {
        const int skip = skip_b ? uni(skip_b[j]) : -1;
        V3 sray = live ? sub(q, p) : v3(0, 0, 0);
        // a void segment (dt_rays_occluded's rule) is an inactive lane, as in dt_rayq_occl_kernel
        const bool act = live && !dtd::irr_void_dir(sray);
        if (!act) sray = v3(0, 0, 0);
        const V3 org = act ? p : v3(0, 0, 0);
        const float t_max = (float)norm(sray);
        const V3 sn = act ? normalized(sray) : v3(1, 0, 0);
        const V3 bstart = add(org, mul(1e-3, sray)), sstart = add(org, mul(1e-3, sn));
        const unsigned long long am = __ballot(act);
        traced += (unsigned long long)__popcll(am);
        bool occl = false;
        if (am) {
          const Walk w = make_walk(P, act, sray, bstart, 0.0f);
          const bool o = w.inf_wave ? occluded_walk<1>(S, P, w, act, bstart, sn, sstart, t_max, skip, 0.0f, cnt)
                                    : occluded_walk<0>(S, P, w, act, bstart, sn, sstart, t_max, skip, 0.0f, cnt);
          occl = act && o;
        }
        visible = live && !occl;
        if (partial) {
          double wij = 0.0;
          if (visible && act) {
            const double cc = dtd::irr_cosine(na, sray) * dtd::irr_cosine(nb, mul(-1, sray));
            wij = falloff ? cc / dot(sray, sray) : cc;
          }
          wsum = wsum + wij;
        }
        const unsigned long long vm = __ballot(visible);
        if (count_b && vm && lane == 0) atomicAdd(count_b + j, (int)__popcll(vm));
      }
      if (visible) {
        word |= 1u << (unsigned)(j & 31);
        ++seen;
      }
      if ((j & 31) == 31 || j + 1 == j1) {
        if (in && bits) bits[i * words + (j >> 5)] = word;
        word = 0;
      }
    }
    if (in && count_a && seen) atomicAdd(count_a + i, seen);
    if (in && partial) partial[tile * n_a + i] = wsum;
  }
  if (lane == 0 && traced) atomicAdd(S.stats + ST_SHADOW, traced);
}
// weight_a[i] = the f64 sum of source i's tile sums in ascending tile order, from 0.0; one lane per source
extern "C" __global__ void __launch_bounds__(256)
dt_points_vis_sum_kernel(int64_t n_a, int64_t n_tiles, const double* __restrict__ partial, double* __restrict__ weight_a)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_a) return;
  double s = 0.0;
  for (int64_t t = 0; t < n_tiles; ++t) s = s + partial[t * n_a + i];
  weight_a[i] = s;
}
extern "C" hipError_t dt_launch_points_vis(const void* dev_launch, int64_t n_a, const double* a, int64_t n_b,
                                           const double* b, const int32_t* skip_b, const double* normal_a,
                                           const double* normal_b, int falloff, uint32_t* bits, int32_t* count_a,
                                           int32_t* count_b, double* partial, double* weight_a, int grid,
                                           hipStream_t stream)
{
  hipLaunchKernelGGL(dt_points_vis_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n_a, a, n_b, b,
                     skip_b, normal_a, normal_b, falloff, bits, count_a, count_b, partial);
  if (hipError_t e = hipGetLastError()) return e;
  if (!weight_a) return hipSuccess;
  const int64_t n_tiles = (n_b + DT_PVIS_TILE - 1) / DT_PVIS_TILE;
  hipLaunchKernelGGL(dt_points_vis_sum_kernel, dim3((unsigned)((n_a + 255) / 256)), dim3(256), 0, stream, n_a, n_tiles,
                     partial, weight_a);
  return hipGetLastError();
}
extern "C" const void* dt_points_vis_kernel_ptr(void) { return (const void*)dt_points_vis_kernel; }
