// dt_hitlist.h — the multi-hit walk and its register list (dt_rayq_multi.hip only).
#pragma once
#include "dt_device.h"

// Multi-hit walks (dt_rayq_multi_kernel, include/dt.h dt_trace_rays_multi): a lane's K nearest hits, sorted by
// the key (t, shape) ascending; an empty slot holds (FLT_MAX, INT_MAX), which every hit's key (t < FLT_MAX)
// precedes, so the number of hits is the number of slots with t < FLT_MAX and no count is carried. The
// list must stay in registers: every slot is named by a constant (the recursion over J below, no loop to
// unroll, no dynamic index that would send the array to scratch).
template <int K>
struct HitList {
  float t[K];
  int s[K];
};

template <int K>
__device__ __forceinline__ void hitlist_clear(HitList<K>& L)
{
#pragma unroll
  for (int j = 0; j < K; ++j) {
    L.t[j] = FLT_MAX;
    L.s[j] = 0x7fffffff;
  }
}

__device__ __forceinline__ bool hitkey_less(float t, int s, float t1, int s1)
{
  return t < t1 || (t == t1 && s < s1);
}

// Slots J .. 0 of a compare-and-shift insertion, from the back: slot J takes slot J-1 where the key precedes
// that one too (read before the step below overwrites it), the key where it precedes slot J only. `here`: on,
// and the key precedes slot J. One key compare per slot.
template <int K, int J>
__device__ __forceinline__ void hitlist_step(HitList<K>& L, bool on, float t, int s, bool here)
{
  if constexpr (J > 0) {
    const bool prev = on && hitkey_less(t, s, L.t[J - 1], L.s[J - 1]);
    L.t[J] = prev ? L.t[J - 1] : here ? t : L.t[J];
    L.s[J] = prev ? L.s[J - 1] : here ? s : L.s[J];
    hitlist_step<K, J - 1>(L, on, t, s, prev);
  } else {
    L.t[0] = here ? t : L.t[0];
    L.s[0] = here ? s : L.s[0];
  }
}

template <int K>
__device__ __forceinline__ void hitlist_insert(HitList<K>& L, bool on, float t, int s)
{
  hitlist_step<K, K - 1>(L, on, t, s, on && hitkey_less(t, s, L.t[K - 1], L.s[K - 1]));
}

// The first entry, and the rest moved up by one (the attribute loop of dt_rayq_multi_kernel takes the hits
// one by one through slot 0, so its runtime trip count indexes nothing)
template <int K>
__device__ __forceinline__ void hitlist_pop(HitList<K>& L, float& t, int& s)
{
  t = L.t[0];
  s = L.s[0];
#pragma unroll
  for (int j = 0; j + 1 < K; ++j) {
    L.t[j] = L.t[j + 1];
    L.s[j] = L.s[j + 1];
  }
  L.t[K - 1] = FLT_MAX;
  L.s[K - 1] = 0x7fffffff;
}

// closest_hit_walk's structure at shift 0 (MODE 0: finite rays on the fast tree; 1: the reference tree, exact
// for any wave), with every gathered shape tested on its own (t enters as FLT_MAX, nothing carried) and kept
// in the lane's list; a hit is a true return with t < FLT_MAX (false for NaN and for the edge-on
// checkerboard return, which leaves t alone). The list is a function of the set of gathered shapes only (a
// total order on (t, shape), every shape in one leaf), so neither tree nor visiting order shows in it, and
// the edge-on re-walk of closest_hit has no counterpart here.
// Culling: closest_hit_walk's bound, from the K-th distance once the list is full (tcull = FLT_MAX before).
// A hit that could still enter the list has t <= t_K, at a point of its shape, hence inside the leaf's box:
// the box's entry parameter is <= t up to the rounding of the two float computations, which the bound's
// relative 1e-4 and absolute 1e-4 cover as they do for closest_hit_walk's t_min, so the leaf passes
// tmin <= tcull, equal t included. t_K only shrinks, so with the monotone finite-ray slab test a lane that
// failed an ancestor fails below it too (no resume point, as in closest_hit_walk). MODE 1 does not cull
// (node_hit<true> reads no tcull).
template <int MODE, int K>
__device__ __forceinline__ void multi_hit_walk(const DScene& S, const DParams& P, const Walk& w, bool active, V3 ray,
                                               V3 org, HitList<K>& L)
{
  static_assert(MODE == 0 || MODE == 1, "the shift is 0: never the bump tree");
  constexpr bool GENERAL = MODE == 1;
  const bool ftree = !GENERAL && P.n_fnodes > 0 && (P.ftree_mode & 1);
  const DNodeDev* const NODES = ftree ? S.fnodes : S.nodes;
  const int n_nodes = ftree ? P.n_fnodes : P.n_nodes;
  int resume = active ? 0 : 0x7fffffff;
  const unsigned long long am = __ballot(active);
  int i = 0;
  while (i < n_nodes) {
    const DNodeDev nd = cas(NODES)[i];
    const bool act = GENERAL ? resume <= i : inv(am);
    const float tk = L.t[K - 1];
    const float tcull = tk == FLT_MAX ? FLT_MAX : tk * 1.0001f + 1e-4f;
    const unsigned long long hbm = node_mask<GENERAL>(w, nd, 0.0f, org, tcull, am, act);
    const bool hb = inv(hbm);
    if (nd.meta & DN_LEAF) {
      if (hbm) {
        const int nq = (nd.meta & DN_SINGLE) ? 1 : nd.aux;
        for (int q = 0; q < nq; ++q) {
          int sid, type, off;
          uint32_t flags;
          leaf_shape(S, nd, q, sid, type, flags, off);
          if (inv(hbm)) {
            float t = FLT_MAX;
            int ins = 0, cc = -1, edge = 0;
            const bool ret = shape_hit(S, sid, type, flags, cas(S.geom) + off, ray, org, 0.0f, t, ins, cc, edge);
            hitlist_insert(L, ret && t < FLT_MAX, t, sid);
          }
        }
      }
      if (GENERAL && act) resume = nd.skip;
      i = i + 1;
    } else {
      if (GENERAL && act && !hb) resume = nd.skip;
      i = hbm ? i + 1 : nd.skip;
    }
  }
}
