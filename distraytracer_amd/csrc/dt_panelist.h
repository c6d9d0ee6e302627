// dt_panelist.h — the transmittance walk and its pane list (dt_rayq_transmit.hip, dt_points_occl.hip's glass build).
#pragma once
#include "dt_device.h"

// Transmittance walks (dt_rayq_transmit_kernel, dt_points_occl_glass_kernel; include/dt.h
// dt_rays_transmittance): the any-hit walk with a filter. A shape counts for a lane as it occludes it in
// occluded_walk (not the skip shape, shape_shadow true); a counting shape that is not glass blocks the lane,
// which retires as an occluded lane does there; a counting glass shape adds one to the lane's `panes` and, for
// K >= 1, its index to the lane's list, and the lane walks on. The wave leaves the walk when every active lane
// is blocked or the tree is exhausted.
// Counting precondition: a plain count is right because every shape sits in exactly one leaf of either tree.
// The reference tree's leaves are disjoint slices of the index list (host_bvh.cpp generate: each node hands
// [0, slice) and [slice, n) to its two children), and the fast tree keeps each of those leaves exactly once
// under new inner nodes (host_fasttree.cpp build_fast_tree: one LeafRef per reference leaf, none split or
// copied). A lane reaches a leaf at most once in a walk (i only grows), so it tests a shape at most once, and
// finite waves take the fast tree as occluded_walk<0> does; nothing here falls back to the reference tree.
// The box cull is occluded_walk's (shadow_tcull): a culled box holds no shape that can count, glass or not.
// The list holds the K smallest indices of the counting glass shapes, ascending; an empty slot holds INT_MAX.
// It must stay in registers: every slot is named by a constant, as in HitList (K = 0: no list at all).
template <int K>
struct PaneList {
  int s[K > 0 ? K : 1];
};

template <int K>
__device__ __forceinline__ void panelist_clear(PaneList<K>& L)
{
#pragma unroll
  for (int j = 0; j < (K > 0 ? K : 1); ++j) L.s[j] = 0x7fffffff;
}

// hitlist_step with the shape index alone as the key
template <int K, int J>
__device__ __forceinline__ void panelist_step(PaneList<K>& L, bool on, int s, bool here)
{
  if constexpr (J > 0) {
    const bool prev = on && s < L.s[J - 1];
    L.s[J] = prev ? L.s[J - 1] : here ? s : L.s[J];
    panelist_step<K, J - 1>(L, on, s, prev);
  } else {
    L.s[0] = here ? s : L.s[0];
  }
}

template <int K>
__device__ __forceinline__ void panelist_insert(PaneList<K>& L, bool on, int s)
{
  if constexpr (K > 0) panelist_step<K, K - 1>(L, on, s, on && s < L.s[K - 1]);
}

// the first entry, and the rest moved up by one (hitlist_pop)
template <int K>
__device__ __forceinline__ int panelist_pop(PaneList<K>& L)
{
  const int s = L.s[0];
#pragma unroll
  for (int j = 0; j + 1 < K; ++j) L.s[j] = L.s[j + 1];
  L.s[K > 0 ? K - 1 : 0] = 0x7fffffff;
  return s;
}

// shadow_leaf with the filter: bm collects the blocked lanes
template <int K>
__device__ __forceinline__ void transmit_leaf(const DScene& S, const DNodeDev& nd, unsigned long long hbm,
                                              unsigned long long& bm, int& panes, PaneList<K>& L, V3 sn, V3 sstart,
                                              float t_max, int skip_shape)
{
  const int nq = (nd.meta & DN_SINGLE) ? 1 : nd.aux;
  for (int q = 0; q < nq; ++q) {
    int sid, type, off;
    uint32_t flags;
    leaf_shape(S, nd, q, sid, type, flags, off);
    const unsigned long long tm = sid != skip_shape ? hbm & ~bm : 0ull;   // lanes that test this shape
    if (!tm) continue;
    bool o = false;
    if (inv(tm)) o = shape_shadow(type, flags, cas(S.geom) + off, sn, sstart, t_max, 0.0f);
    if (uni(cas(S.mat)[sid].material) == DT_MAT_GLASS) {   // wave-uniform
      panes += o ? 1 : 0;
      panelist_insert(L, o, sid);
    } else {
      bm |= __ballot(o);
    }
  }
}

// occluded_walk<0/1> at shift 0 with transmit_leaf: true for a blocked lane
template <int MODE, int K>
__device__ __forceinline__ bool transmit_walk(const DScene& S, const DParams& P, const Walk& w, bool active, V3 bstart,
                                              V3 sn, V3 sstart, float t_max, int skip_shape, int& panes,
                                              PaneList<K>& L)
{
  static_assert(MODE == 0 || MODE == 1, "the shift is 0: never the bump tree");
  constexpr bool GENERAL = MODE == 1;
  const bool ftree = !GENERAL && P.n_fnodes > 0 && (P.ftree_mode & 2);
  const DNodeDev* const NODES = ftree ? S.fnodes : S.nodes;
  const int n_nodes = ftree ? P.n_fnodes : P.n_nodes;
  int resume = active ? 0 : 0x7fffffff;
  const unsigned long long am = __ballot(active);
  unsigned long long bm = 0;   // blocked lanes
  const float tcull = shadow_tcull(t_max);
  int i = 0;
  while (i < n_nodes) {
    const DNodeDev nd = cas(NODES)[i];
    const bool act = GENERAL ? resume <= i : inv(am & ~bm);   // see closest_hit_walk
    const unsigned long long hbm = node_mask<GENERAL>(w, nd, 0.0f, bstart, tcull, am & ~bm, act);
    const bool hb = inv(hbm);
    if (nd.meta & DN_LEAF) {
      if (hbm) transmit_leaf(S, nd, hbm, bm, panes, L, sn, sstart, t_max, skip_shape);
      if (GENERAL) {
        if (act) resume = inv(bm) ? 0x7fffffff : nd.skip;
        if (!__ballot(resume != 0x7fffffff)) break;
      } else if (!(am & ~bm)) {
        break;
      }
      i = i + 1;
    } else {
      if (GENERAL && act && !hb) resume = nd.skip;
      i = hbm ? i + 1 : nd.skip;
    }
  }
  return inv(bm);
}
