// host_launch.h — the host side of a render launch that needs no device: the grow-only device
// buffer and the launch policy (dt_api.cpp enqueue_render). No HIP include, so
// tests/launch_host_check.cpp exercises both with a counting allocator and no GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "dt_scene_dev.h"

namespace dth {

// A device buffer that only grows. Mem supplies `typedef ... Stream`, `int alloc(void**, size_t)`,
// `void free(void*)` and `int sync(Stream)` (0: success). A buffer that is too small is replaced,
// never extended: earlier launches on the stream may still use it, so the stream drains before the
// free; an empty buffer has no such launch and drains nothing. A failed allocation leaves
// (nullptr, 0), so that the next launch allocates again instead of trusting a stale capacity.
template <class Mem> struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;   // bytes
  template <class T> T* as() const { return (T*)p; }
  int reserve(size_t bytes, typename Mem::Stream st, bool* grew = nullptr)
  {
    if (bytes <= cap) return 0;
    if (p) {
      if (int e = Mem::sync(st)) return e;
      Mem::free(p);
    }
    p = nullptr;
    cap = 0;
    if (int e = Mem::alloc(&p, bytes)) {
      p = nullptr;
      return e;
    }
    cap = bytes;
    if (grew) *grew = true;
    return 0;
  }
  void release()
  {
    if (p) Mem::free(p);
    p = nullptr;
    cap = 0;
  }
};

// The launch policy: pure functions of the render's parameters, the grid and the environment, which
// is read on every call (the tests change it between renders).

// Chunk items (spp > 64: C4's 256): every 64-sample chunk of a pixel is a queue item of its own, so
// a pixel's chunks run on different waves and a long pixel no longer holds one wave for four
// chunks in turn. The chunks store their sample colours; dt_chunk_sum_kernel adds each pixel's up
// in sample order after the trace launch(es) (dt_kernels.hip). For a rank's share of a split frame
// (world > 1): C4's world-8 shares 44.0 against 48.6 ms for the slowest (profiles/r06c_rb_*). A
// whole frame keeps one item per pixel: there the stored colours and the sum kernel cost C4 1.5%
// (1710 against 1736 Mpixel-samples/s with the chunks of a pixel dequeued together, r06b).
// DT_CHUNK_ITEMS=0 / 1 / 2 (2: the queue chunk-major, the tests' check) overrides the default.
// traits, traits_sky: of the build and of the *_sky build that renders its sky items.
inline int launch_chunk_items(const dtd::DParams& P, int traits, int traits_sky, bool window)
{
  const char* ci_env = getenv("DT_CHUNK_ITEMS");
  int chunk_items = ci_env ? atoi(ci_env) : (P.world > 1 ? 1 : 0);
  // (the build and, for a sky-item launch, its *_sky build must carry the code: trait bit 1)
  if (!(traits & 2) || !(traits_sky & 2) || P.chunks < 2 || P.chunks > 255 || chunk_items < 0 ||
      chunk_items > 2 || (double)P.n_items * P.chunks >= 4294967296.0)
    chunk_items = 0;
  // a window launch runs per-pixel items whatever DT_CHUNK_ITEMS says: the window's chunks in turn
  // on one wave, the pixel's sums going on from the accumulator (dt_kernels.hip DT_WINDOW)
  if (window) chunk_items = 0;
  return chunk_items;
}

struct LaunchPolicy { int chunk_items, item_batch, queue_segs, prio_steps; };

// n_queue: the queue's items (n_items, times chunks with chunk items); grid: the waves launched
inline LaunchPolicy launch_policy(const dtd::DParams& P, int chunk_items, int64_t n_queue, int64_t grid)
{
  LaunchPolicy L;
  L.chunk_items = chunk_items;
  // two items per queue atomic pays when every wave takes many items (C3: ~500, +2%; C3's 1/8
  // tile share: 63, its kernel -3.3%, profiles/r03x); with few (C2: ~30) the coarser tail costs
  // more (-11%). DT_BATCH_ITEMS: the items per wave from which DT_BATCH_SIZE (2) are dequeued at once
  const char* bi = getenv("DT_BATCH_ITEMS");
  const char* bs = getenv("DT_BATCH_SIZE");
  const int64_t batch_from = bi && atoi(bi) > 0 ? atoi(bi) : 32;
  // Items of several 64-sample chunks (spp > 64: C4's 256) take one per atomic: their dequeues are
  // rare already, and two consecutive pixels per wave cost C4 2.7% (profiles/r04zl_c4_batch.log)
  // Three per atomic once every wave takes 256 or more (a whole C3 frame: ~405 per wave, +0.6%,
  // profiles/r05q_ab_switches.txt); the 1/8 shares (~50 per wave) keep two, where three cost their
  // bound 2.5% in round 4 (r04zj_ab_batch_policies.log)
  L.item_batch = n_queue >= batch_from * grid && (P.chunks == 1 || (bs && atoi(bs) > 0))
                     ? (bs && atoi(bs) > 0 ? atoi(bs) : (n_queue >= 256 * grid ? 3 : 2)) : 1;
  // The queue in 8 contiguous segments, each with its own counter, wave b's home segment b % 8 (the
  // XCD workgroup b runs on), a drained segment sending its waves on to the next (dt_kernels.hip),
  // for a rank's share of a split frame of one-chunk items: C3's world-8 shares 4.46 against 4.54 ms
  // (bound 0.933 against 0.921, profiles/r05zg_rank_balance_segs_default.log), C2's 0.569 against
  // 0.591. A whole frame keeps one counter (C3 -1.4%, C4 -3.4%, C2 -0.5% with eight), and so do
  // pixels of several chunks in one item (C4's world-8 shares 49.4 against 47.1 ms with eight,
  // profiles/r05zi_*). Chunk items take eight: C4's slowest world-8 share 43.97 against 45.77 ms
  // (profiles/r06c_rb_m1s8.log, r06c_rb_m1.log). DT_QUEUE_SEGS=<n> (1..8) overrides.
  const char* qs = getenv("DT_QUEUE_SEGS");
  const int qn = qs ? atoi(qs) : 0;
  L.queue_segs = qs ? (qn < 1 ? 1 : qn > DT_QSEG_MAX ? DT_QSEG_MAX : qn)
                    : (P.world > 1 && (P.chunks == 1 || chunk_items) ? DT_QSEG_MAX : 1);
  // deep-cascade waves raise their priority (dt_kernels.hip, DT_PRIO_STEPS) when the frame is split
  // over ranks, where one such wave bounds a rank's kernel, and after 2 DFS steps in whole frames of
  // several pixels per wave (spp < 64: C2, whose frame is bounded by a column of 30x-mean glossy items,
  // profiles/r06h_tail_c2.log): C2 +0.9%, C3 +0.1%, C4 -0.4% (so not there; profiles/r06o_ab.txt).
  // DT_PRIO_STEPS=<n> overrides (0: off)
  const char* ps = getenv("DT_PRIO_STEPS");
  L.prio_steps = ps ? atoi(ps) : (P.world > 1 ? 8 : P.ppw > 1 ? 2 : 0);
  return L;
}

}  // namespace dth
