// dt_mattes.hip — the ranked per-pixel group coverage of dt_render_mattes.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_aux_wave.h"

// Object mattes (include/dt.h dt_render_mattes; no reference counterpart): for the samples 0 .. n_samples-1 of
// every owned pixel the render's own primary ray to its closest hit, as dt_features_kernel takes it (items
// and lanes, camera_ray, closest_hit at shift 0, the primary-list block rule), and per pixel the histogram
// of the hit shapes' groups (gmap[shape], or the shape itself), ranked.
// A segment is the `per` lanes of one pixel (spp >= 64: the wave; spp < 64: spp lanes, P.ppw segments). Its
// table lives in its own lanes' registers: lane sl holds entry sl (tid, tcnt), tsize is the same in every
// lane of the segment. A pixel has at most min(n_samples, DT_MATTE_TABLE) entries, so they fit (spp < 64:
// one chunk of `per` samples; spp >= 64: 64 lanes = DT_MATTE_TABLE), and the table carries over from chunk
// to chunk in registers.
// A chunk is merged by a distinct-value loop, one pass per distinct group of the segment and every segment
// at once: the segment's lowest pending lane names the group, a ballot finds its equals (popcount: how many
// samples), a ballot finds its entry; without one the group takes entry tsize, or with the table full it is
// dropped and the pixel overflows. Lowest pending lane first = order of first appearance in ascending sample
// order, the table's insertion order; no atomics, no per-sample loop.
// Ranking by counting: an entry's layer is the number of entries of its table that come before it (count
// descending, group ascending; groups are distinct, so the order is total), found in tsize shuffle steps;
// typical pixels hold one to three groups.
static_assert(DT_MATTE_TABLE == DT_WAVE, "one table entry per lane");
extern "C" __global__ void __launch_bounds__(64)
dt_mattes_kernel(const DLaunch* __restrict__ Lp, int n_samples, const int32_t* __restrict__ gmap, int layers,
                 int32_t* __restrict__ id_out, float* __restrict__ weight_out, int32_t* __restrict__ distinct_out,
                 unsigned long long* __restrict__ overflow)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  Counters cnt = aux_counters(wc_lds, lane);
  Ctx c = aux_ctx(S, P);
  const bool lists = P.pl_block > 0 && P.n_fnodes > 0 && (P.ftree_mode & 1);
  const int group = P.ppw;
  const int per = P.spp < DT_WAVE ? P.spp : DT_WAVE;
  const int j = lane / per, sl = lane - j * per, base = j * per;
  const unsigned long long segmask = per < DT_WAVE ? ((1ull << per) - 1ull) << base : ~0ull;
  const int chunks = (n_samples + DT_WAVE - 1) / DT_WAVE;
  unsigned int n_over = 0;
  for (int64_t item = blockIdx.x; item < P.n_items; item += gridDim.x) {
    int px_x = 0, px_y = 0;
    int64_t px_off = 0;
    bool px_valid = false;
    pixel_of(P, item * group + (j < group ? j : 0), px_x, px_y, px_off, px_valid);
    px_valid = px_valid && j < group;
    int tid = -1, tcnt = 0, tsize = 0;
    bool over = false;
    for (int chunk = 0; chunk < chunks; ++chunk) {
      const int sample = chunk * DT_WAVE + sl;
      const bool valid = px_valid && sample < n_samples;
      c.rng.pixel = (uint32_t)(px_y * P.xRes + px_x);
      c.rng.sample = (uint32_t)sample;
      V3 eye_sample = v3a(P.eye), ray0 = v3(0, 0, 0);
      if (valid) camera_ray(c, P, px_x, px_y, eye_sample, ray0);
      const unsigned long long vm = __ballot(valid);
      int gid = -1;   // the sample's group; -1: a miss, or no sample
      if (vm) {
        int pblock = -1;
        if (lists) {   // the block of the wave's valid pixels, when they share one
          const int blk = (px_y / P.pl_block) * P.pl_nbx + px_x / P.pl_block;
          const int b0 = __shfl(blk, (int)__builtin_ctzll(vm));
          if (!__ballot(valid && blk != b0)) pblock = b0;
        }
        HitRec h;
        h.t_min = FLT_MAX; h.shape = -1; h.ccol = -1;
        const bool any = closest_hit(S, P, valid, ray0, eye_sample, 0.0f, h, cnt, pblock);
        if (any && valid && h.shape >= 0) gid = gmap ? gmap[h.shape] : h.shape;
      }
      bool todo = gid >= 0;
      unsigned long long tm;
      while ((tm = __ballot(todo)) != 0) {
        const unsigned long long mine = tm & segmask;   // the segment's pending lanes
        const int gv = __shfl(gid, mine ? (int)__builtin_ctzll(mine) : lane);
        const bool eq = todo && gid == gv;
        const int n_eq = (int)__popcll(__ballot(eq) & segmask);
        const unsigned long long fm = __ballot(sl < tsize && tid == gv) & segmask;   // its entry, if any
        if (mine) {
          if (fm) {
            if (lane == (int)__builtin_ctzll(fm)) tcnt += n_eq;
          } else if (tsize < DT_MATTE_TABLE) {
            if (sl == tsize) { tid = gv; tcnt = n_eq; }
            ++tsize;
          } else {
            over = true;
          }
        }
        todo = todo && !eq;
      }
    }
    n_over += (unsigned int)__popcll(__ballot(over && sl == 0));
    // rank = the entries of the segment's table that come before this lane's
    const bool ent = px_valid && sl < tsize;
    int rank = 0;
    for (int i = 0; __ballot(i < tsize) != 0; ++i) {
      const int src = (base + i) & (DT_WAVE - 1);
      const int kc = __shfl(tcnt, src), ki = __shfl(tid, src);
      if (i < tsize && (kc > tcnt || (kc == tcnt && ki < tid))) ++rank;
    }
    if (px_valid) {
      const int64_t q = P.layout == DT_OUT_SLAB ? px_off / 3 : (int64_t)(P.yRes - 1 - px_y) * P.xRes + px_x;
      if (ent && rank < layers) {
        if (id_out) id_out[layers * q + rank] = tid;
        if (weight_out) weight_out[layers * q + rank] = (float)((double)tcnt / (double)n_samples);
      }
      for (int jj = sl; jj < layers; jj += per)
        if (jj >= tsize) {
          if (id_out) id_out[layers * q + jj] = -1;
          if (weight_out) weight_out[layers * q + jj] = 0.0f;
        }
      if (sl == 0 && distinct_out) distinct_out[q] = tsize;
    }
  }
  if (lane == 0 && n_over) atomicAdd(overflow, (unsigned long long)n_over);
}
extern "C" hipError_t dt_launch_mattes(const void* dev_launch, int n_samples, const int32_t* gmap, int layers, int32_t* id,
                                       float* weight, int32_t* distinct, unsigned long long* overflow, int grid,
                                       hipStream_t stream)
{
  hipLaunchKernelGGL(dt_mattes_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n_samples, gmap, layers,
                     id, weight, distinct, overflow);
  return hipGetLastError();
}
extern "C" const void* dt_mattes_kernel_ptr(void) { return (const void*)dt_mattes_kernel; }
