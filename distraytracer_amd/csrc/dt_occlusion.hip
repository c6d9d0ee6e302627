// dt_occlusion.hip — the occlusion feature buffers of dt_render_occlusion.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_aux_wave.h"
#include "dt_occl.h"

// Occlusion feature buffers (include/dt.h dt_render_occlusion; no reference counterpart): for the samples
// 0 .. n_samples-1 of every owned pixel the render's own primary ray to its closest hit, as
// dt_features_kernel takes it (items and lanes, camera_ray, closest_hit at shift 0, the primary-list block
// rule, shape_norm + fixNorm), and from every hit ao_rays ambient-occlusion probes and one probe per listed
// light, generated in registers (dt_occl.h: one definition for this kernel and the host exports) and
// answered as dt_rayq_occl_kernel answers a ray: make_walk + occluded_walk<0/1> over the lanes that hit,
// pblock -1, tree walks only. The probe index k is wave-uniform (k < ao_rays: AO probe k; else light slot
// k - ao_rays, whose skip shape is the light's own, one value for the wave), so a probe is one walk and the
// AO loop and the light loop share one call site of the walk code.
// The lanes of a chunk are the samples of one pixel (spp >= 64) or of P.ppw pixels (spp < 64): their
// probes start next to each other. Counting is by ballot: lane jj < P.ppw owns pixel jj of the wave and
// adds the popcount of its segment's unoccluded lanes to its own LDS entry (integers: no summation order);
// a void probe is not traced and counts as unoccluded. One wave owns all chunks of a pixel, so the
// counts carry over in LDS from chunk to chunk; the owning lane stores the planes after the last chunk.
extern "C" __global__ void __launch_bounds__(64)
dt_occlusion_kernel(const DLaunch* __restrict__ Lp, int n_samples, int ao_rays, float ao_radius, int n_lights,
                    const dtd::OcclLight* __restrict__ lights, float* __restrict__ ao_out, float* __restrict__ light_out)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  __shared__ unsigned int occ[DT_OCCL_MAX_LIGHTS + 1][DT_WAVE];   // row 0: AO, row 1 + j: light slot j
  Counters cnt = aux_counters(wc_lds, lane);
  Ctx c = aux_ctx(S, P);
  const bool lists = P.pl_block > 0 && P.n_fnodes > 0 && (P.ftree_mode & 1);
  const int group = P.ppw;
  const int per = P.spp < DT_WAVE ? P.spp : DT_WAVE;
  const int j = lane / per, sl = lane - j * per;
  // the lanes of the pixel this lane owns (lane < group only)
  const unsigned long long segmask =
      per < DT_WAVE ? (lane < group ? ((1ull << per) - 1ull) << (lane * per) : 0ull) : ~0ull;
  const int chunks = (n_samples + DT_WAVE - 1) / DT_WAVE;
  const int n_probes = ao_rays + n_lights;
  unsigned long long traced = 0;   // wave-uniform
  for (int64_t item = blockIdx.x; item < P.n_items; item += gridDim.x) {
    if (lane < group)
      for (int r = 0; r <= DT_OCCL_MAX_LIGHTS; ++r) occ[r][lane] = 0;
    int px_x = 0, px_y = 0;
    int64_t px_off = 0;
    bool px_valid = false;
    pixel_of(P, item * group + (j < group ? j : 0), px_x, px_y, px_off, px_valid);
    px_valid = px_valid && j < group;
    for (int chunk = 0; chunk < chunks; ++chunk) {
      const int sample = chunk * DT_WAVE + sl;
      const bool valid = px_valid && sample < n_samples;
      c.rng.pixel = (uint32_t)(px_y * P.xRes + px_x);
      c.rng.sample = (uint32_t)sample;
      V3 eye_sample = v3a(P.eye), ray0 = v3(0, 0, 0);
      if (valid) camera_ray(c, P, px_x, px_y, eye_sample, ray0);
      const unsigned long long vm = __ballot(valid);
      bool hit = false;
      HitRec h;
      h.t_min = FLT_MAX; h.shape = -1; h.ccol = -1;
      if (vm) {
        int pblock = -1;
        if (lists) {   // the block of the wave's valid pixels, when they share one
          const int blk = (px_y / P.pl_block) * P.pl_nbx + px_x / P.pl_block;
          const int b0 = __shfl(blk, (int)__builtin_ctzll(vm));
          if (!__ballot(valid && blk != b0)) pblock = b0;
        }
        const bool any = closest_hit(S, P, valid, ray0, eye_sample, 0.0f, h, cnt, pblock);
        hit = any && valid && h.shape >= 0;
      }
      V3 p = v3(0, 0, 0), nrm = v3(0, 0, 0);
      if (hit) {
        const int sid = h.shape;
        const DShapeHdr hd = S.hdr[sid];
        GP g = cas(S.geom) + hd.off;
        p = add(eye_sample, mul(h.t_min, ray0));
        nrm = shape_norm(hd.type, hd.flags, g, p, 0.0f, cnt.wc + WC_PRISM, h.ccol);
        const V3 in = normalized(ray0);
        if (dot(mul(1e4, in), nrm) >= 0) nrm = mul(-1, nrm);   // fixNorm
      }
      if (!__ballot(hit)) continue;   // wave-uniform: a chunk of misses adds nothing
      for (int k = 0; k < n_probes; ++k) {
        V3 sray = v3(0, 0, 0);
        int skip = -1;
        if (k < ao_rays) {
          if (hit) sray = dtd::occl_ao_dir(P.seed, P.frame, c.rng.pixel, c.rng.sample, k, ao_radius, nrm);
        } else {
          const dtd::OcclLight L = lights[k - ao_rays];   // wave-uniform
          skip = uni(L.shape_index);
          if (hit) sray = dtd::occl_light_dir(P.seed, P.frame, c.rng.pixel, c.rng.sample, k - ao_rays, L, p);
        }
        // a void probe (dt_rays_occluded's rule) is an inactive lane, as in dt_rayq_occl_kernel
        const bool act = hit && isfinite(sray.x) && isfinite(sray.y) && isfinite(sray.z) && isfinite(p.x) &&
                         isfinite(p.y) && isfinite(p.z) && (sray.x != 0 || sray.y != 0 || sray.z != 0);
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
        const unsigned long long um = __ballot(hit && !occl);
        const int row = k < ao_rays ? 0 : 1 + k - ao_rays;
        if (lane < group) occ[row][lane] += (unsigned int)__popcll(um & segmask);
      }
    }
    if (lane < group) {
      int qx, qy;
      int64_t qo;
      bool qv;
      pixel_of(P, item * group + lane, qx, qy, qo, qv);
      if (qv) {
        const int64_t q = P.layout == DT_OUT_SLAB ? qo / 3 : (int64_t)(P.yRes - 1 - qy) * P.xRes + qx;
        const double n = (double)n_samples;
        if (ao_out) ao_out[q] = (float)((double)occ[0][lane] / (n * (double)ao_rays));
        if (light_out)
          for (int l = 0; l < n_lights; ++l) light_out[(int64_t)n_lights * q + l] = (float)((double)occ[1 + l][lane] / n);
      }
    }
  }
  __syncthreads();
  if (lane == 0) {
    if (traced) atomicAdd(S.stats + ST_SHADOW, traced);
    if (wc_lds[WC_PRISM]) atomicAdd(S.stats + ST_PRISM, (unsigned long long)wc_lds[WC_PRISM]);
  }
}
extern "C" hipError_t dt_launch_occlusion(const void* dev_launch, int n_samples, int ao_rays, float ao_radius, int n_lights,
                                          const void* lights, float* ao, float* light, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(dt_occlusion_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n_samples, ao_rays,
                     ao_radius, n_lights, (const dtd::OcclLight*)lights, ao, light);
  return hipGetLastError();
}
extern "C" const void* dt_occlusion_kernel_ptr(void) { return (const void*)dt_occlusion_kernel; }
