// dt_features_path.hip — the specular-path feature buffers of dt_render_features_path.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_aux_wave.h"
#include "dt_hit_color.h"
#include "dt_guide.h"

// Specular-path feature buffers (include/dt.h dt_render_features_path; no reference counterpart): the
// samples, items, lanes and LDS column sums of dt_features_kernel, but a sample's guide ray follows up to
// max_bounces perfect specular bounces (dt_guide.h guide_bounce: the trace kernel's mirror and glass
// arithmetic without the Fresnel weights) and the planes describe the surface it ends on. Segment 0 is
// the primary ray through the pixel block's primary list, as dt_features_kernel takes it; the later
// segments go as dt_rayq_kernel's rays do (pblock -1, the lanes still travelling as the mask, a void ray
// -- the refraction at normal incidence, 1 / sin_theta = inf -- not traced: the sample is a miss).
// The bounce loop is wave-uniform and capped by max_bounces: after the first bounce the wave visits the
// union of its lanes' nodes, and lanes whose sample has ended wait for the others.
// One more column than dt_features_kernel: the segments a sample followed beyond the first (counted for
// samples that end as a miss too).
enum { FP_A = 0, FP_N0 = 3, FP_D = 6, FP_H = 7, FP_B = 8, FP_N = 9 };
extern "C" __global__ void __launch_bounds__(64)
dt_features_path_kernel(const DLaunch* __restrict__ Lp, int n_samples, int max_bounces, float* __restrict__ albedo,
                        float* __restrict__ normal, float* __restrict__ depth, float* __restrict__ coverage,
                        int32_t* __restrict__ shape_out, float* __restrict__ bounces)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  // (a row is 65 doubles: the FP_N column walkers of a pixel start 130 banks apart, not on one bank)
  __shared__ double val[FP_N][DT_WAVE + 1];
  __shared__ double fsum[FP_N][DT_WAVE];
  Counters cnt = aux_counters(wc_lds, lane);
  Ctx c;
  c.S = &S;
  c.P = &P;
  c.rng.k0 = P.seed;
  c.rng.k1 = (uint32_t)P.frame;
  const bool lists = P.pl_block > 0 && P.n_fnodes > 0 && (P.ftree_mode & 1);
  const int group = P.ppw;
  const int per = P.spp < DT_WAVE ? P.spp : DT_WAVE;
  const int j = lane / per, sl = lane - j * per;
  const int chunks = (n_samples + DT_WAVE - 1) / DT_WAVE;
  unsigned long long traced = 0;   // wave-uniform: the segments traced
  for (int64_t item = blockIdx.x; item < P.n_items; item += gridDim.x) {
    for (int idx = lane; idx < group * FP_N; idx += DT_WAVE) fsum[idx % FP_N][idx / FP_N] = 0;
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
      V3 org = v3a(P.eye), ray = v3(0, 0, 0);
      if (valid) camera_ray(c, P, px_x, px_y, org, ray);
      bool live = valid;     // the sample's guide ray is still travelling
      bool ended = false;    // ... it ended on a surface
      int end_shape = -1, followed = 0;
      V3 col = v3(0, 0, 0), nrm = v3(0, 0, 0);
      double len = 0;        // the path's length so far
      for (int k = 0; k <= max_bounces && __ballot(live); ++k) {
        int pblock = -1;
        if (k == 0) {
          if (lists) {   // the block of the wave's valid pixels, when they share one
            const int blk = (px_y / P.pl_block) * P.pl_nbx + px_x / P.pl_block;
            const int b0 = __shfl(blk, (int)__builtin_ctzll(__ballot(live)));
            if (!__ballot(live && blk != b0)) pblock = b0;
          }
        } else {
          // a void ray is not traced: its sample is a miss
          live = live && isfinite(org.x) && isfinite(org.y) && isfinite(org.z) && isfinite(ray.x) &&
                 isfinite(ray.y) && isfinite(ray.z) && (ray.x != 0 || ray.y != 0 || ray.z != 0);
          if (!live) { org = v3a(P.eye); ray = v3(0, 0, 0); }
        }
        const unsigned long long am = __ballot(live);
        if (!am) break;
        traced += (unsigned long long)__popcll(am);
        HitRec h;
        h.t_min = FLT_MAX; h.shape = -1; h.ccol = -1; h.inside = 0;
        const bool any = closest_hit(S, P, live, ray, org, 0.0f, h, cnt, pblock);
        const bool hit = any && live && h.shape >= 0;
        live = hit;   // a miss ends the sample and adds nothing
        if (hit) {
          const int sid = h.shape;
          const DShapeHdr hd = S.hdr[sid];
          GP g = cas(S.geom) + hd.off;
          const DMat& M = S.mat[sid];
          const V3 p = add(org, mul(h.t_min, ray));
          V3 nk = shape_norm(hd.type, hd.flags, g, p, 0.0f, cnt.wc + WC_PRISM, h.ccol);
          const V3 in = normalized(ray);
          if (dot(mul(1e4, in), nk) >= 0) nk = mul(-1, nk);   // fixNorm
          len = len + (double)h.t_min * norm(ray);
          int go = DT_GUIDE_STOP;
          V3 ndir = v3(0, 0, 0), nstart = v3(0, 0, 0);
          if (k < max_bounces) {
            bool refl_err = false;
            go = guide_bounce(P.reflect, P.nogloss, P.refr_air, P.refr_glass, M.material, M.flags, h.inside, in, nk, p,
                              ndir, nstart, refl_err);
            if (refl_err) atomicAdd(cnt.wc + WC_REFL, 1u);
          }
          if (go != DT_GUIDE_STOP) {
            ray = ndir;
            org = nstart;
            followed += 1;
          } else {
            live = false;
            ended = true;
            end_shape = sid;
            nrm = nk;
            col = hit_color(g, M, h.ccol);
            if (M.flags & DT_F_TEXTURE) {
              double tu = 0, tv = 0;
              const int uvt = shape_uv(hd.type, hd.flags, g, p, 0.0f, tu, tv);
              if (uvt == 2) {
                col = v3a(M.bordercolor);
              } else if (uvt == 1 && M.tex >= 0) {
                col = texel_color(S, M, tu, tv);
                atomicAdd(cnt.wc + WC_TEX, 1u);
              }
              if (uvt != 0 && (tu < 0 || tv < 0 || tu > 1 || tv > 1)) atomicAdd(cnt.wc + WC_UV, 1u);
            }
          }
        }
      }
      val[FP_A + 0][lane] = col.x; val[FP_A + 1][lane] = col.y; val[FP_A + 2][lane] = col.z;
      val[FP_N0 + 0][lane] = nrm.x; val[FP_N0 + 1][lane] = nrm.y; val[FP_N0 + 2][lane] = nrm.z;
      val[FP_D][lane] = ended ? len : 0.0;
      val[FP_H][lane] = ended ? 1.0 : 0.0;
      val[FP_B][lane] = (double)followed;
      if (valid && sample == 0 && shape_out)
        shape_out[P.layout == DT_OUT_SLAB ? px_off / 3 : (int64_t)(P.yRes - 1 - px_y) * P.xRes + px_x] = ended ? end_shape : -1;
      __syncthreads();
      int ns = n_samples - chunk * DT_WAVE;
      if (ns > per) ns = per;
      for (int idx = lane; idx < group * FP_N; idx += DT_WAVE) {
        const int jj = idx / FP_N, kk = idx - jj * FP_N, base = jj * per;
        double s = fsum[kk][jj];
        for (int i = 0; i < ns; ++i) s = s + val[kk][base + i];
        fsum[kk][jj] = s;
      }
      __syncthreads();
    }
    if (lane < group) {
      int qx, qy;
      int64_t qo;
      bool qv;
      pixel_of(P, item * group + lane, qx, qy, qo, qv);
      if (qv) {
        const int64_t q = P.layout == DT_OUT_SLAB ? qo / 3 : (int64_t)(P.yRes - 1 - qy) * P.xRes + qx;
        const double n = (double)n_samples, H = fsum[FP_H][lane];
        if (albedo)
          for (int k = 0; k < 3; ++k) albedo[3 * q + k] = (float)(fsum[FP_A + k][lane] / n);
        if (normal)
          for (int k = 0; k < 3; ++k) normal[3 * q + k] = (float)(fsum[FP_N0 + k][lane] / n);
        if (coverage) coverage[q] = (float)(H / n);
        if (depth) depth[q] = H > 0 ? (float)(fsum[FP_D][lane] / H) : 0.0f;
        if (bounces) bounces[q] = (float)(fsum[FP_B][lane] / n);
      }
    }
    __syncthreads();   // the sums are read before the next item clears them
  }
  __syncthreads();
  const int st_of[WC_N] = {ST_RAYS, ST_SHADOW, ST_TEX, ST_STACK, ST_REFL, ST_GLOSSY, ST_UV, ST_PRISM, ST_SPHL};
  if (lane < WC_N) {
    const unsigned long long v = lane == WC_RAYS ? traced : wc_lds[lane];
    if (v) atomicAdd(S.stats + st_of[lane], v);
  }
}
extern "C" hipError_t dt_launch_features_path(const void* dev_launch, int n_samples, int max_bounces, float* albedo,
                                              float* normal, float* depth, float* coverage, int32_t* shape,
                                              float* bounces, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(dt_features_path_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n_samples,
                     max_bounces, albedo, normal, depth, coverage, shape, bounces);
  return hipGetLastError();
}
extern "C" const void* dt_features_path_kernel_ptr(void) { return (const void*)dt_features_path_kernel; }
