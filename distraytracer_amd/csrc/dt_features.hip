// dt_features.hip — the first-hit feature buffers of dt_render_features.
// One unit per auxiliary kernel family over the device library (dt_device.h);
// launched through dt_api_aux.cpp AuxLaunch.
#include "dt_kernel_iface.h"
#include "dt_aux_wave.h"
#include "dt_hit_color.h"

// First-hit feature buffers (include/dt.h dt_render_features; no reference counterpart): for the samples
// 0 .. n_samples-1 of every owned pixel, the render's own primary ray (the trace kernel's RNG pixel,
// sample and key, camera_ray, closest_hit at shift 0 as dt_isect_kernel calls it) and, per hit, the
// base colour (hit_color; texel_color or the border colour for textured shapes, as the shading loop
// takes them), the root ray's normal (shape_norm + fixNorm) and the distance t * |ray|.
// Items and lanes as the trace kernel's: spp >= 64, one pixel per wave, lane = sample, the pixel's
// chunks in turn (the pixel block's primary list stays wave-uniform); spp < 64, P.ppw pixels per wave.
// The per-pixel sums are f64, left to right in sample order: every lane writes its FT_N values to LDS
// and lane FT_N * jj + k walks column k of pixel jj; one wave owns all chunks of a pixel, so the
// sums carry over in LDS (fsum) from chunk to chunk. A miss writes zeros: the sums start at +0 and
// x + 0 == x in every bit for every x a sum from +0 can hold (never -0), so it contributes nothing.
enum { FT_A = 0, FT_N0 = 3, FT_D = 6, FT_H = 7, FT_N = 8 };
extern "C" __global__ void __launch_bounds__(64)
dt_features_kernel(const DLaunch* __restrict__ Lp, int n_samples, float* __restrict__ albedo,
                   float* __restrict__ normal, float* __restrict__ depth, float* __restrict__ coverage,
                   int32_t* __restrict__ shape_out)
{
  const DScene& S = Lp->S;
  const DParams& P = Lp->P;
  const int lane = threadIdx.x;
  __shared__ unsigned int wc_lds[WC_N];
  // (a row is 65 doubles: the FT_N column walkers of a pixel start 130 banks apart, not on one bank)
  __shared__ double val[FT_N][DT_WAVE + 1];
  __shared__ double fsum[FT_N][DT_WAVE];
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
  for (int64_t item = blockIdx.x; item < P.n_items; item += gridDim.x) {
    for (int idx = lane; idx < group * FT_N; idx += DT_WAVE) fsum[idx % FT_N][idx / FT_N] = 0;
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
      V3 col = v3(0, 0, 0), nrm = v3(0, 0, 0);
      double dist = 0;
      if (hit) {
        const int sid = h.shape;
        const DShapeHdr hd = S.hdr[sid];
        GP g = cas(S.geom) + hd.off;
        const DMat& M = S.mat[sid];
        const V3 p = add(eye_sample, mul(h.t_min, ray0));
        nrm = shape_norm(hd.type, hd.flags, g, p, 0.0f, cnt.wc + WC_PRISM, h.ccol);
        const V3 in = normalized(ray0);
        if (dot(mul(1e4, in), nrm) >= 0) nrm = mul(-1, nrm);   // fixNorm
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
        dist = (double)h.t_min * norm(ray0);
      }
      val[FT_A + 0][lane] = col.x; val[FT_A + 1][lane] = col.y; val[FT_A + 2][lane] = col.z;
      val[FT_N0 + 0][lane] = nrm.x; val[FT_N0 + 1][lane] = nrm.y; val[FT_N0 + 2][lane] = nrm.z;
      val[FT_D][lane] = dist;
      val[FT_H][lane] = hit ? 1.0 : 0.0;
      if (valid && sample == 0 && shape_out)
        shape_out[P.layout == DT_OUT_SLAB ? px_off / 3 : (int64_t)(P.yRes - 1 - px_y) * P.xRes + px_x] = hit ? h.shape : -1;
      __syncthreads();
      int ns = n_samples - chunk * DT_WAVE;
      if (ns > per) ns = per;
      for (int idx = lane; idx < group * FT_N; idx += DT_WAVE) {
        const int jj = idx / FT_N, k = idx - jj * FT_N, base = jj * per;
        double s = fsum[k][jj];
        for (int i = 0; i < ns; ++i) s = s + val[k][base + i];
        fsum[k][jj] = s;
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
        const double n = (double)n_samples, H = fsum[FT_H][lane];
        if (albedo)
          for (int k = 0; k < 3; ++k) albedo[3 * q + k] = (float)(fsum[FT_A + k][lane] / n);
        if (normal)
          for (int k = 0; k < 3; ++k) normal[3 * q + k] = (float)(fsum[FT_N0 + k][lane] / n);
        if (coverage) coverage[q] = (float)(H / n);
        if (depth) depth[q] = H > 0 ? (float)(fsum[FT_D][lane] / H) : 0.0f;
      }
    }
    __syncthreads();   // the sums are read before the next item clears them
  }
  __syncthreads();
  const int st_of[WC_N] = {ST_RAYS, ST_SHADOW, ST_TEX, ST_STACK, ST_REFL, ST_GLOSSY, ST_UV, ST_PRISM, ST_SPHL};
  if (lane < WC_N) {
    const unsigned long long v = wc_lds[lane];
    if (v) atomicAdd(S.stats + st_of[lane], v);
  }
}
extern "C" hipError_t dt_launch_features(const void* dev_launch, int n_samples, float* albedo, float* normal, float* depth,
                                         float* coverage, int32_t* shape, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(dt_features_kernel, dim3(grid), dim3(64), 0, stream, (const DLaunch*)dev_launch, n_samples, albedo,
                     normal, depth, coverage, shape);
  return hipGetLastError();
}
extern "C" const void* dt_features_kernel_ptr(void) { return (const void*)dt_features_kernel; }
