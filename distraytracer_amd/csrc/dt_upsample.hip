// dt_upsample — guided upsampling of previews: joint-bilateral upsampling (Kopf et al. 2007) of a
// low-resolution colour image demodulated by its first-hit albedo, steered by full-resolution albedo,
// normal and depth, remodulated by the full-resolution albedo. No reference counterpart. The
// specification is the comment block of dt_upsample in include/dt.h; tests/upsample_ref.py restates it in
// numpy, and the host loop, the kernel and that restatement agree bit for bit: every operation is one
// rounded IEEE f32 operation (no contraction, correctly rounded division), and a pixel's arithmetic is one
// function (up_pixel) that the host loop and the kernel both call.
//
// A translation unit of its own (dt_kernels.hip and dt_api.cpp stay as they are). R, dist2, the
// demodulation divisor, the host's helpers and the timed launch are dt_post.h's; the tent up_T is used here
// alone and stays here.
#include "dt_post.h"

namespace {

#define UP_HD __host__ __device__ __forceinline__

// everything a pixel needs: the planes of both resolutions and the host's constants
struct UpArgs {
  const float *C_lo, *A_lo, *N_lo, *Z_lo;   // w x h
  const float *A_hi, *N_hi, *Z_hi;          // W x H
  float* out;                               // 3*W*H
  int32_t W, H, w, h, s, demodulate;
  float isn, isa, isz, fs;
};

UP_HD float up_T(float t) { return fmaxf(0.0f, 1.0f - fabsf(t) * 0.5f); }

// The full-resolution pixel (R, X), 0 <= R < H, 0 <= X < W: its nine taps in the stated order, the
// fallback and the store (include/dt.h). Every low-resolution read is at a tap inside w x h.
UP_HD void up_pixel(const UpArgs& a, int R, int X)
{
  const int64_t p = (int64_t)R * a.W + X;
  const float a0 = a.A_hi[3 * p], a1 = a.A_hi[3 * p + 1], a2 = a.A_hi[3 * p + 2];
  const float n0 = a.N_hi[3 * p], n1 = a.N_hi[3 * p + 1], n2 = a.N_hi[3 * p + 2];
  const float z = a.Z_hi[p];
  const float rz = 1.0f / (z * z + 1e-6f);
  const int xc = X / a.s, rc = R / a.s;
  const float fx = ((float)X + 0.5f) / a.fs - 0.5f;
  const float fy = ((float)R + 0.5f) / a.fs - 0.5f;
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wt = 0.0f;
  for (int j = -1; j <= 1; ++j) {
    const int rq = rc + j;
    if (rq < 0 || rq >= a.h) continue;
    const float ty = up_T(fy - (float)rq);
    for (int i = -1; i <= 1; ++i) {
      const int xq = xc + i;
      if (xq < 0 || xq >= a.w) continue;
      const int64_t q = (int64_t)rq * a.w + xq;
      const float c0 = a.C_lo[3 * q], c1 = a.C_lo[3 * q + 1], c2 = a.C_lo[3 * q + 2];
      if (c0 != c0 || c1 != c1 || c2 != c2) continue;   // a bad tap
      const float* Aq = a.A_lo + 3 * q;
      const float hsp = up_T(fx - (float)xq) * ty;
      const float xn = post::dist2(n0, n1, n2, a.N_lo + 3 * q) * a.isn;
      const float xa = post::dist2(a0, a1, a2, Aq) * a.isa;
      const float dz = z - a.Z_lo[q];
      const float xz = ((dz * dz) * rz) * a.isz;
      const float wq = (hsp * (post::R(xn) * post::R(xz))) * post::R(xa);
      if (wq > 0.0f) {
        s0 = s0 + wq * (c0 / post::demod(Aq[0], a.demodulate));
        s1 = s1 + wq * (c1 / post::demod(Aq[1], a.demodulate));
        s2 = s2 + wq * (c2 / post::demod(Aq[2], a.demodulate));
        wt = wt + wq;
      }
    }
  }
  float e0, e1, e2;
  if (wt > 0.0f) {
    e0 = s0 / wt;
    e1 = s1 / wt;
    e2 = s2 / wt;
  } else {
    const int64_t q = (int64_t)rc * a.w + xc;   // the nearest low-resolution pixel
    const float c0 = a.C_lo[3 * q], c1 = a.C_lo[3 * q + 1], c2 = a.C_lo[3 * q + 2];
    if (c0 != c0 || c1 != c1 || c2 != c2) {
      a.out[3 * p] = c0;
      a.out[3 * p + 1] = c1;
      a.out[3 * p + 2] = c2;
      return;
    }
    e0 = c0 / post::demod(a.A_lo[3 * q], a.demodulate);
    e1 = c1 / post::demod(a.A_lo[3 * q + 1], a.demodulate);
    e2 = c2 / post::demod(a.A_lo[3 * q + 2], a.demodulate);
  }
  a.out[3 * p] = fminf(fmaxf(e0 * post::demod(a0, a.demodulate), 0.0f), 255.0f);
  a.out[3 * p + 1] = fminf(fmaxf(e1 * post::demod(a1, a.demodulate), 0.0f), 255.0f);
  a.out[3 * p + 2] = fminf(fmaxf(e2 * post::demod(a2, a.demodulate), 0.0f), 255.0f);
}

// Block (64, 4): a wave is 64 consecutive X of one full-resolution row, so its reads of A, N, Z and its
// stores are contiguous segments, and its taps are at most 64/s + 2 consecutive low-resolution records of
// three rows: s neighbouring lanes read the same record and the block's whole footprint,
// (64/s + 2) x (4/s + 2) records of 40 bytes, stays in the vector L1 between its waves. The tap's row
// test is the same for the whole wave; its column test and the weight test are a lane's own. A lane past
// the row's end does nothing; there is no barrier.
__global__ __launch_bounds__(256) void dt_upsample_kernel(UpArgs a)
{
  const int64_t X = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (X >= a.W) return;
  for (int64_t R = (int64_t)blockIdx.y * 4 + threadIdx.y; R < a.H; R += (int64_t)gridDim.y * 4) up_pixel(a, (int)R, (int)X);
}

constexpr post::Fail up_fail{"dt_upsample"};

}  // namespace

extern "C" {

void dt_upsample_params_default(dt_upsample_params* p)
{
  if (!p) return;
  p->factor = 2;
  p->demodulate = 1;
  // chosen on the quality measurement of tools/upsample_bench.py
  p->sigma_normal = 1.0f;
  p->sigma_depth = 0.2f;
  p->sigma_albedo = 0.5f;
  p->_pad = 0.0f;
}

int dt_upsample(int32_t xRes, int32_t yRes, const float* colour_lo, const dt_features* feat_lo, const dt_features* feat_hi,
                const dt_upsample_params* p, float* out, int32_t on_device, void* stream, float* kernel_ms)
{
  if (!colour_lo) return up_fail("null colour_lo");
  if (!feat_lo) return up_fail("null feat_lo");
  if (!feat_hi) return up_fail("null feat_hi");
  if (!p) return up_fail("null params");
  if (!out) return up_fail("null out");
  if (const std::string m = post::planes_missing(feat_lo, "feat_lo"); !m.empty()) return up_fail(m);
  if (const std::string m = post::planes_missing(feat_hi, "feat_hi"); !m.empty()) return up_fail(m);
  if (xRes < 1) return up_fail("xRes < 1");
  if (yRes < 1) return up_fail("yRes < 1");
  if (p->factor < 2 || p->factor > 4) return up_fail("factor outside 2..4");
  if (xRes % p->factor) return up_fail("xRes is not a multiple of factor");
  if (yRes % p->factor) return up_fail("yRes is not a multiple of factor");
  if (p->demodulate != 0 && p->demodulate != 1) return up_fail("demodulate must be 0 or 1");
  if (!post::sigma_ok(p->sigma_normal)) return up_fail("sigma_normal must be > 0");
  if (!post::sigma_ok(p->sigma_depth)) return up_fail("sigma_depth must be > 0");
  if (!post::sigma_ok(p->sigma_albedo)) return up_fail("sigma_albedo must be > 0");
  UpArgs a;
  a.C_lo = colour_lo;
  a.A_lo = feat_lo->albedo;
  a.N_lo = feat_lo->normal;
  a.Z_lo = feat_lo->depth;
  a.A_hi = feat_hi->albedo;
  a.N_hi = feat_hi->normal;
  a.Z_hi = feat_hi->depth;
  a.out = out;
  a.W = xRes;
  a.H = yRes;
  a.s = p->factor;
  a.w = xRes / a.s;
  a.h = yRes / a.s;
  a.demodulate = p->demodulate;
  a.isn = 1.0f / (p->sigma_normal * p->sigma_normal);
  a.isa = 1.0f / (p->sigma_albedo * p->sigma_albedo);
  a.isz = 1.0f / (p->sigma_depth * p->sigma_depth);
  a.fs = (float)a.s;
  const int64_t n_hi = (int64_t)a.W * a.H, n_lo = (int64_t)a.w * a.h;
  if (post::overlap(out, 3 * n_hi, a.C_lo, 3 * n_lo)) return up_fail("out aliases colour_lo");
  if (post::overlap(out, 3 * n_hi, a.A_lo, 3 * n_lo)) return up_fail("out aliases feat_lo->albedo");
  if (post::overlap(out, 3 * n_hi, a.N_lo, 3 * n_lo)) return up_fail("out aliases feat_lo->normal");
  if (post::overlap(out, 3 * n_hi, a.Z_lo, n_lo)) return up_fail("out aliases feat_lo->depth");
  if (post::overlap(out, 3 * n_hi, a.A_hi, 3 * n_hi)) return up_fail("out aliases feat_hi->albedo");
  if (post::overlap(out, 3 * n_hi, a.N_hi, 3 * n_hi)) return up_fail("out aliases feat_hi->normal");
  if (post::overlap(out, 3 * n_hi, a.Z_hi, n_hi)) return up_fail("out aliases feat_hi->depth");
  if (!on_device) {
    for (int R = 0; R < a.H; ++R)
      for (int X = 0; X < a.W; ++X) up_pixel(a, R, X);
    if (kernel_ms) *kernel_ms = 0.0f;
    return DT_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  return post::launch(st, kernel_ms, up_fail.who, [&] {
    hipLaunchKernelGGL(dt_upsample_kernel, post::row_grid(a.W, a.H), dim3(64, 4), 0, st, a);
    return hipGetLastError();
  });
}

}  // extern "C"
