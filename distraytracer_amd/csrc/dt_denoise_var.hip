// dt_variance and dt_denoise_var — variance-guided denoising of previews: dt_denoise's edge-avoiding
// a-trous filter with the colour width of every pixel taken from the variance of its own mean, which
// adaptive sampling's sums supply, and carried through the levels (the scheme of SVGF, Schied et al.
// 2017). No reference counterpart. The specification is the comment blocks of dt_variance and
// dt_denoise_var in include/dt.h; tests/denoise_var_ref.py restates them in numpy, and the host loops,
// the kernels and that restatement agree bit for bit: every operation is one rounded IEEE operation (no
// contraction, correctly rounded division), and the arithmetic is in functions (dv_variance, dv_prepare,
// dv_vbar_term, dv_tap, dv_finish) that the host loops and the kernels both call.
//
// A translation unit of its own: dt_denoise.hip, dt_kernels.hip and dt_api.cpp, and with them every
// object they compile to, stay as they are; the small helpers (R, dist2, K) are restated here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/dt.h"

namespace dth {
void set_error(const std::string& e);   // dt_api.cpp (dt_last_error's message)
}

namespace {

#define DV_HD __host__ __device__ __forceinline__

// ---- dt_variance -------------------------------------------------------------------------------

// the variance of the mean of one channel, in grey levels squared: s1 the sum of the sample colours,
// s2 of their squares, count the samples in them (dt_adapt.h adapt_converged's d, the same order)
DV_HD float dv_variance(double s1, double s2, uint32_t count)
{
  const double n = (double)count;
  if (n < 2.0) return 0.0f;
  const double d = s2 - (s1 * s1) / n;
  const double v = fmax(d, 0.0) / (n * (n - 1.0));   // fmax drops a NaN
  return (float)(v * 65025.0);
}

__global__ __launch_bounds__(256) void dt_variance_kernel(const double* __restrict__ accum, const double* __restrict__ accum2,
                                                          const uint32_t* __restrict__ count, float* __restrict__ variance,
                                                          int64_t n)
{
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    variance[i] = dv_variance(accum[i], accum2[i], count[i / 3]);
}

// ---- dt_denoise_var ----------------------------------------------------------------------------

// packed guides: 16-byte records, so a tap is three dwordx4 loads (N|Z, A|rz, E|V)
struct alignas(16) DvRec {
  float a, b, c, w;
};

// per-level constants; isn, isa, sv2 and the level's isz come from the host (dv_level)
struct DvLevel {
  int32_t W, H, step, last, demodulate;
  float isn, isa, isz, sv2, vf;
};

DV_HD float dv_R(float x)
{
  const float t = fmaxf(0.0f, 1.0f - x);
  return t * t;
}

DV_HD float dv_dist2(const DvRec& p, const DvRec& q)
{
  const float d0 = p.a - q.a, d1 = p.b - q.b, d2 = p.c - q.c;
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

DV_HD float dv_K(int i) { return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f; }

DV_HD float dv_G(int i) { return i == 0 ? 0.5f : 0.25f; }

// the colour term's factor of pixel p from its 3x3 prefiltered variance sg / gw
DV_HD float dv_cv(float sg, float gw, const DvLevel& L)
{
  const float vbar = sg / gw;
  return 1.0f / (L.sv2 * (vbar + L.vf));
}

// the weight of tap q for pixel p: h * the four edge-stopping terms (include/dt.h); the E records carry
// V in their fourth float, which dv_dist2 does not read
DV_HD float dv_tap(float h, const DvRec& nz_p, const DvRec& ar_p, const DvRec& e_p, float cv_p, const DvRec& nz_q,
                   const DvRec& ar_q, const DvRec& e_q, const DvLevel& L)
{
  const float xn = dv_dist2(nz_p, nz_q) * L.isn;
  const float xa = dv_dist2(ar_p, ar_q) * L.isa;
  const float xc = dv_dist2(e_p, e_q) * cv_p;
  const float dz = nz_p.w - nz_q.w;
  const float xz = ((dz * dz) * ar_p.w) * L.isz;
  return (h * (dv_R(xn) * dv_R(xz))) * (dv_R(xa) * dv_R(xc));
}

DV_HD float dv_demod(float a, int demodulate) { return demodulate ? fmaxf(a, 0.0625f) : 1.0f; }

// prepare: {N, Z}, {A, rz} and {E0 = C / d, V0}: V0 the variance of the demodulated colour vector
DV_HD void dv_prepare(const float* colour, const float* var, const float* A, const float* N, const float* Z, int64_t q,
                      int demodulate, DvRec* nz, DvRec* ar, DvRec* e)
{
  const float c0 = colour[3 * q], c1 = colour[3 * q + 1], c2 = colour[3 * q + 2];
  const float v0 = var[3 * q], v1 = var[3 * q + 1], v2 = var[3 * q + 2];
  const float a0 = A[3 * q], a1 = A[3 * q + 1], a2 = A[3 * q + 2];
  const float d0 = dv_demod(a0, demodulate), d1 = dv_demod(a1, demodulate), d2 = dv_demod(a2, demodulate);
  const float z = Z[q];
  const float x = ((v0 / (d0 * d0)) + (v1 / (d1 * d1))) + (v2 / (d2 * d2));
  nz[q] = DvRec{N[3 * q], N[3 * q + 1], N[3 * q + 2], z};
  ar[q] = DvRec{a0, a1, a2, 1.0f / (z * z + 1e-6f)};
  e[q] = DvRec{c0 / d0, c1 / d1, c2 / d2, fminf(fmaxf(x, 0.0f), 1e12f)};
}

// finish: remodulate and clamp; a NaN-colour pixel is its input
DV_HD void dv_finish(const DvRec& e, const DvRec& ar_p, const float* colour, int64_t p, int demodulate, float* out)
{
  const float c0 = colour[3 * p], c1 = colour[3 * p + 1], c2 = colour[3 * p + 2];
  if (c0 != c0 || c1 != c1 || c2 != c2) {
    out[3 * p] = c0;
    out[3 * p + 1] = c1;
    out[3 * p + 2] = c2;
    return;
  }
  out[3 * p] = fminf(fmaxf(e.a * dv_demod(ar_p.a, demodulate), 0.0f), 255.0f);
  out[3 * p + 1] = fminf(fmaxf(e.b * dv_demod(ar_p.b, demodulate), 0.0f), 255.0f);
  out[3 * p + 2] = fminf(fmaxf(e.c * dv_demod(ar_p.c, demodulate), 0.0f), 255.0f);
}

__global__ __launch_bounds__(256) void dt_denoise_var_prepare_kernel(const float* colour, const float* var, const float* A,
                                                                     const float* N, const float* Z, int64_t n_px,
                                                                     int demodulate, DvRec* nz, DvRec* ar, DvRec* e)
{
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n_px; q += (int64_t)gridDim.x * 256)
    dv_prepare(colour, var, A, N, Z, q, demodulate, nz, ar, e);
}

// One a-trous level, the shape of dt_denoise_level_kernel. Block (64, 4): a wave is 64 consecutive x of
// one row, so for every step a wave's tap (i, j) is one contiguous row segment of 16-byte records. A tap
// row outside the image is the same for the whole wave (a scalar branch); a tap column outside it is a
// lane's own: the lane loads its centre record instead (an address inside the image) and the select
// keeps S, Wt and SV, which is exactly the skip. Lanes past the row's end work on the row's last pixel
// and store nothing. The 3x3 variance prefilter runs here, before the taps: eight 4-byte reads of the
// fourth float of the centre's neighbours' E records (the centre's is in e_p), row and column skips
// as for the taps. The last level remodulates and writes `out` (dv_finish).
__global__ __launch_bounds__(256) void dt_denoise_var_level_kernel(const DvRec* __restrict__ nz, const DvRec* __restrict__ ar,
                                                                   const DvRec* __restrict__ ein, DvRec* __restrict__ eout,
                                                                   const float* __restrict__ colour, float* __restrict__ out,
                                                                   DvLevel L)
{
  const int x = blockIdx.x * 64 + threadIdx.x;
  const bool live = x < L.W;
  const int xp = live ? x : L.W - 1;
  const int ty = __builtin_amdgcn_readfirstlane(threadIdx.y);
  for (int r = blockIdx.y * 4 + ty; r < L.H; r += gridDim.y * 4) {
    const int64_t p = (int64_t)r * L.W + xp;
    const DvRec nz_p = nz[p], ar_p = ar[p], e_p = ein[p];
    float sg = 0.0f, gw = 0.0f;
#pragma unroll
    for (int b = -1; b <= 1; ++b) {
      const int rq = r + b;
      if (rq < 0 || rq >= L.H) continue;   // wave-uniform
      const int64_t row = (int64_t)rq * L.W;
#pragma unroll
      for (int a = -1; a <= 1; ++a) {
        const int xq = xp + a;
        const bool inside = xq >= 0 && xq < L.W;
        const float v_q = (a == 0 && b == 0) ? e_p.w : ein[inside ? row + xq : p].w;
        const float g = dv_G(a) * dv_G(b);
        sg = inside ? sg + g * v_q : sg;
        gw = inside ? gw + g : gw;
      }
    }
    const float cv_p = dv_cv(sg, gw, L);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wt = 0.0f, sv = 0.0f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
      const int rq = r + j * L.step;
      if (rq < 0 || rq >= L.H) continue;   // wave-uniform
      const int64_t row = (int64_t)rq * L.W;
#pragma unroll
      for (int i = -2; i <= 2; ++i) {
        const int xq = xp + i * L.step;
        const bool inside = xq >= 0 && xq < L.W;
        const int64_t q = inside ? row + xq : p;
        const DvRec nz_q = nz[q], ar_q = ar[q], e_q = ein[q];
        const float w = dv_tap(dv_K(i) * dv_K(j), nz_p, ar_p, e_p, cv_p, nz_q, ar_q, e_q, L);
        const bool take = inside && w > 0.0f;
        s0 = take ? s0 + w * e_q.a : s0;
        s1 = take ? s1 + w * e_q.b : s1;
        s2 = take ? s2 + w * e_q.c : s2;
        wt = take ? wt + w : wt;
        sv = take ? sv + (w * w) * e_q.w : sv;
      }
    }
    DvRec e = e_p;
    if (wt > 0.0f) {
      e.a = s0 / wt;
      e.b = s1 / wt;
      e.c = s2 / wt;
      e.w = sv / (wt * wt);
    }
    if (!live) continue;
    if (L.last) dv_finish(e, ar_p, colour, p, L.demodulate, out);
    else eout[p] = e;
  }
}

int dv_fail(const char* msg)
{
  dth::set_error(std::string("dt_denoise_var: ") + msg);
  return DT_E_INVALID;
}

bool dv_sigma_ok(float s) { return s > 0.0f; }   // false for a NaN

// the first argument check that fails, or null
const char* dv_check_params(const dt_denoise_var_params* p)
{
  if (p->levels < 1 || p->levels > 6) return "levels outside 1..6";
  if (p->demodulate != 0 && p->demodulate != 1) return "demodulate must be 0 or 1";
  if (!dv_sigma_ok(p->sigma_normal)) return "sigma_normal must be > 0";
  if (!dv_sigma_ok(p->sigma_depth)) return "sigma_depth must be > 0";
  if (!dv_sigma_ok(p->sigma_albedo)) return "sigma_albedo must be > 0";
  if (!dv_sigma_ok(p->sigma_variance)) return "sigma_variance must be > 0";
  if (!(p->variance_floor > 0.0f) || std::isinf(p->variance_floor)) return "variance_floor must be finite and > 0";
  return nullptr;
}

DvLevel dv_level(int32_t W, int32_t H, const dt_denoise_var_params* p, int l)
{
  DvLevel L;
  L.W = W;
  L.H = H;
  L.step = 1 << l;
  L.last = l == p->levels - 1;
  L.demodulate = p->demodulate;
  const float sz = p->sigma_depth * (float)(1 << l);   // 2^l, exact
  L.isn = 1.0f / (p->sigma_normal * p->sigma_normal);
  L.isa = 1.0f / (p->sigma_albedo * p->sigma_albedo);
  L.isz = 1.0f / (sz * sz);
  L.sv2 = p->sigma_variance * p->sigma_variance;
  L.vf = p->variance_floor;
  return L;
}

bool dv_overlap(const float* a, int64_t na, const float* b, int64_t nb)
{
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(float);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(float);
  return a0 < b1 && b0 < a1;
}

// work holds four arrays of n_px records behind its first 16-byte boundary: {N, Z}, {A, rz}, {E, V}, {E', V'}
constexpr int64_t DV_WORK_SLACK = 4;   // floats, for the alignment of a float* the caller owns

DvRec* dv_align(float* work) { return (DvRec*)(((uintptr_t)work + 15u) & ~(uintptr_t)15u); }

void dv_host(int32_t W, int32_t H, const float* colour, const float* var, const dt_features* feat,
             const dt_denoise_var_params* p, float* out, DvRec* nz, DvRec* ar, DvRec* e0, DvRec* e1)
{
  const int64_t n_px = (int64_t)W * H;
  for (int64_t q = 0; q < n_px; ++q)
    dv_prepare(colour, var, feat->albedo, feat->normal, feat->depth, q, p->demodulate, nz, ar, e0);
  DvRec *ein = e0, *eout = e1;
  for (int l = 0; l < p->levels; ++l) {
    const DvLevel L = dv_level(W, H, p, l);
    for (int r = 0; r < H; ++r)
      for (int x = 0; x < W; ++x) {
        const int64_t pp = (int64_t)r * W + x;
        const DvRec nz_p = nz[pp], ar_p = ar[pp], e_p = ein[pp];
        float sg = 0.0f, gw = 0.0f;
        for (int b = -1; b <= 1; ++b) {
          const int rq = r + b;
          if (rq < 0 || rq >= H) continue;
          for (int a = -1; a <= 1; ++a) {
            const int xq = x + a;
            if (xq < 0 || xq >= W) continue;
            const float g = dv_G(a) * dv_G(b);
            sg = sg + g * ein[(int64_t)rq * W + xq].w;
            gw = gw + g;
          }
        }
        const float cv_p = dv_cv(sg, gw, L);
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wt = 0.0f, sv = 0.0f;
        for (int j = -2; j <= 2; ++j) {
          const int rq = r + j * L.step;
          if (rq < 0 || rq >= H) continue;
          for (int i = -2; i <= 2; ++i) {
            const int xq = x + i * L.step;
            if (xq < 0 || xq >= W) continue;
            const int64_t q = (int64_t)rq * W + xq;
            const DvRec e_q = ein[q];
            const float w = dv_tap(dv_K(i) * dv_K(j), nz_p, ar_p, e_p, cv_p, nz[q], ar[q], e_q, L);
            if (w > 0.0f) {
              s0 = s0 + w * e_q.a;
              s1 = s1 + w * e_q.b;
              s2 = s2 + w * e_q.c;
              wt = wt + w;
              sv = sv + (w * w) * e_q.w;
            }
          }
        }
        DvRec e = e_p;
        if (wt > 0.0f) {
          e.a = s0 / wt;
          e.b = s1 / wt;
          e.c = s2 / wt;
          e.w = sv / (wt * wt);
        }
        if (L.last) dv_finish(e, ar_p, colour, pp, p->demodulate, out);
        else eout[pp] = e;
      }
    DvRec* t = ein;
    ein = eout;
    eout = t;
  }
}

hipError_t dv_device(int32_t W, int32_t H, const float* colour, const float* var, const dt_features* feat,
                     const dt_denoise_var_params* p, float* out, DvRec* nz, DvRec* ar, DvRec* e0, DvRec* e1, hipStream_t st)
{
  const int64_t n_px = (int64_t)W * H;
  int64_t blocks = (n_px + 255) / 256;
  if (blocks > 8192) blocks = 8192;   // (grid-stride past that)
  hipLaunchKernelGGL(dt_denoise_var_prepare_kernel, dim3((unsigned)blocks), dim3(256), 0, st, colour, var,
                     (const float*)feat->albedo, (const float*)feat->normal, (const float*)feat->depth, n_px,
                     (int)p->demodulate, nz, ar, e0);
  hipError_t e = hipGetLastError();
  int64_t gy = ((int64_t)H + 3) / 4;
  if (gy > 65535) gy = 65535;   // (the kernel strides over rows past that)
  const dim3 grid((unsigned)(((int64_t)W + 63) / 64), (unsigned)gy);
  DvRec *ein = e0, *eout = e1;
  for (int l = 0; l < p->levels && e == hipSuccess; ++l) {
    hipLaunchKernelGGL(dt_denoise_var_level_kernel, grid, dim3(64, 4), 0, st, (const DvRec*)nz, (const DvRec*)ar,
                       (const DvRec*)ein, eout, colour, out, dv_level(W, H, p, l));
    e = hipGetLastError();
    DvRec* t = ein;
    ein = eout;
    eout = t;
  }
  return e;
}

}  // namespace

extern "C" {

int dt_variance(const dt_globals* g, const dt_tiles* tiles, const double* accum, const double* accum2,
                const uint32_t* count, float* variance, int32_t on_device, void* stream)
{
  if (!g || !accum || !accum2 || !count || !variance) {
    dth::set_error("dt_variance: null argument");
    return DT_E_INVALID;
  }
  const int64_t n = dt_accum_doubles(g, tiles);
  if (n < 0) {
    dth::set_error("dt_variance: invalid globals or tiles");
    return DT_E_INVALID;
  }
  if (!on_device) {
    for (int64_t i = 0; i < n; ++i) variance[i] = dv_variance(accum[i], accum2[i], count[i / 3]);
    return DT_OK;
  }
  if (n == 0) return DT_OK;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;   // (grid-stride past that)
  hipLaunchKernelGGL(dt_variance_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, accum, accum2, count,
                     variance, n);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    dth::set_error(std::string("dt_variance: ") + hipGetErrorString(e));
    return DT_E_NO_DEVICE;
  }
  return DT_OK;
}

void dt_denoise_var_params_default(dt_denoise_var_params* p)
{
  if (!p) return;
  p->levels = 5;
  p->demodulate = 1;
  // chosen on the quality measurement of tools/denoise_bench.py --variance
  p->sigma_normal = 0.0625f;
  p->sigma_depth = 0.00625f;
  p->sigma_albedo = 0.03125f;
  p->sigma_variance = 4.0f;
  p->variance_floor = 0.25f;
  p->_pad = 0.0f;
}

int64_t dt_denoise_var_workspace_floats(int32_t xRes, int32_t yRes, const dt_denoise_var_params* p)
{
  if (xRes < 1) return dv_fail("xRes < 1");
  if (yRes < 1) return dv_fail("yRes < 1");
  if (p)
    if (const char* bad = dv_check_params(p)) return dv_fail(bad);
  return 16 * (int64_t)xRes * yRes + DV_WORK_SLACK;
}

int dt_denoise_var(int32_t xRes, int32_t yRes, const float* colour, const float* variance, const dt_features* feat,
                   const dt_denoise_var_params* p, float* out, float* work, int32_t on_device, void* stream,
                   float* kernel_ms)
{
  if (!colour) return dv_fail("null colour");
  if (!variance) return dv_fail("null variance");
  if (!feat) return dv_fail("null feat");
  if (!p) return dv_fail("null params");
  if (!out) return dv_fail("null out");
  if (!work) return dv_fail("null work");
  if (!feat->albedo) return dv_fail("feat->albedo missing");
  if (!feat->normal) return dv_fail("feat->normal missing");
  if (!feat->depth) return dv_fail("feat->depth missing");
  if (xRes < 1) return dv_fail("xRes < 1");
  if (yRes < 1) return dv_fail("yRes < 1");
  if (const char* bad = dv_check_params(p)) return dv_fail(bad);
  const int64_t n_px = (int64_t)xRes * yRes;
  if (dv_overlap(out, 3 * n_px, colour, 3 * n_px)) return dv_fail("out aliases colour");
  if (dv_overlap(out, 3 * n_px, variance, 3 * n_px)) return dv_fail("out aliases variance");
  if (dv_overlap(out, 3 * n_px, work, 16 * n_px + DV_WORK_SLACK)) return dv_fail("out aliases work");
  DvRec* nz = dv_align(work);
  DvRec *ar = nz + n_px, *e0 = ar + n_px, *e1 = e0 + n_px;
  if (!on_device) {
    dv_host(xRes, yRes, colour, variance, feat, p, out, nz, ar, e0, e1);
    if (kernel_ms) *kernel_ms = 0.0f;
    return DT_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipError_t e = hipSuccess;
  if (kernel_ms) {
    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, st);
  }
  if (e == hipSuccess) e = dv_device(xRes, yRes, colour, variance, feat, p, out, nz, ar, e0, e1, st);
  if (kernel_ms) {
    if (e == hipSuccess) e = hipEventRecord(ev1, st);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(kernel_ms, ev0, ev1);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  if (e != hipSuccess) {
    dth::set_error(std::string("dt_denoise_var: ") + hipGetErrorString(e));
    return DT_E_NO_DEVICE;
  }
  return DT_OK;
}

}  // extern "C"
