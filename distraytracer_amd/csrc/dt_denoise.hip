// dt_denoise — feature-guided denoising of previews: an edge-avoiding a-trous wavelet filter
// (Dammertz et al. 2010) demodulated by the first-hit albedo. No reference counterpart. The
// specification is the comment block of dt_denoise in include/dt.h; tests/denoise_ref.py restates it in
// numpy, and the host loop, the kernels and that restatement agree bit for bit: every operation is one
// rounded IEEE f32 operation (no contraction, correctly rounded division), and the tap's arithmetic is
// one function (dn_tap) that the host loop and the level kernel both call.
//
// A translation unit of its own: dt_kernels.hip and dt_api.cpp, and with them every object they
// compile to, stay as they are.
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

#define DN_HD __host__ __device__ __forceinline__

// packed guides: 16-byte records, so a tap is three dwordx4 loads (N|Z, A|rz, E|flag)
struct alignas(16) DnRec {
  float a, b, c, w;
};

// per-level constants; isn, isa and the level's isc, isz come from the host (dn_consts)
struct DnLevel {
  int32_t W, H, step, last, demodulate;
  float isn, isa, isc, isz;
};

DN_HD float dn_R(float x)
{
  const float t = fmaxf(0.0f, 1.0f - x);
  return t * t;
}

DN_HD float dn_dist2(const DnRec& p, const DnRec& q)
{
  const float d0 = p.a - q.a, d1 = p.b - q.b, d2 = p.c - q.c;
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// the weight of tap q for pixel p: h * the four edge-stopping terms (include/dt.h)
DN_HD float dn_tap(float h, const DnRec& nz_p, const DnRec& ar_p, const DnRec& e_p, const DnRec& nz_q,
                   const DnRec& ar_q, const DnRec& e_q, const DnLevel& L)
{
  const float xn = dn_dist2(nz_p, nz_q) * L.isn;
  const float xa = dn_dist2(ar_p, ar_q) * L.isa;
  const float xc = dn_dist2(e_p, e_q) * L.isc;
  const float dz = nz_p.w - nz_q.w;
  const float xz = ((dz * dz) * ar_p.w) * L.isz;
  return (h * (dn_R(xn) * dn_R(xz))) * (dn_R(xa) * dn_R(xc));
}

DN_HD float dn_demod(float a, int demodulate) { return demodulate ? fmaxf(a, 0.0625f) : 1.0f; }

// prepare: {N, Z}, {A, rz} and E0 = C / d with the NaN-colour flag in E's fourth float
DN_HD void dn_prepare(const float* colour, const float* A, const float* N, const float* Z, int64_t q, int demodulate,
                      DnRec* nz, DnRec* ar, DnRec* e)
{
  const float c0 = colour[3 * q], c1 = colour[3 * q + 1], c2 = colour[3 * q + 2];
  const float a0 = A[3 * q], a1 = A[3 * q + 1], a2 = A[3 * q + 2];
  const float z = Z[q];
  nz[q] = DnRec{N[3 * q], N[3 * q + 1], N[3 * q + 2], z};
  ar[q] = DnRec{a0, a1, a2, 1.0f / (z * z + 1e-6f)};
  e[q] = DnRec{c0 / dn_demod(a0, demodulate), c1 / dn_demod(a1, demodulate), c2 / dn_demod(a2, demodulate),
               (c0 != c0 || c1 != c1 || c2 != c2) ? 1.0f : 0.0f};
}

// finish: remodulate and clamp; a NaN-colour pixel is its input
DN_HD void dn_finish(const DnRec& e, const DnRec& ar_p, const float* colour, int64_t p, int demodulate, float* out)
{
  if (e.w != 0.0f) {
    out[3 * p] = colour[3 * p];
    out[3 * p + 1] = colour[3 * p + 1];
    out[3 * p + 2] = colour[3 * p + 2];
    return;
  }
  out[3 * p] = fminf(fmaxf(e.a * dn_demod(ar_p.a, demodulate), 0.0f), 255.0f);
  out[3 * p + 1] = fminf(fmaxf(e.b * dn_demod(ar_p.b, demodulate), 0.0f), 255.0f);
  out[3 * p + 2] = fminf(fmaxf(e.c * dn_demod(ar_p.c, demodulate), 0.0f), 255.0f);
}

DN_HD float dn_K(int i) { return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f; }

__global__ __launch_bounds__(256) void dt_denoise_prepare_kernel(const float* colour, const float* A, const float* N,
                                                                 const float* Z, int64_t n_px, int demodulate,
                                                                 DnRec* nz, DnRec* ar, DnRec* e)
{
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n_px; q += (int64_t)gridDim.x * 256)
    dn_prepare(colour, A, N, Z, q, demodulate, nz, ar, e);
}

// One a-trous level. Block (64, 4): a wave is 64 consecutive x of one row, so for every step a wave's
// tap (i, j) is one contiguous row segment of 16-byte records and the gathers stay coalesced at every
// level. A tap row outside the image is the same for the whole wave (a scalar branch); a tap column
// outside it is a lane's own: the lane loads its centre record instead (an address inside the image)
// and the select below keeps S and Wt, which is exactly the skip. Lanes past the row's end work on the
// row's last pixel and store nothing. The last level remodulates and writes `out` (dn_finish): fusing it
// changes no rounding.
__global__ __launch_bounds__(256) void dt_denoise_level_kernel(const DnRec* __restrict__ nz, const DnRec* __restrict__ ar,
                                                               const DnRec* __restrict__ ein, DnRec* __restrict__ eout,
                                                               const float* __restrict__ colour, float* __restrict__ out,
                                                               DnLevel L)
{
  const int x = blockIdx.x * 64 + threadIdx.x;
  const bool live = x < L.W;
  const int xp = live ? x : L.W - 1;
  const int ty = __builtin_amdgcn_readfirstlane(threadIdx.y);
  for (int r = blockIdx.y * 4 + ty; r < L.H; r += gridDim.y * 4) {
    const int64_t p = (int64_t)r * L.W + xp;
    const DnRec nz_p = nz[p], ar_p = ar[p], e_p = ein[p];
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wt = 0.0f;
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
        const DnRec nz_q = nz[q], ar_q = ar[q], e_q = ein[q];
        const float w = dn_tap(dn_K(i) * dn_K(j), nz_p, ar_p, e_p, nz_q, ar_q, e_q, L);
        const bool take = inside && w > 0.0f;
        s0 = take ? s0 + w * e_q.a : s0;
        s1 = take ? s1 + w * e_q.b : s1;
        s2 = take ? s2 + w * e_q.c : s2;
        wt = take ? wt + w : wt;
      }
    }
    DnRec e = e_p;
    if (wt > 0.0f) {
      e.a = s0 / wt;
      e.b = s1 / wt;
      e.c = s2 / wt;
    }
    if (!live) continue;
    if (L.last) dn_finish(e, ar_p, colour, p, L.demodulate, out);
    else eout[p] = e;
  }
}

int dn_fail(const char* msg)
{
  dth::set_error(std::string("dt_denoise: ") + msg);
  return DT_E_INVALID;
}

bool dn_sigma_ok(float s) { return s > 0.0f; }   // false for a NaN

// the first argument check that fails, or null
const char* dn_check_params(const dt_denoise_params* p)
{
  if (p->levels < 1 || p->levels > 6) return "levels outside 1..6";
  if (p->demodulate != 0 && p->demodulate != 1) return "demodulate must be 0 or 1";
  if (!dn_sigma_ok(p->sigma_normal)) return "sigma_normal must be > 0";
  if (!dn_sigma_ok(p->sigma_depth)) return "sigma_depth must be > 0";
  if (!dn_sigma_ok(p->sigma_colour)) return "sigma_colour must be > 0";
  if (!dn_sigma_ok(p->sigma_albedo)) return "sigma_albedo must be > 0";
  return nullptr;
}

DnLevel dn_level(int32_t W, int32_t H, const dt_denoise_params* p, int l)
{
  DnLevel L;
  L.W = W;
  L.H = H;
  L.step = 1 << l;
  L.last = l == p->levels - 1;
  L.demodulate = p->demodulate;
  const float up = (float)(1 << l), down = 1.0f / up;   // 2^l and 2^-l, exact
  const float sc = p->sigma_colour * down, sz = p->sigma_depth * up;
  L.isn = 1.0f / (p->sigma_normal * p->sigma_normal);
  L.isa = 1.0f / (p->sigma_albedo * p->sigma_albedo);
  L.isc = 1.0f / (sc * sc);
  L.isz = 1.0f / (sz * sz);
  return L;
}

bool dn_overlap(const float* a, int64_t na, const float* b, int64_t nb)
{
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(float);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(float);
  return a0 < b1 && b0 < a1;
}

// work holds four arrays of n_px records behind its first 16-byte boundary: {N, Z}, {A, rz}, E, E'
constexpr int64_t DN_WORK_SLACK = 4;   // floats, for the alignment of a float* the caller owns

DnRec* dn_align(float* work) { return (DnRec*)(((uintptr_t)work + 15u) & ~(uintptr_t)15u); }

void dn_host(int32_t W, int32_t H, const float* colour, const dt_features* feat, const dt_denoise_params* p, float* out,
             DnRec* nz, DnRec* ar, DnRec* e0, DnRec* e1)
{
  const int64_t n_px = (int64_t)W * H;
  for (int64_t q = 0; q < n_px; ++q) dn_prepare(colour, feat->albedo, feat->normal, feat->depth, q, p->demodulate, nz, ar, e0);
  DnRec *ein = e0, *eout = e1;
  for (int l = 0; l < p->levels; ++l) {
    const DnLevel L = dn_level(W, H, p, l);
    for (int r = 0; r < H; ++r)
      for (int x = 0; x < W; ++x) {
        const int64_t pp = (int64_t)r * W + x;
        const DnRec nz_p = nz[pp], ar_p = ar[pp], e_p = ein[pp];
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wt = 0.0f;
        for (int j = -2; j <= 2; ++j) {
          const int rq = r + j * L.step;
          if (rq < 0 || rq >= H) continue;
          for (int i = -2; i <= 2; ++i) {
            const int xq = x + i * L.step;
            if (xq < 0 || xq >= W) continue;
            const int64_t q = (int64_t)rq * W + xq;
            const DnRec e_q = ein[q];
            const float w = dn_tap(dn_K(i) * dn_K(j), nz_p, ar_p, e_p, nz[q], ar[q], e_q, L);
            if (w > 0.0f) {
              s0 = s0 + w * e_q.a;
              s1 = s1 + w * e_q.b;
              s2 = s2 + w * e_q.c;
              wt = wt + w;
            }
          }
        }
        DnRec e = e_p;
        if (wt > 0.0f) {
          e.a = s0 / wt;
          e.b = s1 / wt;
          e.c = s2 / wt;
        }
        if (L.last) dn_finish(e, ar_p, colour, pp, p->demodulate, out);
        else eout[pp] = e;
      }
    DnRec* t = ein;
    ein = eout;
    eout = t;
  }
}

hipError_t dn_device(int32_t W, int32_t H, const float* colour, const dt_features* feat, const dt_denoise_params* p,
                     float* out, DnRec* nz, DnRec* ar, DnRec* e0, DnRec* e1, hipStream_t st)
{
  const int64_t n_px = (int64_t)W * H;
  int64_t blocks = (n_px + 255) / 256;
  if (blocks > 8192) blocks = 8192;   // (grid-stride past that)
  hipLaunchKernelGGL(dt_denoise_prepare_kernel, dim3((unsigned)blocks), dim3(256), 0, st, colour, (const float*)feat->albedo,
                     (const float*)feat->normal, (const float*)feat->depth, n_px, (int)p->demodulate, nz, ar, e0);
  hipError_t e = hipGetLastError();
  int64_t gy = ((int64_t)H + 3) / 4;
  if (gy > 65535) gy = 65535;   // (the kernel strides over rows past that)
  const dim3 grid((unsigned)(((int64_t)W + 63) / 64), (unsigned)gy);
  DnRec *ein = e0, *eout = e1;
  for (int l = 0; l < p->levels && e == hipSuccess; ++l) {
    hipLaunchKernelGGL(dt_denoise_level_kernel, grid, dim3(64, 4), 0, st, (const DnRec*)nz, (const DnRec*)ar,
                       (const DnRec*)ein, eout, colour, out, dn_level(W, H, p, l));
    e = hipGetLastError();
    DnRec* t = ein;
    ein = eout;
    eout = t;
  }
  return e;
}

}  // namespace

extern "C" {

void dt_denoise_params_default(dt_denoise_params* p)
{
  if (!p) return;
  p->levels = 5;
  p->demodulate = 1;
  // chosen on the quality measurement of tools/denoise_bench.py
  p->sigma_normal = 0.0625f;
  p->sigma_depth = 0.00625f;
  p->sigma_colour = 64.0f;
  p->sigma_albedo = 0.03125f;
}

int64_t dt_denoise_workspace_floats(int32_t xRes, int32_t yRes, const dt_denoise_params* p)
{
  if (xRes < 1) return dn_fail("xRes < 1");
  if (yRes < 1) return dn_fail("yRes < 1");
  if (p)
    if (const char* bad = dn_check_params(p)) return dn_fail(bad);
  return 16 * (int64_t)xRes * yRes + DN_WORK_SLACK;
}

int dt_denoise(int32_t xRes, int32_t yRes, const float* colour, const dt_features* feat, const dt_denoise_params* p,
               float* out, float* work, int32_t on_device, void* stream, float* kernel_ms)
{
  if (!colour) return dn_fail("null colour");
  if (!feat) return dn_fail("null feat");
  if (!p) return dn_fail("null params");
  if (!out) return dn_fail("null out");
  if (!work) return dn_fail("null work");
  if (!feat->albedo) return dn_fail("feat->albedo missing");
  if (!feat->normal) return dn_fail("feat->normal missing");
  if (!feat->depth) return dn_fail("feat->depth missing");
  if (xRes < 1) return dn_fail("xRes < 1");
  if (yRes < 1) return dn_fail("yRes < 1");
  if (const char* bad = dn_check_params(p)) return dn_fail(bad);
  const int64_t n_px = (int64_t)xRes * yRes;
  if (dn_overlap(out, 3 * n_px, colour, 3 * n_px)) return dn_fail("out aliases colour");
  if (dn_overlap(out, 3 * n_px, work, 16 * n_px + DN_WORK_SLACK)) return dn_fail("out aliases work");
  DnRec* nz = dn_align(work);
  DnRec *ar = nz + n_px, *e0 = ar + n_px, *e1 = e0 + n_px;
  if (!on_device) {
    dn_host(xRes, yRes, colour, feat, p, out, nz, ar, e0, e1);
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
  if (e == hipSuccess) e = dn_device(xRes, yRes, colour, feat, p, out, nz, ar, e0, e1, st);
  if (kernel_ms) {
    if (e == hipSuccess) e = hipEventRecord(ev1, st);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(kernel_ms, ev0, ev1);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  if (e != hipSuccess) {
    dth::set_error(std::string("dt_denoise: ") + hipGetErrorString(e));
    return DT_E_NO_DEVICE;
  }
  return DT_OK;
}

}  // extern "C"
