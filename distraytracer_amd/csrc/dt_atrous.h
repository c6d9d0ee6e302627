// The edge-avoiding a-trous filter of dt_denoise and dt_denoise_var, written once: prepare, the tap's
// weight, one pixel of one level, finish, the level constants, the host driver, the device driver and the
// workspace layout, as templates on VAR ("with variance": dt_denoise_var). What VAR adds is behind
// `if constexpr`, so the plain filter's kernels hold no load and no register for it: V instead of the
// NaN-colour flag in E's fourth float, the 3x3 variance prefilter and the pixel's own colour factor cv_p in
// place of the level's isc, the sum SV, and the NaN test from `colour` in finish.
//
// A pixel of a level is one function (pixel) that the host loop and the level kernel both call, so the two
// agree by construction, border rule included. The kernels themselves are named in dt_denoise.hip and
// dt_denoise_var.hip (each includes this header and calls prepare_all / level_rows), so each object holds
// its own two and they keep their names.
#pragma once
#include <type_traits>
#include <utility>

#include "dt_post.h"

namespace post {

// per-level constants, from the host (level): isn, isa and the level's isz; then the plain filter's isc of
// the level, or the variance filter's sv2 = sigma_variance^2 and vf = variance_floor
struct LevelGuides {
  int32_t W, H, step, last, demodulate;
  float isn, isa, isz;
};
struct PlainLevel : LevelGuides {
  float isc;
};
struct VarLevel : LevelGuides {
  float sv2, vf;
};
template <bool VAR>
using Level = std::conditional_t<VAR, VarLevel, PlainLevel>;
template <bool VAR>
using Params = std::conditional_t<VAR, dt_denoise_var_params, dt_denoise_params>;

template <bool VAR>
Level<VAR> level(int32_t W, int32_t H, const Params<VAR>* p, int l)
{
  Level<VAR> L;
  L.W = W;
  L.H = H;
  L.step = 1 << l;
  L.last = l == p->levels - 1;
  L.demodulate = p->demodulate;
  const float up = (float)(1 << l);   // 2^l, exact
  const float sz = p->sigma_depth * up;
  L.isn = 1.0f / (p->sigma_normal * p->sigma_normal);
  L.isa = 1.0f / (p->sigma_albedo * p->sigma_albedo);
  L.isz = 1.0f / (sz * sz);
  if constexpr (VAR) {
    L.sv2 = p->sigma_variance * p->sigma_variance;
    L.vf = p->variance_floor;
  } else {
    const float sc = p->sigma_colour * (1.0f / up);   // 2^-l, exact
    L.isc = 1.0f / (sc * sc);
  }
  return L;
}

POST_HD float G(int i) { return i == 0 ? 0.5f : 0.25f; }   // the 3x3 prefilter's kernel, i in -1..1

// the colour term's factor of pixel p from its 3x3 prefiltered variance sg / gw
POST_HD float cv(float sg, float gw, const VarLevel& L)
{
  const float vbar = sg / gw;
  return 1.0f / (L.sv2 * (vbar + L.vf));
}

// the weight of tap q for pixel p: h * the four edge-stopping terms (include/dt.h); ic the colour term's
// factor (isc or cv_p); dist2 does not read the E records' fourth float
POST_HD float tap(float h, const Rec& nz_p, const Rec& ar_p, const Rec& e_p, float ic, const Rec& nz_q, const Rec& ar_q,
                  const Rec& e_q, const LevelGuides& L)
{
  const float xn = dist2(nz_p, nz_q) * L.isn;
  const float xa = dist2(ar_p, ar_q) * L.isa;
  const float xc = dist2(e_p, e_q) * ic;
  const float dz = nz_p.w - nz_q.w;
  const float xz = ((dz * dz) * ar_p.w) * L.isz;
  return (h * (R(xn) * R(xz))) * (R(xa) * R(xc));
}

// prepare: {N, Z}, {A, rz} and E0 = C / d, with the NaN-colour flag in E's fourth float or (VAR) V0, the
// variance of the demodulated colour vector. var is read with VAR only.
template <bool VAR>
POST_HD void prepare(const float* colour, const float* var, const float* A, const float* N, const float* Z, int64_t q,
                     int demodulate, Rec* nz, Rec* ar, Rec* e)
{
  const float c0 = colour[3 * q], c1 = colour[3 * q + 1], c2 = colour[3 * q + 2];
  const float a0 = A[3 * q], a1 = A[3 * q + 1], a2 = A[3 * q + 2];
  const float d0 = demod(a0, demodulate), d1 = demod(a1, demodulate), d2 = demod(a2, demodulate);
  const float z = Z[q];
  float w;
  if constexpr (VAR) {
    const float v0 = var[3 * q], v1 = var[3 * q + 1], v2 = var[3 * q + 2];
    const float x = ((v0 / (d0 * d0)) + (v1 / (d1 * d1))) + (v2 / (d2 * d2));
    w = fminf(fmaxf(x, 0.0f), 1e12f);
  } else {
    w = (c0 != c0 || c1 != c1 || c2 != c2) ? 1.0f : 0.0f;
  }
  nz[q] = Rec{N[3 * q], N[3 * q + 1], N[3 * q + 2], z};
  ar[q] = Rec{a0, a1, a2, 1.0f / (z * z + 1e-6f)};
  e[q] = Rec{c0 / d0, c1 / d1, c2 / d2, w};
}

// finish: remodulate and clamp; a NaN-colour pixel is its input (the flag, or with VAR, whose fourth float
// is V, the colour itself tells)
template <bool VAR>
POST_HD void finish(const Rec& e, const Rec& ar_p, const float* colour, int64_t p, int demodulate, float* out)
{
  bool nan;
  if constexpr (VAR) {
    const float c0 = colour[3 * p], c1 = colour[3 * p + 1], c2 = colour[3 * p + 2];
    nan = c0 != c0 || c1 != c1 || c2 != c2;
  } else {
    nan = e.w != 0.0f;
  }
  if (nan) {
    out[3 * p] = colour[3 * p];
    out[3 * p + 1] = colour[3 * p + 1];
    out[3 * p + 2] = colour[3 * p + 2];
    return;
  }
  out[3 * p] = fminf(fmaxf(e.a * demod(ar_p.a, demodulate), 0.0f), 255.0f);
  out[3 * p + 1] = fminf(fmaxf(e.b * demod(ar_p.b, demodulate), 0.0f), 255.0f);
  out[3 * p + 2] = fminf(fmaxf(e.c * demod(ar_p.c, demodulate), 0.0f), 255.0f);
}

// The pixel (r, xp) of one level. A tap row outside the image is skipped by a branch: in the kernel it is
// the same for the whole wave (a scalar branch). A tap column outside it is a lane's own: the centre
// record is loaded instead (an address inside the image) and the selects below keep the sums, which is
// exactly the skip. With VAR the 3x3 variance prefilter runs first: eight 4-byte reads of the fourth float
// of the centre's neighbours' E records (the centre's is in e_p), row and column skips as for the taps.
// The last level remodulates and writes `out` (finish): fusing it changes no rounding. A pixel that is not
// live (a lane past the row's end, working on the row's last pixel) stores nothing.
template <bool VAR>
POST_HD void pixel(const Rec* __restrict__ nz, const Rec* __restrict__ ar, const Rec* __restrict__ ein,
                   Rec* __restrict__ eout, const float* __restrict__ colour, float* __restrict__ out, Level<VAR> L,
                   int r, int xp, bool live)
{
  const int64_t p = (int64_t)r * L.W + xp;
  const Rec nz_p = nz[p], ar_p = ar[p], e_p = ein[p];
  float ic;
  if constexpr (VAR) {
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
        const float g = G(a) * G(b);
        sg = inside ? sg + g * v_q : sg;
        gw = inside ? gw + g : gw;
      }
    }
    ic = cv(sg, gw, L);
  } else {
    ic = L.isc;
  }
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, wt = 0.0f;
  [[maybe_unused]] float sv = 0.0f;
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
      const Rec nz_q = nz[q], ar_q = ar[q], e_q = ein[q];
      const float w = tap(K(i) * K(j), nz_p, ar_p, e_p, ic, nz_q, ar_q, e_q, L);
      const bool take = inside && w > 0.0f;
      s0 = take ? s0 + w * e_q.a : s0;
      s1 = take ? s1 + w * e_q.b : s1;
      s2 = take ? s2 + w * e_q.c : s2;
      wt = take ? wt + w : wt;
      if constexpr (VAR) sv = take ? sv + (w * w) * e_q.w : sv;
    }
  }
  Rec e = e_p;
  if (wt > 0.0f) {
    e.a = s0 / wt;
    e.b = s1 / wt;
    e.c = s2 / wt;
    if constexpr (VAR) e.w = sv / (wt * wt);
  }
  if (!live) return;
  if (L.last) finish<VAR>(e, ar_p, colour, p, L.demodulate, out);
  else eout[p] = e;
}

// the body of a prepare kernel: blocks of 256, grid-stride
template <bool VAR>
__device__ __forceinline__ void prepare_all(const float* colour, const float* var, const float* A, const float* N,
                                            const float* Z, int64_t n_px, int demodulate, Rec* nz, Rec* ar, Rec* e)
{
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n_px; q += (int64_t)gridDim.x * 256)
    prepare<VAR>(colour, var, A, N, Z, q, demodulate, nz, ar, e);
}

// The body of a level kernel. Block (64, 4): a wave is 64 consecutive x of one row, so for every step a
// wave's tap (i, j) is one contiguous row segment of 16-byte records and the gathers stay coalesced at
// every level; the row is made wave-uniform for the compiler (readfirstlane), so pixel's row skips are
// scalar branches. Lanes past the row's end work on the row's last pixel and store nothing.
template <bool VAR>
__device__ __forceinline__ void level_rows(const Rec* __restrict__ nz, const Rec* __restrict__ ar,
                                           const Rec* __restrict__ ein, Rec* __restrict__ eout,
                                           const float* __restrict__ colour, float* __restrict__ out, Level<VAR> L)
{
  const int x = blockIdx.x * 64 + threadIdx.x;
  const bool live = x < L.W;
  const int xp = live ? x : L.W - 1;
  const int ty = __builtin_amdgcn_readfirstlane(threadIdx.y);
  for (int r = blockIdx.y * 4 + ty; r < L.H; r += gridDim.y * 4) pixel<VAR>(nz, ar, ein, eout, colour, out, L, r, xp, live);
}

// work holds four arrays of n_px records behind its first 16-byte boundary: {N, Z}, {A, rz}, E, E' (the E
// records with the flag or V)
inline int64_t atrous_work_floats(int64_t n_px) { return 16 * n_px + WORK_SLACK; }

// The filter after the entry point's argument checks, on the host or on st: prepare, then p->levels levels
// that ping-pong between E and E'; the last writes out. `prepare_kernel` and `level_kernel` are the unit's
// own; variance is passed on with VAR only.
template <bool VAR, class PrepareKernel, class LevelKernel>
int atrous(const char* who, PrepareKernel prepare_kernel, LevelKernel level_kernel, int32_t W, int32_t H, const float* colour,
           const float* variance, const dt_features* feat, const Params<VAR>* p, float* out, float* work, int32_t on_device,
           void* stream, float* kernel_ms)
{
  const int64_t n_px = (int64_t)W * H;
  const float *A = feat->albedo, *N = feat->normal, *Z = feat->depth;
  Rec* nz = align_records(work);
  Rec *ar = nz + n_px, *ein = ar + n_px, *eout = ein + n_px;
  if (!on_device) {
    for (int64_t q = 0; q < n_px; ++q) prepare<VAR>(colour, variance, A, N, Z, q, p->demodulate, nz, ar, ein);
    for (int l = 0; l < p->levels; ++l, std::swap(ein, eout)) {
      const Level<VAR> L = level<VAR>(W, H, p, l);
      for (int r = 0; r < H; ++r)
        for (int x = 0; x < W; ++x) pixel<VAR>(nz, ar, ein, eout, colour, out, L, r, x, true);
    }
    if (kernel_ms) *kernel_ms = 0.0f;
    return DT_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  return launch(st, kernel_ms, who, [&] {
    const dim3 grid = linear_grid(n_px, 8192);
    if constexpr (VAR)
      hipLaunchKernelGGL(prepare_kernel, grid, dim3(256), 0, st, colour, variance, A, N, Z, n_px, (int)p->demodulate, nz, ar, ein);
    else
      hipLaunchKernelGGL(prepare_kernel, grid, dim3(256), 0, st, colour, A, N, Z, n_px, (int)p->demodulate, nz, ar, ein);
    hipError_t e = hipGetLastError();
    for (int l = 0; l < p->levels && e == hipSuccess; ++l, std::swap(ein, eout)) {
      hipLaunchKernelGGL(level_kernel, row_grid(W, H), dim3(64, 4), 0, st, (const Rec*)nz, (const Rec*)ar, (const Rec*)ein,
                         eout, colour, out, level<VAR>(W, H, p, l));
      e = hipGetLastError();
    }
    return e;
  });
}

}  // namespace post
