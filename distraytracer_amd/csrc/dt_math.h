// dt_math.h — double-precision 3-vectors with the reference's Eigen semantics, usable from
// host precomputation (g++ -ffp-contract=off) and device code (hipcc -ffp-contract=off).
// The reference's VEC3 is Eigen::Matrix<double,3,1> (SETTINGS.h:13,20); the operation
// orders below are those of Eigen 3.3/3.4's default x86-64 SSE2 build:
//   dot = (a0*b0 + a1*b1) + a2*b2 ; normalized = a / sqrt(dot(a,a)) if > 0 ;
//   isApprox(0) <=> dot(a,a) <= 1e-24*min(dot(a,a),0) ; cross as in Eigen's cross_impl.
// Identical IEEE operation sequences on host and device give identical bits (division and
// sqrt are correctly rounded on both; no FMA contraction anywhere).
#pragma once

#if defined(__HIPCC__)
#define DT_HD __host__ __device__ __forceinline__
#else
#define DT_HD inline
#endif

#include <math.h>
#include <float.h>
#include <stdint.h>

namespace dtm {

struct V3 {
  double x, y, z;
};

DT_HD V3 v3(double x, double y, double z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
DT_HD V3 v3a(const double* a) { return v3(a[0], a[1], a[2]); }
DT_HD V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
DT_HD V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
DT_HD V3 mul(double s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
DT_HD V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
DT_HD V3 divs_plain(V3 a, double s) { return v3(a.x / s, a.y / s, a.z / s); }
// DT_VDIV=1 (default): device code divides a vector's three components by one s with one reciprocal
// refinement instead of three (DT_VDIV=0: three plain divisions, as the host always does).
#ifndef DT_VDIV
#define DT_VDIV 1
#endif
#if defined(__HIPCC__)
// The compiler's f64 division n / d on gfx950, in its order (read off the ISA of the builds without this):
//   ds = div_scale(d, d, n); r = rcp(ds); e = fma(-ds, r, 1); r = fma(r, e, r); e = fma(-ds, r, 1);
//   r = fma(r, e, r); ns, vcc = div_scale(n, d, n); q = ns * r; t = fma(-ds, q, ns);
//   div_fixup(div_fmas(t, r, q, vcc), d, n)
// div_scale names the numerator, so the compiler keeps one r chain per quotient; but ds is the same bit
// pattern for all three unless an exponent is near the range's ends. Where the three ds are bitwise equal
// the three r chains are the same instructions on the same operands: one is computed, and every quotient
// is the plain division's sequence on the plain division's operands, so its bits. Any other lane
// divides plainly in a branch (shared = false there). The test of equality is the only guard.
__device__ __forceinline__ double vdiv_quot(double n, double d, double ds, double r)
{
  bool vcc;
  const double ns = __builtin_amdgcn_div_scale(n, d, true, &vcc);
  const double q = ns * r;
  const double t = __builtin_fma(-ds, q, ns);
  return __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(t, r, q, vcc), d, n);
}
__device__ __forceinline__ V3 divs_shared(V3 a, double s, bool& shared)
{
  bool unused;
  const double dx = __builtin_amdgcn_div_scale(a.x, s, false, &unused);
  const double dy = __builtin_amdgcn_div_scale(a.y, s, false, &unused);
  const double dz = __builtin_amdgcn_div_scale(a.z, s, false, &unused);
  const uint64_t bx = __builtin_bit_cast(uint64_t, dx);
  shared = bx == __builtin_bit_cast(uint64_t, dy) && bx == __builtin_bit_cast(uint64_t, dz);
  if (__builtin_expect(!shared, 0)) return divs_plain(a, s);
  double r = __builtin_amdgcn_rcp(dx);
  double e = __builtin_fma(-dx, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-dx, r, 1.0);
  r = __builtin_fma(r, e, r);
  return v3(vdiv_quot(a.x, s, dx, r), vdiv_quot(a.y, s, dx, r), vdiv_quot(a.z, s, dx, r));
}
#endif
DT_HD V3 divs(V3 a, double s)
{
#if defined(__HIP_DEVICE_COMPILE__) && DT_VDIV
  bool shared;
  return divs_shared(a, s, shared);
#else
  return divs_plain(a, s);
#endif
}
DT_HD double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
DT_HD V3 cross(V3 a, V3 b)
{
  return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
DT_HD double norm(V3 a) { return sqrt(dot(a, a)); }
// DT_VNORM=1 (default): device code takes a vector's length and its normalisation from one square-root
// refinement (DT_VNORM=0: sqrt, then a division that starts again from v_rcp_f64, as the host always does).
#ifndef DT_VNORM
#define DT_VNORM 1
#endif
#if defined(__HIPCC__)
// The compiler's sqrt(d) for f64 on gfx950, in its order (read off the ISA of the builds without this):
//   sc = d < 2^-767; x = ldexp(d, sc ? 256 : 0); y = rsq(x); g = x * y; h = y * 0.5; r = fma(-h, g, 0.5);
//   g = fma(g, r, g); h = fma(h, r, h); e = fma(-g, g, x); g = fma(e, h, g); e = fma(-g, g, x);
//   g = fma(e, h, g); g = ldexp(g, sc ? -128 : 0); class(x, +-0 | +inf) ? x : g
// In range (below) nothing is scaled and the class test fails, so s restates the middle of it operation
// for operation: the bits of sqrt(d). h ends as 1 / (2 sqrt(d)) to about 2^-50, so 2h (exact) with one
// Newton step against the rounded s is 1 / s to about 2^-100 before its rounding, which is what the
// division's v_rcp_f64 and two steps arrive at; the quotients then take the division's own q = n * r,
// t = fma(-s, q, n), fma(t, r, q), correctly rounded with either r.
// In range: 2^-600 <= d < 2^600 (so 2^-300 <= s <= 2^300; false for NaN) and 2^-600 <= |n| for each
// component n (|n| <= s always). Far inside every threshold of the plain sequences: sqrt scales below
// d = 2^-767; v_div_scale_f64 leaves the divisor s and the numerator n as they are and vcc clear unless
// n or s is 0, s is subnormal, 1 / s is (s >= 2^1022), n / s is (exponents more than 1022 apart, here at
// most 900), the exponents are 768 or more apart the other way (|n| <= s) or n is below 2^-969;
// v_div_fixup_f64 passes the quotient through unless an operand is 0, inf or NaN or the exponents are
// more than 1075 apart. So div_scale, div_fmas' scaling and div_fixup are identities here and are left
// out. Any other lane (zero or tiny components, huge, inf, NaN) takes sqrt and divs in a branch.
__device__ __forceinline__ double vnorm_quot(double n, double s, double r)
{
  const double q = n * r;
  const double t = __builtin_fma(-s, q, n);
  return __builtin_fma(t, r, q);
}
__device__ __forceinline__ V3 vnorm_fused(V3 a, double d, double& s, bool& fused)
{
  // on the high words (sign, exponent field, 20 fraction bits), as integers: no f64 literal to materialise;
  // d is +0 or more, or a NaN, whose high word lies above hi with either sign
  const uint32_t lo = (1023u - 600u) << 20, hi = (1023u + 600u) << 20;
  const uint32_t hd = (uint32_t)(__builtin_bit_cast(uint64_t, d) >> 32);
  const uint32_t hx = (uint32_t)(__builtin_bit_cast(uint64_t, a.x) >> 32) & 0x7fffffffu;
  const uint32_t hy = (uint32_t)(__builtin_bit_cast(uint64_t, a.y) >> 32) & 0x7fffffffu;
  const uint32_t hz = (uint32_t)(__builtin_bit_cast(uint64_t, a.z) >> 32) & 0x7fffffffu;
  const uint32_t hmin = hx < hy ? (hx < hz ? hx : hz) : (hy < hz ? hy : hz);
  fused = hd - lo < hi - lo && hmin >= lo;
  if (__builtin_expect(!fused, 0)) {
    s = sqrt(d);
    if (d > 0) return divs(a, s);
    return a;
  }
  const double y = __builtin_amdgcn_rsq(d);
  double g = d * y;
  double h = y * 0.5;
  const double r0 = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r0, g);
  h = __builtin_fma(h, r0, h);
  double e = __builtin_fma(-g, g, d);
  g = __builtin_fma(e, h, g);
  e = __builtin_fma(-g, g, d);
  g = __builtin_fma(e, h, g);
  s = g;
  double r = h + h;
  e = __builtin_fma(-g, r, 1.0);
  r = __builtin_fma(r, e, r);
  return v3(vnorm_quot(a.x, g, r), vnorm_quot(a.y, g, r), vnorm_quot(a.z, g, r));
}
#endif
// normalized(a) and, in len, norm(a)
DT_HD V3 normalized_len(V3 a, double& len)
{
  const double n = dot(a, a);
#if defined(__HIP_DEVICE_COMPILE__) && DT_VNORM
  bool fused;
  return vnorm_fused(a, n, len, fused);
#else
  len = sqrt(n);
  if (n > 0) return divs(a, len);
  return a;
#endif
}
DT_HD V3 normalized(V3 a)
{
#if defined(__HIP_DEVICE_COMPILE__) && DT_VNORM
  double len;
  return normalized_len(a, len);
#else
  double n = dot(a, a);
  if (n > 0) return divs(a, sqrt(n));
  return a;
#endif
}
DT_HD double dmin(double a, double b) { return (b < a) ? b : a; }   // std::min
DT_HD double dmax(double a, double b) { return (a < b) ? b : a; }   // std::max
DT_HD float fminr(float a, float b) { return (b < a) ? b : a; }
DT_HD float fmaxr(float a, float b) { return (a < b) ? b : a; }
DT_HD bool is_approx_zero(V3 a)
{
  double s = dot(a, a);
  return s <= 1e-24 * dmin(s, 0.0);
}
DT_HD V3 cmin(V3 a, V3 b) { return v3(dmin(a.x, b.x), dmin(a.y, b.y), dmin(a.z, b.z)); }
DT_HD V3 cmax(V3 a, V3 b) { return v3(dmax(a.x, b.x), dmax(a.y, b.y), dmax(a.z, b.z)); }
DT_HD V3 cwise(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
// helpers.h:231-236 — clamp takes and returns float
DT_HD float clampf01(float v)
{
  if (v < 0.0) return 0.0f;
  else if (v > 1.0) return 1.0f;
  return v;
}

}  // namespace dtm
