// What the post-processing units share (dt_denoise.hip, dt_denoise_var.hip, dt_temporal.hip,
// dt_matte_mask.hip, dt_upsample.hip; the Makefile's POST): the arithmetic that their bit-for-bit contract
// with tests/*_ref.py needs to be the same everywhere, the host's argument-check helpers, the launch grids
// and the launch epilogue with its optional timing. Each function is one rounded IEEE f32 operation after
// another in the stated parenthesisation (no contraction, correctly rounded division): the expression
// shapes here are the specification of include/dt.h, so they change only with it. Arithmetic that a single
// unit uses stays in that unit (up_T, dv_G, dv_cv, tp_dot, ...).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/dt.h"

namespace dth {
void set_error(const std::string& e);   // dt_api.cpp (dt_last_error's message)
}

namespace post {

#define POST_HD __host__ __device__ __forceinline__

// ---- arithmetic, host and device ------------------------------------------------------------------

// packed guides of the a-trous filters: 16-byte records, so a tap is three dwordx4 loads
struct alignas(16) Rec {
  float a, b, c, w;
};

// the edge-stopping function
POST_HD float R(float x)
{
  const float t = fmaxf(0.0f, 1.0f - x);
  return t * t;
}

// squared distance of the first three floats (the fourth is not read)
POST_HD float dist2(const Rec& p, const Rec& q)
{
  const float d0 = p.a - q.a, d1 = p.b - q.b, d2 = p.c - q.c;
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

POST_HD float dist2(float p0, float p1, float p2, const float* q)
{
  const float d0 = p0 - q[0], d1 = p1 - q[1], d2 = p2 - q[2];
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// the B3-spline kernel of the a-trous taps, i in -2..2
POST_HD float K(int i) { return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f; }

// the demodulation divisor of an albedo channel
POST_HD float demod(float a, int demodulate) { return demodulate ? fmaxf(a, 0.0625f) : 1.0f; }

// ---- argument checks ------------------------------------------------------------------------------

// DT_E_INVALID with "<who>: <msg>" as dt_last_error's message
struct Fail {
  const char* who;
  int operator()(const std::string& msg) const
  {
    dth::set_error(std::string(who) + ": " + msg);
    return DT_E_INVALID;
  }
};

inline bool sigma_ok(float s) { return s > 0.0f; }   // false for a NaN

// the first of the albedo, normal and depth planes that f lacks, as "<name>->albedo missing"; or empty
inline std::string planes_missing(const dt_features* f, const char* name)
{
  const char* plane = !f->albedo ? "albedo" : !f->normal ? "normal" : !f->depth ? "depth" : nullptr;
  return plane ? std::string(name) + "->" + plane + " missing" : std::string();
}

// whether the half-open ranges [a, a + na) and [b, b + nb) of 4-byte elements share a byte
inline bool overlap(const void* a, int64_t na, const void* b, int64_t nb)
{
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * 4;
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * 4;
  return a0 < b1 && b0 < a1;
}

// a workspace of records starts at the first 16-byte boundary of a float* the caller owns
constexpr int64_t WORK_SLACK = 4;   // floats

inline Rec* align_records(float* work) { return (Rec*)(((uintptr_t)work + 15u) & ~(uintptr_t)15u); }

// ---- launches -------------------------------------------------------------------------------------

// blocks of (64, 4) over a W x H image: a wave is 64 consecutive x of one row (the kernels stride over
// rows past the cap)
inline dim3 row_grid(int32_t W, int32_t H)
{
  int64_t gy = ((int64_t)H + 3) / 4;
  if (gy > 65535) gy = 65535;
  return dim3((unsigned)(((int64_t)W + 63) / 64), (unsigned)gy);
}

// blocks of 256 over n elements, at most `cap` (grid-stride past that)
inline dim3 linear_grid(int64_t n, int64_t cap)
{
  const int64_t blocks = (n + 255) / 256;
  return dim3((unsigned)(blocks < cap ? blocks : cap));
}

// Enqueues work on st (`enqueue` returns the hipError_t of its launches) and maps an error anywhere to
// DT_E_NO_DEVICE with "<who>: <hipGetErrorString>". With kernel_ms, the work is bracketed by two events
// and the call waits for the second (synchronous); without, no event exists and nothing waits.
template <class Enqueue>
int launch(hipStream_t st, float* kernel_ms, const char* who, Enqueue enqueue)
{
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipError_t e = hipSuccess;
  if (kernel_ms) {
    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, st);
  }
  if (e == hipSuccess) e = enqueue();
  if (kernel_ms) {
    if (e == hipSuccess) e = hipEventRecord(ev1, st);
    if (e == hipSuccess) e = hipEventSynchronize(ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(kernel_ms, ev0, ev1);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  if (e != hipSuccess) {
    dth::set_error(std::string(who) + ": " + hipGetErrorString(e));
    return DT_E_NO_DEVICE;
  }
  return DT_OK;
}

}  // namespace post
