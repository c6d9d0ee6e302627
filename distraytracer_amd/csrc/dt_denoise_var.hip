// dt_variance and dt_denoise_var — variance-guided denoising of previews: dt_denoise's edge-avoiding
// a-trous filter with the colour width of every pixel taken from the variance of its own mean, which
// adaptive sampling's sums supply, and carried through the levels (the scheme of SVGF, Schied et al.
// 2017). No reference counterpart. The specification is the comment blocks of dt_variance and
// dt_denoise_var in include/dt.h; tests/denoise_var_ref.py restates them in numpy, and the host loops,
// the kernels and that restatement agree bit for bit: every operation is one rounded IEEE operation (no
// contraction, correctly rounded division), and the arithmetic is in functions (dv_variance here;
// dt_atrous.h prepare, pixel with its prefilter and taps, finish) that the host loops and the kernels both
// call.
//
// A translation unit of its own (dt_kernels.hip and dt_api.cpp stay as they are). The filter is
// dt_atrous.h's, shared with dt_denoise.hip, here with variance; R, dist2, K, the demodulation divisor, the
// record type and the host's helpers are dt_post.h's. What is here: dt_variance, the two filter kernels'
// names, the defaults and the argument checks.
#include "dt_atrous.h"

namespace {

using post::Rec;

// ---- dt_variance -------------------------------------------------------------------------------

// the variance of the mean of one channel, in grey levels squared: s1 the sum of the sample colours,
// s2 of their squares, count the samples in them (dt_adapt.h adapt_converged's d, the same order)
__host__ __device__ __forceinline__ float dv_variance(double s1, double s2, uint32_t count)
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

__global__ __launch_bounds__(256) void dt_denoise_var_prepare_kernel(const float* colour, const float* var, const float* A,
                                                                     const float* N, const float* Z, int64_t n_px,
                                                                     int demodulate, Rec* nz, Rec* ar, Rec* e)
{
  post::prepare_all<true>(colour, var, A, N, Z, n_px, demodulate, nz, ar, e);
}

// one a-trous level with the 3x3 variance prefilter before the taps (dt_atrous.h level_rows); the records:
// N|Z, A|rz, E|V
__global__ __launch_bounds__(256) void dt_denoise_var_level_kernel(const Rec* __restrict__ nz, const Rec* __restrict__ ar,
                                                                   const Rec* __restrict__ ein, Rec* __restrict__ eout,
                                                                   const float* __restrict__ colour, float* __restrict__ out,
                                                                   post::Level<true> L)
{
  post::level_rows<true>(nz, ar, ein, eout, colour, out, L);
}

constexpr post::Fail dv_fail{"dt_denoise_var"};

// the first argument check that fails, or null
const char* dv_check_params(const dt_denoise_var_params* p)
{
  if (p->levels < 1 || p->levels > 6) return "levels outside 1..6";
  if (p->demodulate != 0 && p->demodulate != 1) return "demodulate must be 0 or 1";
  if (!post::sigma_ok(p->sigma_normal)) return "sigma_normal must be > 0";
  if (!post::sigma_ok(p->sigma_depth)) return "sigma_depth must be > 0";
  if (!post::sigma_ok(p->sigma_albedo)) return "sigma_albedo must be > 0";
  if (!post::sigma_ok(p->sigma_variance)) return "sigma_variance must be > 0";
  if (!(p->variance_floor > 0.0f) || std::isinf(p->variance_floor)) return "variance_floor must be finite and > 0";
  return nullptr;
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
  hipStream_t st = (hipStream_t)stream;
  return post::launch(st, nullptr, "dt_variance", [&] {   // untimed: nothing waits
    hipLaunchKernelGGL(dt_variance_kernel, post::linear_grid(n, 8192), dim3(256), 0, st, accum, accum2, count, variance, n);
    return hipGetLastError();
  });
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
  return post::atrous_work_floats((int64_t)xRes * yRes);
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
  if (const std::string m = post::planes_missing(feat, "feat"); !m.empty()) return dv_fail(m);
  if (xRes < 1) return dv_fail("xRes < 1");
  if (yRes < 1) return dv_fail("yRes < 1");
  if (const char* bad = dv_check_params(p)) return dv_fail(bad);
  const int64_t n_px = (int64_t)xRes * yRes;
  if (post::overlap(out, 3 * n_px, colour, 3 * n_px)) return dv_fail("out aliases colour");
  if (post::overlap(out, 3 * n_px, variance, 3 * n_px)) return dv_fail("out aliases variance");
  if (post::overlap(out, 3 * n_px, work, post::atrous_work_floats(n_px))) return dv_fail("out aliases work");
  return post::atrous<true>(dv_fail.who, dt_denoise_var_prepare_kernel, dt_denoise_var_level_kernel, xRes, yRes, colour,
                            variance, feat, p, out, work, on_device, stream, kernel_ms);
}

}  // extern "C"
