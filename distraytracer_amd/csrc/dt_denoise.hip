// dt_denoise — feature-guided denoising of previews: an edge-avoiding a-trous wavelet filter
// (Dammertz et al. 2010) demodulated by the first-hit albedo. No reference counterpart. The
// specification is the comment block of dt_denoise in include/dt.h; tests/denoise_ref.py restates it in
// numpy, and the host loop, the kernels and that restatement agree bit for bit: every operation is one
// rounded IEEE f32 operation (no contraction, correctly rounded division), and a pixel's arithmetic, taps
// and border rule included, is one function (dt_atrous.h pixel) that the host loop and the level kernel
// both call.
//
// A translation unit of its own (dt_kernels.hip and dt_api.cpp stay as they are). The filter is
// dt_atrous.h's, shared with dt_denoise_var.hip, here without variance; R, dist2, K, the demodulation
// divisor, the record type and the host's helpers are dt_post.h's. What is here: the two kernels' names,
// the defaults and the argument checks.
#include "dt_atrous.h"

namespace {

using post::Rec;

__global__ __launch_bounds__(256) void dt_denoise_prepare_kernel(const float* colour, const float* A, const float* N,
                                                                 const float* Z, int64_t n_px, int demodulate,
                                                                 Rec* nz, Rec* ar, Rec* e)
{
  post::prepare_all<false>(colour, nullptr, A, N, Z, n_px, demodulate, nz, ar, e);
}

// one a-trous level (dt_atrous.h level_rows); the records: N|Z, A|rz, E|flag
__global__ __launch_bounds__(256) void dt_denoise_level_kernel(const Rec* __restrict__ nz, const Rec* __restrict__ ar,
                                                               const Rec* __restrict__ ein, Rec* __restrict__ eout,
                                                               const float* __restrict__ colour, float* __restrict__ out,
                                                               post::Level<false> L)
{
  post::level_rows<false>(nz, ar, ein, eout, colour, out, L);
}

constexpr post::Fail dn_fail{"dt_denoise"};

// the first argument check that fails, or null
const char* dn_check_params(const dt_denoise_params* p)
{
  if (p->levels < 1 || p->levels > 6) return "levels outside 1..6";
  if (p->demodulate != 0 && p->demodulate != 1) return "demodulate must be 0 or 1";
  if (!post::sigma_ok(p->sigma_normal)) return "sigma_normal must be > 0";
  if (!post::sigma_ok(p->sigma_depth)) return "sigma_depth must be > 0";
  if (!post::sigma_ok(p->sigma_colour)) return "sigma_colour must be > 0";
  if (!post::sigma_ok(p->sigma_albedo)) return "sigma_albedo must be > 0";
  return nullptr;
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
  return post::atrous_work_floats((int64_t)xRes * yRes);
}

int dt_denoise(int32_t xRes, int32_t yRes, const float* colour, const dt_features* feat, const dt_denoise_params* p,
               float* out, float* work, int32_t on_device, void* stream, float* kernel_ms)
{
  if (!colour) return dn_fail("null colour");
  if (!feat) return dn_fail("null feat");
  if (!p) return dn_fail("null params");
  if (!out) return dn_fail("null out");
  if (!work) return dn_fail("null work");
  if (const std::string m = post::planes_missing(feat, "feat"); !m.empty()) return dn_fail(m);
  if (xRes < 1) return dn_fail("xRes < 1");
  if (yRes < 1) return dn_fail("yRes < 1");
  if (const char* bad = dn_check_params(p)) return dn_fail(bad);
  const int64_t n_px = (int64_t)xRes * yRes;
  if (post::overlap(out, 3 * n_px, colour, 3 * n_px)) return dn_fail("out aliases colour");
  if (post::overlap(out, 3 * n_px, work, post::atrous_work_floats(n_px))) return dn_fail("out aliases work");
  return post::atrous<false>(dn_fail.who, dt_denoise_prepare_kernel, dt_denoise_level_kernel, xRes, yRes, colour, nullptr,
                             feat, p, out, work, on_device, stream, kernel_ms);
}

}  // extern "C"
