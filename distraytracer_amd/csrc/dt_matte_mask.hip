// dt_matte_mask -- the matte of a set of groups from the ranked layers of dt_render_mattes: per pixel the f32
// sum, from 0.0f, in layer order, of the weights of the layers whose id is in the set. No reference
// counterpart. The specification is the comment block of dt_matte_mask in include/dt.h; tests/mattes_ref.py
// restates it in numpy, and the host loop, the kernel and that restatement agree bit for bit: the pixel is
// one function (mm_pixel) of plain f32 additions that the host loop and the kernel both call.
//
// A translation unit of its own, compiled once for both libraries: dt_kernels.hip's objects stay as they are.
// The error prefix, the 1-D grid and the (untimed) launch are dt_post.h's.
#include "dt_post.h"

namespace {

#define MM_MAX_GROUPS 64

struct MmArgs {   // by value: the set travels with the launch
  int64_t n_pixels;
  int32_t layers, n_groups;
  const int32_t* id;
  const float* weight;
  float* mask;
  int32_t groups[MM_MAX_GROUPS];
};

__host__ __device__ __forceinline__ void mm_pixel(const MmArgs& a, int64_t q)
{
  float m = 0.0f;
  for (int j = 0; j < a.layers; ++j) {
    const int32_t g = a.id[a.layers * q + j];
    bool in = false;
    for (int k = 0; k < a.n_groups; ++k) in = in || g == a.groups[k];   // (entries are >= 0: -1 never matches)
    if (in) m = m + a.weight[a.layers * q + j];
  }
  a.mask[q] = m;
}

__global__ __launch_bounds__(256) void dt_matte_mask_kernel(MmArgs a)
{
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < a.n_pixels; q += (int64_t)gridDim.x * 256) mm_pixel(a, q);
}

constexpr post::Fail mm_fail{"dt_matte_mask"};

}  // namespace

extern "C" int dt_matte_mask(int64_t n_pixels, int32_t layers, const int32_t* id, const float* weight,
                             const int32_t* groups, int32_t n_groups, float* mask, int32_t on_device, void* stream)
{
  if (!id) return mm_fail("null id");
  if (!weight) return mm_fail("null weight");
  if (!groups) return mm_fail("null groups");
  if (!mask) return mm_fail("null mask");
  if (n_pixels < 0) return mm_fail("n_pixels < 0");
  if (layers < 1 || layers > DT_MATTE_MAX_LAYERS)
    return mm_fail("layers " + std::to_string(layers) + " outside 1.." + std::to_string(DT_MATTE_MAX_LAYERS));
  if (n_groups < 1 || n_groups > MM_MAX_GROUPS)
    return mm_fail("n_groups " + std::to_string(n_groups) + " outside 1.." + std::to_string(MM_MAX_GROUPS));
  MmArgs a;
  a.n_pixels = n_pixels;
  a.layers = layers;
  a.n_groups = n_groups;
  a.id = id;
  a.weight = weight;
  a.mask = mask;
  for (int k = 0; k < MM_MAX_GROUPS; ++k) a.groups[k] = -2;
  for (int k = 0; k < n_groups; ++k) {
    if (groups[k] < 0) return mm_fail("groups[" + std::to_string(k) + "] is negative");
    a.groups[k] = groups[k];
  }
  if (n_pixels == 0) return DT_OK;
  if (!on_device) {
    for (int64_t q = 0; q < n_pixels; ++q) mm_pixel(a, q);
    return DT_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  return post::launch(st, nullptr, mm_fail.who, [&] {   // untimed: nothing waits
    hipLaunchKernelGGL(dt_matte_mask_kernel, post::linear_grid(n_pixels, 65536), dim3(256), 0, st, a);
    return hipGetLastError();
  });
}
