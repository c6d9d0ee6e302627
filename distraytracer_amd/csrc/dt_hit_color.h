// dt_hit_color.h — a hit's base colour, for the auxiliary units that report one; never the trace kernel.
#pragma once
#include "dt_device.h"

// What dt_features_kernel takes from run_pass (dt_rayq_kernel, dt_rayq_multi_kernel, dt_features_path_kernel,
// dt_rayq_path_kernel and dt_points_irr_kernel too), as copies for those units only: with run_pass calling
// these helpers, some trace builds' objects came out as other bytes (the room builds with hit_color,
// every build with texel_color), and the product kernels' objects are to stay byte-identical.
// hit_color: the colour the reference's intersect() leaves in the hit shape (a Checkerboard's square,
// ccol), else the shape's own.
__device__ __forceinline__ V3 hit_color(GP g, const DMat& M, int ccol)
{
  return ccol >= 0 ? G3(g, ccol) : v3a(M.color);
}

// texel_color: the texel at (tu, tv) / 255, the light loop's lookup (float products, truncation, the
// index clamped to the texture).
__device__ __forceinline__ V3 texel_color(const DScene& S, const DMat& M, double tu, double tv)
{
  double dims0 = M.tex_w;
  int x_tex = (int)((float)(M.tex_w - 1) * (float)tu);
  int y_tex = (int)((float)(M.tex_h - 1) * (float)tv);
  int uv_ind = (int)(y_tex * dims0 + x_tex);
  if (uv_ind < 0) uv_ind = 0;
  if (uv_ind >= M.tex_w * M.tex_h) uv_ind = M.tex_w * M.tex_h - 1;
  const uint8_t* px = S.tex + M.tex_off + (int64_t)uv_ind * M.tex_ch;
  return v3(px[0] / 255.0, px[1] / 255.0, px[2] / 255.0);
}
