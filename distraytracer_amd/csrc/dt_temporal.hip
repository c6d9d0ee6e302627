// dt_camera_get and dt_reproject — temporal reuse for animation previews: every pixel's first hit is
// reprojected into the previous frame's camera, the history found there (four bilinear taps, each checked
// against the previous frame's depth, normal, albedo and shape planes) is blended with the current preview, and
// the blend becomes the next frame's history (the temporal accumulation of SVGF, Schied et al. 2017).
// No reference counterpart. The specification is the comment block of dt_reproject in include/dt.h;
// tests/temporal_ref.py restates it in numpy, and the host loop, the kernel and that restatement agree bit
// for bit: every operation is one rounded IEEE f32 operation (no contraction, correctly rounded division
// and square root), and the whole pixel, taps included, is one function (tp_pixel) that the host loop and
// the kernel both call.
//
// A translation unit of its own (dt_kernels.hip and dt_api.cpp stay as they are). The demodulation
// divisor, the overlap test, the row grid and the timed launch are dt_post.h's; the projection's
// arithmetic (tp_dot, tp_pixel) is used here alone and stays here.
#include "dt_post.h"

namespace dth {
int camera_record(const dt_globals& g, dt_camera& out, std::string& err);   // host_flatten.cpp
}

namespace {

#define TP_HD __host__ __device__ __forceinline__

// a camera in f32: the record's doubles converted once, on the host
struct TpCam {
  float eye[3], X[3], Y[3], Z[3];
  float l, r, b, t, near_plane;
};

struct TpArgs {
  int32_t W, H, demodulate, has_prev;
  float alpha_min, max_history, depth_tol, nt2, at2;
  TpCam cur, prev;
  const float *C, *Vc, *A, *N, *Z;   // the current frame (Vc, shape: may be null)
  const int32_t* shape;
  const float *pA, *pN, *pZ;         // the previous frame's guides (pshape: may be null)
  const int32_t* pshape;
  const float *hc, *hv, *hl;         // the history read
  float *out, *out_var, *oc, *ov, *ol;   // out, out_var and the history written
};

TP_HD float tp_dot(const float* u, const float* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

TP_HD int tp_clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// One pixel, steps 1-9 of include/dt.h: x the column, r the buffer row (render row y = H-1-r). The four
// taps are loaded from addresses clamped into the image whatever the projection gave, and a select keeps
// the sums of a tap that is not valid: no load depends on a lane's own condition. The only branches
// around loads are on has_prev and on the optional planes, the same for every pixel of a call.
TP_HD void tp_pixel(const TpArgs& a, int x, int r)
{
  const int W = a.W, H = a.H;
  const int y = H - 1 - r;
  const int64_t q = (int64_t)r * W + x;
  const bool has_var = a.Vc != nullptr;
  float c[3], d[3], e_p[3], vc[3], ve[3], n_p[3], a_p[3];
  for (int k = 0; k < 3; ++k) {
    c[k] = a.C[3 * q + k];
    a_p[k] = a.A[3 * q + k];
    d[k] = post::demod(a_p[k], a.demodulate);
    e_p[k] = c[k] / d[k];
    vc[k] = has_var ? a.Vc[3 * q + k] : 0.0f;
    ve[k] = vc[k] / (d[k] * d[k]);
    n_p[k] = a.N[3 * q + k];
  }
  const bool nan = c[0] != c[0] || c[1] != c[1] || c[2] != c[2];
  float s[3] = {0.0f, 0.0f, 0.0f}, sv[3] = {0.0f, 0.0f, 0.0f}, sl = 0.0f, wt = 0.0f;
  if (a.has_prev) {
    const TpCam& cc = a.cur;
    const TpCam& pc = a.prev;
    const float fa = cc.l + ((cc.r - cc.l) * (float)x) / (float)W;
    const float fb = cc.b + ((cc.t - cc.b) * (float)y) / (float)H;
    float dir[3], v[3];
    for (int k = 0; k < 3; ++k) dir[k] = (fa * cc.X[k] + fb * cc.Y[k]) - cc.near_plane * cc.Z[k];
    const float z = a.Z[q];
    const bool surf = z > 0.0f;
    const float sc = z / sqrtf(tp_dot(dir, dir));
    for (int k = 0; k < 3; ++k) {
      const float pw = cc.eye[k] + sc * dir[k];
      v[k] = surf ? pw - pc.eye[k] : dir[k];
    }
    const float dq = sqrtf(tp_dot(v, v));
    const float zc = -tp_dot(v, pc.Z);
    const float pa = (pc.near_plane * tp_dot(v, pc.X)) / zc;
    const float pb = (pc.near_plane * tp_dot(v, pc.Y)) / zc;
    const float fx = ((pa - pc.l) * (float)W) / (pc.r - pc.l);
    const float fy = ((pb - pc.b) * (float)H) / (pc.t - pc.b);
    const bool sought = zc > 0.0f && -1.0f < fx && fx < (float)W && -1.0f < fy && fy < (float)H;
    const float fxs = sought ? fx : 0.0f, fys = sought ? fy : 0.0f;   // in range before the conversion
    const float x0 = floorf(fxs), y0 = floorf(fys);
    const float tx = fxs - x0, ty = fys - y0;
    const int ix = (int)x0, iy = (int)y0;
    const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
    const float dtol = a.depth_tol * dq;
    const int32_t sh_p = (a.shape && a.pshape) ? a.shape[q] : 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float w = wx[i] * wy[j];
        const int u = ix + i, t = iy + j;
        const bool inside = u >= 0 && u < W && t >= 0 && t < H;
        const int64_t qt = (int64_t)(H - 1 - tp_clampi(t, H - 1)) * W + tp_clampi(u, W - 1);
        const float hl = a.hl[qt];
        const float h0 = a.hc[3 * qt], h1 = a.hc[3 * qt + 1], h2 = a.hc[3 * qt + 2];
        const float zt = a.pZ[qt];
        const float dn[3] = {n_p[0] - a.pN[3 * qt], n_p[1] - a.pN[3 * qt + 1], n_p[2] - a.pN[3 * qt + 2]};
        const float da[3] = {a_p[0] - a.pA[3 * qt], a_p[1] - a.pA[3 * qt + 1], a_p[2] - a.pA[3 * qt + 2]};
        const bool depth_ok = surf ? fabsf(zt - dq) <= dtol : zt == 0.0f;
        const bool normal_ok = tp_dot(dn, dn) <= a.nt2;
        const bool albedo_ok = tp_dot(da, da) <= a.at2;
        const bool shape_ok = (a.shape && a.pshape) ? a.pshape[qt] == sh_p : true;
        const bool valid = sought && inside && w > 0.0f && hl > 0.0f && h0 == h0 && h1 == h1 && h2 == h2 &&
                           depth_ok && normal_ok && albedo_ok && shape_ok;
        wt = valid ? wt + w : wt;
        s[0] = valid ? s[0] + w * h0 : s[0];
        s[1] = valid ? s[1] + w * h1 : s[1];
        s[2] = valid ? s[2] + w * h2 : s[2];
        sl = valid ? sl + w * hl : sl;
        if (has_var)
          for (int k = 0; k < 3; ++k) sv[k] = valid ? sv[k] + w * a.hv[3 * qt + k] : sv[k];
      }
    }
  }
  const bool blend = wt > 0.0f && !nan;
  const float n = fminf(sl / wt + 1.0f, a.max_history);
  const float alpha = fmaxf(a.alpha_min, 1.0f / n);
  const float om = 1.0f - alpha;
  for (int k = 0; k < 3; ++k) {
    const float e_h = s[k] / wt;
    const float e_o = e_h + alpha * (e_p[k] - e_h);
    a.oc[3 * q + k] = blend ? e_o : e_p[k];
    a.out[3 * q + k] = blend ? fminf(fmaxf(e_o * d[k], 0.0f), 255.0f) : c[k];
    if (has_var) {
      const float v_o = (om * om) * (sv[k] / wt) + (alpha * alpha) * ve[k];
      a.ov[3 * q + k] = blend ? v_o : ve[k];
      a.out_var[3 * q + k] = blend ? v_o * (d[k] * d[k]) : vc[k];
    }
  }
  a.ol[q] = blend ? n : nan ? 0.0f : 1.0f;
}

// One thread per pixel. Block (64, 4): a wave is 64 consecutive x of one buffer row, so the current
// frame's loads and every store coalesce, and the four taps are a coherent gather: neighbouring lanes
// project onto neighbouring pixels of the previous frame. Lanes past the row's end leave at once (there
// is no wave-level operation below).
__global__ __launch_bounds__(256) void dt_reproject_kernel(TpArgs a)
{
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= a.W) return;
  for (int r = blockIdx.y * 4 + threadIdx.y; r < a.H; r += gridDim.y * 4) tp_pixel(a, x, r);
}

constexpr post::Fail tp_fail{"dt_reproject"};

TpCam tp_cam(const dt_camera* c)
{
  TpCam o;
  for (int k = 0; k < 3; ++k) {
    o.eye[k] = (float)c->eye[k];
    o.X[k] = (float)c->X[k];
    o.Y[k] = (float)c->Y[k];
    o.Z[k] = (float)c->Z[k];
  }
  o.l = c->l;
  o.r = c->r;
  o.b = c->b;
  o.t = c->t;
  o.near_plane = c->near_plane;
  return o;
}

struct TpPlane {
  const char* name;
  const void* p;
  int64_t floats;   // 4-byte elements
};

bool tp_overlap(const TpPlane& a, const TpPlane& b) { return post::overlap(a.p, a.floats, b.p, b.floats); }

}  // namespace

extern "C" {

int dt_camera_get(const dt_globals* g, dt_camera* out)
{
  if (!g || !out) {
    dth::set_error("dt_camera_get: null argument");
    return DT_E_INVALID;
  }
  std::string err;
  const int rc = dth::camera_record(*g, *out, err);
  if (rc != DT_OK) dth::set_error("dt_camera_get: " + err);
  return rc;
}

void dt_temporal_params_default(dt_temporal_params* p)
{
  if (!p) return;
  p->demodulate = 1;
  // chosen on the sweep of tools/temporal_bench.py
  p->alpha_min = 0.05f;
  p->max_history = 32.0f;
  p->depth_tol = 0.02f;
  p->normal_tol = 0.25f;
  p->albedo_tol = 0.0625f;
}

int dt_reproject(const dt_camera* cur, const float* colour, const float* variance, const dt_features* feat,
                 const dt_camera* prev, const dt_features* prev_feat, const dt_history* hist_in,
                 const dt_temporal_params* p, float* out, float* out_var, const dt_history* hist_out,
                 int32_t on_device, void* stream, float* kernel_ms)
{
  if (!cur) return tp_fail("null cur");
  if (!colour) return tp_fail("null colour");
  if (!feat) return tp_fail("null feat");
  if (!p) return tp_fail("null params");
  if (!out) return tp_fail("null out");
  if (!hist_out) return tp_fail("null hist_out");
  if (const std::string m = post::planes_missing(feat, "feat"); !m.empty()) return tp_fail(m);
  const bool has_prev = prev || prev_feat || hist_in;
  if (has_prev) {
    if (!prev) return tp_fail("null prev with a history");
    if (!prev_feat) return tp_fail("null prev_feat with a history");
    if (!hist_in) return tp_fail("null hist_in with a previous frame");
    if (const std::string m = post::planes_missing(prev_feat, "prev_feat"); !m.empty()) return tp_fail(m);
    if (!hist_in->colour) return tp_fail("hist_in->colour missing");
    if (!hist_in->len) return tp_fail("hist_in->len missing");
    if (variance && !hist_in->var) return tp_fail("hist_in->var missing (variance is given)");
    if (!variance && hist_in->var) return tp_fail("hist_in->var given without variance");
  }
  if (!hist_out->colour) return tp_fail("hist_out->colour missing");
  if (!hist_out->len) return tp_fail("hist_out->len missing");
  if (variance && !hist_out->var) return tp_fail("hist_out->var missing (variance is given)");
  if (!variance && hist_out->var) return tp_fail("hist_out->var given without variance");
  if (variance && !out_var) return tp_fail("null out_var (variance is given)");
  if (!variance && out_var) return tp_fail("out_var given without variance");
  if (cur->xRes < 1) return tp_fail("cur: xRes < 1");
  if (cur->yRes < 1) return tp_fail("cur: yRes < 1");
  if (has_prev && (prev->xRes != cur->xRes || prev->yRes != cur->yRes)) return tp_fail("prev: a camera of another size than cur");
  if (p->demodulate != 0 && p->demodulate != 1) return tp_fail("demodulate must be 0 or 1");
  if (!(p->alpha_min > 0.0f && p->alpha_min <= 1.0f)) return tp_fail("alpha_min outside (0, 1]");
  if (!(p->max_history >= 1.0f)) return tp_fail("max_history must be >= 1");
  if (!(p->depth_tol >= 0.0f)) return tp_fail("depth_tol must be >= 0");
  if (!(p->normal_tol >= 0.0f)) return tp_fail("normal_tol must be >= 0");
  if (!(p->albedo_tol >= 0.0f)) return tp_fail("albedo_tol must be >= 0");
  const int32_t W = cur->xRes, H = cur->yRes;
  const int64_t n_px = (int64_t)W * H;
  const TpPlane outs[] = {{"out", out, 3 * n_px},
                          {"out_var", out_var, 3 * n_px},
                          {"hist_out->colour", hist_out->colour, 3 * n_px},
                          {"hist_out->var", hist_out->var, 3 * n_px},
                          {"hist_out->len", hist_out->len, n_px}};
  const TpPlane ins[] = {{"colour", colour, 3 * n_px},
                         {"variance", variance, 3 * n_px},
                         {"feat->albedo", feat->albedo, 3 * n_px},
                         {"feat->normal", feat->normal, 3 * n_px},
                         {"feat->depth", feat->depth, n_px},
                         {"feat->shape", feat->shape, n_px},
                         {"prev_feat->albedo", has_prev ? prev_feat->albedo : nullptr, 3 * n_px},
                         {"prev_feat->normal", has_prev ? prev_feat->normal : nullptr, 3 * n_px},
                         {"prev_feat->depth", has_prev ? prev_feat->depth : nullptr, n_px},
                         {"prev_feat->shape", has_prev ? prev_feat->shape : nullptr, n_px},
                         {"hist_in->colour", has_prev ? hist_in->colour : nullptr, 3 * n_px},
                         {"hist_in->var", has_prev ? hist_in->var : nullptr, 3 * n_px},
                         {"hist_in->len", has_prev ? hist_in->len : nullptr, n_px}};
  for (size_t i = 0; i < sizeof(outs) / sizeof(outs[0]); ++i) {
    if (!outs[i].p) continue;
    for (const TpPlane& in : ins)
      if (in.p && tp_overlap(outs[i], in)) return tp_fail(std::string(outs[i].name) + " aliases " + in.name);
    for (size_t j = 0; j < i; ++j)
      if (outs[j].p && tp_overlap(outs[i], outs[j])) return tp_fail(std::string(outs[i].name) + " aliases " + outs[j].name);
  }
  TpArgs a;
  a.W = W;
  a.H = H;
  a.demodulate = p->demodulate;
  a.has_prev = has_prev ? 1 : 0;
  a.alpha_min = p->alpha_min;
  a.max_history = p->max_history;
  a.depth_tol = p->depth_tol;
  a.nt2 = p->normal_tol * p->normal_tol;
  a.at2 = p->albedo_tol * p->albedo_tol;
  a.cur = tp_cam(cur);
  a.prev = tp_cam(has_prev ? prev : cur);
  a.C = colour;
  a.Vc = variance;
  a.A = feat->albedo;
  a.N = feat->normal;
  a.Z = feat->depth;
  a.shape = feat->shape;
  a.pA = has_prev ? prev_feat->albedo : nullptr;
  a.pN = has_prev ? prev_feat->normal : nullptr;
  a.pZ = has_prev ? prev_feat->depth : nullptr;
  a.pshape = has_prev ? prev_feat->shape : nullptr;
  a.hc = has_prev ? hist_in->colour : nullptr;
  a.hv = has_prev ? hist_in->var : nullptr;
  a.hl = has_prev ? hist_in->len : nullptr;
  a.out = out;
  a.out_var = out_var;
  a.oc = hist_out->colour;
  a.ov = hist_out->var;
  a.ol = hist_out->len;
  if (!on_device) {
    for (int r = 0; r < H; ++r)
      for (int x = 0; x < W; ++x) tp_pixel(a, x, r);
    if (kernel_ms) *kernel_ms = 0.0f;
    return DT_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  return post::launch(st, kernel_ms, tp_fail.who, [&] {
    hipLaunchKernelGGL(dt_reproject_kernel, post::row_grid(W, H), dim3(64, 4), 0, st, a);
    return hipGetLastError();
  });
}

}  // extern "C"
