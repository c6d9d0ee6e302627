// dtrender — host CLI mirroring the reference's `./render` modes (render_final_project.cpp:
// 1386-1956) on top of the C-ABI: builds the scene with the host builders, renders on the
// current MI355X through libdt's HIP kernels, writes the PPM. The models and ./ads assets are
// absent: use_model is off, and the tunnel's ad frames are the procedural stand-ins
// of host_scenes.cpp.
//
//   dtrender                 default: 980x540, antialias 2, frame 30 -> buildFinal(240) (1410-1424)
//   dtrender final <n>       1920x1080, antialias 10, depth 10, buildFinal(n*8) (1446-1456)
//   dtrender frame <n>       400x300 preview, aperture 0, 1 spp, no reflection (1428-1444)
//   dtrender nodistr <n>     antialias 6 (1457-1469)
//   dtrender perlin <i>      renderImageCloud 640x480 (1685-1698)
//   dtrender spheres         buildSceneSpheres(0) 256x256 (config C1)
//   dtrender prismcyl <n>    BuildScenePrismCylinder(n) 640x480 (1711-1723)
// options (after the mode): --out FILE(.ppm|.png)  --spp N  --depth N  --res WxH  --seed S
//   --progressive N   render in sample windows of N 64-sample chunks (dt_render_window) onto an f64
//                     accumulator on the device; after every window the output file is overwritten
//                     with the resolved preview (the mean of the samples so far) and samples_done/spp
//                     is printed. The final file is byte-identical to the run without the flag.
//   --adaptive TOL    adaptive sampling (dt_render_window_adaptive): one-chunk windows in which pixels
//                     whose mean has a standard error of at most TOL grey levels stop. --min-samples N:
//                     no pixel stops with fewer (default 64). --counts FILE: samples taken / spp per
//                     pixel as a grey PNG. Prints the share of pixels * spp that was taken.
//   --features PREFIX after the frame, the first-hit feature buffers of all spp samples (dt_render_features)
//                     as 8-bit PNGs: PREFIX.albedo.png (albedo*255), PREFIX.normal.png ((normal*0.5 +
//                     0.5*coverage)*255), PREFIX.depth.png (depth / the frame's largest depth, grey) and
//                     PREFIX.coverage.png (grey), each clamped to 0..255. The frame file is the same bytes
//                     as without the flag.
//   --mattes PREFIX   after the frame, the object mattes of all spp samples (dt_render_mattes; --matte-layers K,
//                     1..8, default 4) as PREFIX.matte.png: a false-colour image, each group a hashed colour,
//                     the layers blended by weight. Groups: one per material signature, as
//                     distraytracer_amd.shape_groups(desc, "material"). The frame file is the same bytes as
//                     without the flag.
//   --denoise         also write the denoised frame (dt_denoise with the default parameters on the frame
//                     and the albedo, normal and depth planes of the samples taken, on the device) to
//                     <stem>.denoised.<ext> beside the frame; with --progressive or --adaptive that file is
//                     overwritten after every window as well. --denoise-levels N: a-trous levels (1..6,
//                     default 5). The frame file is the same bytes as without the flag.
//   --denoise-variance  as --denoise, with the variance-guided filter: dt_variance of the adaptive sampler's
//                     sums, then dt_denoise_var with the default parameters (--denoise-levels applies).
//                     Needs --adaptive: a usage error and exit status 2 without it, before any rendering.
//   --upsample S      also a mixed-resolution preview (S = 2, 3 or 4; the resolution must divide): the frame
//                     rendered once more at 1/S of the resolution in each axis, the albedo, normal and depth
//                     planes at both resolutions, and dt_upsample with the default parameters on the device,
//                     written to <stem>.upsampled.<ext> beside the frame at the full resolution. The frame
//                     file is the same bytes as without the flag.
//   --occlusion PREFIX  after the frame, the occlusion feature buffers of all spp samples (dt_render_occlusion)
//                     as grey 8-bit PNGs, value*255: PREFIX.ao.png (--ao-rays K probes per hitting sample,
//                     0..16, default 4; --ao-radius R world units, default 1.0) and PREFIX.light<j>.png for
//                     the j-th light of --occlusion-lights 0,1,... (indices into the scene's lights, at most 8;
//                     default none). The frame file is the same bytes as without the flag.
//   --bake-occlusion SHAPE  after the frame, a lightmap of shape SHAPE of the scene (a rectangle, checkerboard or
//                     triangle; dt_points_occlusion): --bake-size WxH texels, texel (u, v) centred at
//                     A + ((u+0.5)/W)*(B-A) + ((v+0.5)/H)*(D-A) (a triangle: C-A, texels outside it stay 0), the
//                     normal normalized(cross(B-A, D-A)), as distraytracer_amd.shape_texels; --bake-samples N
//                     samples per texel (default 16) of --ao-rays / --ao-radius / --occlusion-lights probes,
//                     written as --bake-out P: P.ao.png and P.light<j>.png, W x H, row v, grey value*255 as
//                     --occlusion. Without the flag every byte written is the same as before.
//   --bake-through-glass N  with --bake-occlusion: the probes pass through glass (dt_points_occlusion_glass,
//                     max_panes = N in 0..8): P.ao.png and P.light<j>.png by that rule, and P.ao_panes.png and
//                     P.light_panes<j>.png, the pane planes, grey value/8*255 (8 panes are white). Without the flag
//                     every byte written is the same as before.
//   --bake-light SHAPE  after the frame, a lightmap of light on shape SHAPE (dt_points_irradiance) over the texels of
//                     --bake-occlusion (--bake-size WxH, --bake-out P, --bake-samples N): the cosine-weighted
//                     direct light of the lights of --occlusion-lights 0,1,... (needed) as P.direct.png and, with
//                     --bake-gather K (1..16 gather probes per sample, default 0), one diffuse bounce as
//                     P.indirect.png and the share of probes that left the scene as P.sky.png; RGB clamped to
//                     0..1, times 255. Without the flag every byte written and printed is the same as before.
//   --bake-visible SHAPE_A,SHAPE_B  after the frame, how much of SHAPE_B each texel of SHAPE_A sees
//                     (dt_points_visibility): sources are the --bake-size WxH texels of SHAPE_A, targets the
//                     --bake-target-size WxH texels of SHAPE_B (both as --bake-occlusion's), skip_b = SHAPE_B; written
//                     as --bake-out P: P.visible.png, W x H, row v, grey (count_a / targets) * 255. Without the flag
//                     every byte written and printed is the same as before.
//   --peel K          after the frame, depth peeling of the frame's own view (K = 1..8 layers; --peel-out P is
//                     needed; --peel-samples N rays per pixel, 1..1024, default 1): dt_camera_rays, then
//                     dt_trace_rays_multi(K), then one dt_rays_resolve per rank, written as P.layer<j>.png: layer
//                     j's coverage-premultiplied albedo times 255 (the mean over the pixel's rays of the
//                     (j+1)-th surface's albedo, a ray with fewer surfaces adding nothing), as
//                     distraytracer_amd.peel_layers. Without the flag every byte written is the same as before.
//   --pick X,Y        after the frame, what pixel (X, Y) shows (X from the left, Y from the top), mirrors and glass
//                     followed (--pick-bounces K, 0..8, default 4): sample 0's camera ray of the pixel
//                     (dt_camera_rays) through dt_trace_rays_path, printed one line per segment (k, the shape it
//                     hit, its material, the point), then the end (void, miss, surface, cut) and the path's
//                     length L. Without the flag every byte written and printed is the same as before.
//   --guide-bounces K the feature buffers of --features, --denoise, --denoise-variance and --upsample are the
//                     specular-path ones (dt_render_features_path, K = 1..8 perfect specular bounces): the
//                     guides describe what mirrors and glass show, not the reflector. Without it (or with 0)
//                     every byte written is the same as before.
//   --nogloss         glossy reflectors render as perfect mirrors (dt_globals.nogloss = 1, the reference's
//                     switch): the steel doors, the floor and the checker cylinder of `final` then bounce guides
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/dt.h"

static int die(const char* what, int rc)
{
  fprintf(stderr, "%s failed (%d): %s\n", what, rc, dt_last_error());
  return 1;
}

// --guide-bounces K: the guides of every consumer below are dt_render_features_path's
static int guide_bounces = 0;
static int render_guides(const dt_scene* s, const dt_globals& g, int frame, int n_samples, const dt_features* f,
                         int on_device, dt_stats* st)
{
  if (guide_bounces > 0)
    return dt_render_features_path(s, &g, frame, nullptr, n_samples, guide_bounces, f, nullptr, on_device, nullptr, st);
  return dt_render_features(s, &g, frame, nullptr, n_samples, f, on_device, nullptr, st);
}

// the adaptive sampler's device buffers (--denoise-variance filters by them; all null: --denoise)
struct adaptive_sums {
  const double *acc, *acc2;
  const uint32_t* cnt;
};

// --denoise: `img` (host, the frame or a preview of the first n_samples samples of every pixel) and the
// feature planes of those samples through dt_denoise on the device, written to `fn`; with sums, through
// dt_variance and dt_denoise_var
static int write_denoised(const dt_scene* s, const dt_globals& g, int frame, int n_samples, int levels,
                          const std::vector<float>& img, const std::string& fn, bool png,
                          const adaptive_sums* sums = nullptr)
{
  const size_t n_px = (size_t)g.xRes * g.yRes;
  dt_denoise_params dp;
  dt_denoise_params_default(&dp);
  if (levels > 0) dp.levels = levels;
  dt_denoise_var_params vp;
  dt_denoise_var_params_default(&vp);
  if (levels > 0) vp.levels = levels;
  const int64_t n_work = sums ? dt_denoise_var_workspace_floats(g.xRes, g.yRes, &vp) + 3 * (int64_t)n_px
                              : dt_denoise_workspace_floats(g.xRes, g.yRes, &dp);
  if (n_work < 0) return die("dt_denoise_workspace_floats", (int)n_work);
  // colour, albedo, normal (3 per pixel), depth (1), out (3), then (the variance plane, 3, and) the workspace
  float* d = nullptr;
  if (hipMalloc((void**)&d, (13 * n_px + (size_t)n_work) * sizeof(float)) != hipSuccess ||
      hipMemset(d, 0, 13 * n_px * sizeof(float)) != hipSuccess ||
      hipMemcpy(d, img.data(), 3 * n_px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    fprintf(stderr, "denoise buffers: hipMalloc failed\n");
    return 1;
  }
  dt_features f;
  memset(&f, 0, sizeof f);
  f.albedo = d + 3 * n_px; f.normal = d + 6 * n_px; f.depth = d + 9 * n_px;
  float* out = d + 10 * n_px;
  int rc = render_guides(s, g, frame, n_samples, &f, 1, nullptr);
  if (rc) return die("dt_render_features", rc);
  if (sums) {
    float* var = d + 13 * n_px;
    rc = dt_variance(&g, nullptr, sums->acc, sums->acc2, sums->cnt, var, 1, nullptr);
    if (rc) return die("dt_variance", rc);
    rc = dt_denoise_var(g.xRes, g.yRes, d, var, &f, &vp, out, d + 16 * n_px, 1, nullptr, nullptr);
    if (rc) return die("dt_denoise_var", rc);
  } else {
    rc = dt_denoise(g.xRes, g.yRes, d, &f, &dp, out, d + 13 * n_px, 1, nullptr, nullptr);
    if (rc) return die("dt_denoise", rc);
  }
  std::vector<float> clean(3 * n_px);
  if (hipMemcpy(clean.data(), out, 3 * n_px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
    fprintf(stderr, "denoise: hipMemcpy failed\n");
    return 1;
  }
  (void)hipFree(d);
  rc = png ? dt_write_png(fn.c_str(), g.xRes, g.yRes, clean.data()) : dt_write_ppm(fn.c_str(), g.xRes, g.yRes, clean.data());
  if (rc) return die("dt_write_ppm/png (denoised)", rc);
  return 0;
}

// --upsample: the frame of g at 1/factor of the resolution (a scene of its own: the primary-ray lists are
// per resolution), the guides of both resolutions (the full-resolution ones from `s`) and dt_upsample on
// the device, written to `fn`
static int write_upsampled(const dt_scene_desc* desc, const dt_scene* s, const dt_globals& g, int frame, int n_samples,
                           int factor, const std::string& fn, bool png)
{
  dt_upsample_params up;
  dt_upsample_params_default(&up);
  up.factor = factor;
  dt_globals lo = g;
  lo.xRes = g.xRes / factor;
  lo.yRes = g.yRes / factor;
  const size_t n_hi = (size_t)g.xRes * g.yRes, n_lo = (size_t)lo.xRes * lo.yRes;
  // colour, albedo, normal (3 per pixel), depth (1) at the low resolution; albedo, normal, depth, out at the full one
  float* d = nullptr;
  if (hipMalloc((void**)&d, 10 * (n_lo + n_hi) * sizeof(float)) != hipSuccess ||
      hipMemset(d, 0, 10 * (n_lo + n_hi) * sizeof(float)) != hipSuccess) {
    fprintf(stderr, "upsample buffers: hipMalloc failed\n");
    return 1;
  }
  dt_features fl, fh;
  memset(&fl, 0, sizeof fl);
  memset(&fh, 0, sizeof fh);
  fl.albedo = d + 3 * n_lo; fl.normal = d + 6 * n_lo; fl.depth = d + 9 * n_lo;
  float* hi = d + 10 * n_lo;
  fh.albedo = hi; fh.normal = hi + 3 * n_hi; fh.depth = hi + 6 * n_hi;
  float* out = hi + 7 * n_hi;
  dt_scene* sl = nullptr;
  int rc = dt_scene_create(desc, &lo, &sl);
  if (rc) return die("dt_scene_create (low resolution)", rc);
  dt_stats st;
  rc = dt_render(sl, &lo, frame, nullptr, d, 1, nullptr, &st);
  if (rc) return die("dt_render (low resolution)", rc);
  rc = render_guides(sl, lo, frame, n_samples, &fl, 1, nullptr);
  if (rc) return die("dt_render_features (low resolution)", rc);
  dt_scene_destroy(sl);
  rc = render_guides(s, g, frame, n_samples, &fh, 1, nullptr);
  if (rc) return die("dt_render_features", rc);
  float ms = 0.0f;
  rc = dt_upsample(g.xRes, g.yRes, d, &fl, &fh, &up, out, 1, nullptr, &ms);
  if (rc) return die("dt_upsample", rc);
  std::vector<float> img(3 * n_hi);
  if (hipMemcpy(img.data(), out, 3 * n_hi * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
    fprintf(stderr, "upsample: hipMemcpy failed\n");
    return 1;
  }
  (void)hipFree(d);
  rc = png ? dt_write_png(fn.c_str(), g.xRes, g.yRes, img.data()) : dt_write_ppm(fn.c_str(), g.xRes, g.yRes, img.data());
  if (rc) return die("dt_write_ppm/png (upsampled)", rc);
  printf("upsampled: %dx%d traced in %.2f ms, dt_upsample x%d in %.3f ms (kernel) -> %s\n", lo.xRes, lo.yRes, st.kernel_ms,
         factor, ms, fn.c_str());
  return 0;
}

// --ao-rays, --ao-radius and --occlusion-lights as dt_occlusion_params (--occlusion, --bake-occlusion)
static bool occlusion_params(int ao_rays, double ao_radius, const std::string& lights, dt_occlusion_params& op)
{
  dt_occlusion_params_default(&op);
  op.ao_rays = ao_rays;
  for (const char* c = lights.c_str(); *c;) {
    char* end = nullptr;
    const long l = strtol(c, &end, 10);
    if (end == c || op.n_lights >= DT_OCCL_MAX_LIGHTS) {
      fprintf(stderr, "usage: --occlusion-lights takes at most %d comma-separated light indices\n", DT_OCCL_MAX_LIGHTS);
      return false;
    }
    op.lights[op.n_lights++] = (int32_t)l;
    c = *end == ',' ? end + 1 : end;
  }
  if (ao_radius >= 0.0) op.ao_radius = (float)ao_radius;
  return true;
}

// the grey PNGs of occlusion planes of w x h entries: prefix.ao.png (when ao) and prefix.light<j>.png, value*255
// panes: the pane planes of --bake-through-glass instead, prefix.ao_panes.png and prefix.light_panes<j>.png, value/8*255
static int write_occlusion_pngs(const std::string& prefix, int w, int h, const float* ao, const float* light, int n_lights,
                                bool panes = false)
{
  const size_t n_px = (size_t)w * h;
  std::vector<float> pix(3 * n_px);
  const std::string tag = panes ? "_panes" : "";
  for (int plane = ao ? -1 : 0; plane < n_lights; ++plane) {
    for (size_t q = 0; q < n_px; ++q) {
      const float x = plane < 0 ? ao[q] : light[(size_t)n_lights * q + plane];
      const float v = panes ? (x / 8.0f) * 255.0f : x * 255.0f;
      pix[3 * q] = pix[3 * q + 1] = pix[3 * q + 2] = v;
    }
    const std::string pf =
        prefix + (plane < 0 ? ".ao" + tag : ".light" + tag + std::to_string(plane)) + ".png";
    const int rc = dt_write_png(pf.c_str(), w, h, pix.data());
    if (rc) return rc;
  }
  return 0;
}

// The texel centres of a w x h lightmap over a rectangle, checkerboard or triangle and their normal, each operation
// one rounded f64 one (distraytracer_amd.shape_texels computes the same bits): 3 doubles per kept texel in pts and
// nrms, its index v*w + u in keep (a triangle keeps the texels whose centre lies inside it). false: no area.
static bool bake_texels(const dt_shape_desc& sh, int w, int h, std::vector<double>& pts, std::vector<double>& nrms,
                        std::vector<size_t>& keep)
{
  const bool tri = sh.type == DT_SHAPE_TRIANGLE;
  double e1[3], e2[3], nrm[3];
  for (int k = 0; k < 3; ++k) { e1[k] = sh.v[1][k] - sh.v[0][k]; e2[k] = sh.v[tri ? 2 : 3][k] - sh.v[0][k]; }
  nrm[0] = e1[1] * e2[2] - e1[2] * e2[1];
  nrm[1] = e1[2] * e2[0] - e1[0] * e2[2];
  nrm[2] = e1[0] * e2[1] - e1[1] * e2[0];
  const double len = sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
  if (!(std::isfinite(len) && len > 0)) return false;
  for (int v = 0; v < h; ++v)
    for (int u = 0; u < w; ++u) {
      const double a = ((double)u + 0.5) / (double)w, b = ((double)v + 0.5) / (double)h;
      if (tri && !(a + b <= 1.0)) continue;
      keep.push_back((size_t)v * w + u);
      for (int k = 0; k < 3; ++k) {
        pts.push_back((sh.v[0][k] + a * e1[k]) + b * e2[k]);
        nrms.push_back(1.0 * (nrm[k] / len));
      }
    }
  return true;
}

int main(int argc, char** argv)
{
  dt_globals g;
  dt_globals_default(&g);
  g.use_model = 0;   // ./models absent (F6)
  std::string mode = argc > 1 ? argv[1] : "";
  int arg = (argc > 2 && argv[2][0] != '-') ? atoi(argv[2]) : 0;
  std::string out;
  std::string data_dir = DT_DATA_DIR;
  int spp = -1, depth = -1, W = -1, H = -1, progressive = 0, min_samples = 64, denoise = 0, denoise_levels = 0, denoise_variance = 0, upsample = 0;
  double adaptive = -1.0;
  std::string counts_file, features_prefix, mattes_prefix;
  int matte_layers = 4, nogloss = 0;
  std::string occl_prefix, occl_lights;
  int ao_rays = 4;
  double ao_radius = -1.0;   // < 0: dt_occlusion_params_default's
  int bake_shape = -1, bake_w = 0, bake_h = 0, bake_samples = 16, bake_glass = -1;
  std::string bake_prefix;
  bool bake_asked = false;
  int light_shape = -1, bake_gather = 0;
  bool light_asked = false;
  int vis_a = -1, vis_b = -1, vis_tw = 0, vis_th = 0;
  bool vis_asked = false;
  int peel = 0, peel_samples = 1;
  bool peel_asked = false;
  std::string peel_prefix;
  int pick_x = -1, pick_y = -1, pick_bounces = 4;
  bool pick_asked = false, pick_given = false;
  for (int i = 2; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "--out" && i + 1 < argc) out = argv[++i];
    else if (a == "--spp" && i + 1 < argc) spp = atoi(argv[++i]);
    else if (a == "--depth" && i + 1 < argc) depth = atoi(argv[++i]);
    else if (a == "--seed" && i + 1 < argc) g.seed = (uint32_t)strtoul(argv[++i], nullptr, 10);
    else if (a == "--data" && i + 1 < argc) data_dir = argv[++i];
    else if (a == "--res" && i + 1 < argc) sscanf(argv[++i], "%dx%d", &W, &H);
    else if (a == "--progressive" && i + 1 < argc) progressive = atoi(argv[++i]);
    else if (a == "--adaptive" && i + 1 < argc) adaptive = atof(argv[++i]);
    else if (a == "--min-samples" && i + 1 < argc) min_samples = atoi(argv[++i]);
    else if (a == "--counts" && i + 1 < argc) counts_file = argv[++i];
    else if (a == "--features" && i + 1 < argc) features_prefix = argv[++i];
    else if (a == "--mattes" && i + 1 < argc) mattes_prefix = argv[++i];
    else if (a == "--matte-layers" && i + 1 < argc) matte_layers = atoi(argv[++i]);
    else if (a == "--denoise") denoise = 1;
    else if (a == "--denoise-variance") denoise_variance = 1;
    else if (a == "--denoise-levels" && i + 1 < argc) denoise_levels = atoi(argv[++i]);
    else if (a == "--upsample" && i + 1 < argc) upsample = atoi(argv[++i]);
    else if (a == "--guide-bounces" && i + 1 < argc) guide_bounces = atoi(argv[++i]);
    else if (a == "--nogloss") nogloss = 1;
    else if (a == "--occlusion" && i + 1 < argc) occl_prefix = argv[++i];
    else if (a == "--ao-rays" && i + 1 < argc) ao_rays = atoi(argv[++i]);
    else if (a == "--ao-radius" && i + 1 < argc) ao_radius = atof(argv[++i]);
    else if (a == "--occlusion-lights" && i + 1 < argc) occl_lights = argv[++i];
    else if (a == "--bake-occlusion" && i + 1 < argc) { bake_shape = atoi(argv[++i]); bake_asked = true; }
    else if (a == "--bake-light" && i + 1 < argc) { light_shape = atoi(argv[++i]); light_asked = true; }
    else if (a == "--bake-gather" && i + 1 < argc) bake_gather = atoi(argv[++i]);
    else if (a == "--bake-visible" && i + 1 < argc) { sscanf(argv[++i], "%d,%d", &vis_a, &vis_b); vis_asked = true; }
    else if (a == "--bake-target-size" && i + 1 < argc) sscanf(argv[++i], "%dx%d", &vis_tw, &vis_th);
    else if (a == "--bake-size" && i + 1 < argc) sscanf(argv[++i], "%dx%d", &bake_w, &bake_h);
    else if (a == "--bake-out" && i + 1 < argc) bake_prefix = argv[++i];
    else if (a == "--bake-samples" && i + 1 < argc) bake_samples = atoi(argv[++i]);
    else if (a == "--bake-through-glass" && i + 1 < argc) {
      bake_glass = atoi(argv[++i]);
      if (bake_glass < 0 || bake_glass > DT_TRANSMIT_MAX_PANES) {
        fprintf(stderr, "usage: --bake-through-glass N: N in 0..%d\n", DT_TRANSMIT_MAX_PANES);
        return 2;
      }
    }
    else if (a == "--peel" && i + 1 < argc) { peel = atoi(argv[++i]); peel_asked = true; }
    else if (a == "--peel-out" && i + 1 < argc) peel_prefix = argv[++i];
    else if (a == "--peel-samples" && i + 1 < argc) peel_samples = atoi(argv[++i]);
    else if (a == "--pick" && i + 1 < argc) { pick_asked = sscanf(argv[++i], "%d,%d", &pick_x, &pick_y) == 2; pick_given = true; }
    else if (a == "--pick-bounces" && i + 1 < argc) pick_bounces = atoi(argv[++i]);
  }
  if (pick_given && (!pick_asked || pick_bounces < 0 || pick_bounces > DT_RAY_PATH_MAX_BOUNCES)) {
    fprintf(stderr, "usage: --pick X,Y [--pick-bounces K] needs a pixel and K in 0..%d\n", DT_RAY_PATH_MAX_BOUNCES);
    return 2;
  }
  if (pick_given && mode == "perlin") {
    fprintf(stderr, "usage: --pick needs a mode that renders a scene (perlin has none)\n");
    return 2;
  }
  if (guide_bounces < 0 || guide_bounces > DT_GUIDE_MAX_BOUNCES) {
    fprintf(stderr, "usage: --guide-bounces K needs K in 0..%d\n", DT_GUIDE_MAX_BOUNCES);
    return 2;
  }
  if (bake_asked && (bake_shape < 0 || bake_w < 1 || bake_h < 1 || bake_prefix.empty())) {
    fprintf(stderr, "usage: --bake-occlusion SHAPE (>= 0) needs --bake-size WxH and --bake-out PREFIX\n");
    return 2;
  }
  if (light_asked && (light_shape < 0 || bake_w < 1 || bake_h < 1 || bake_prefix.empty() || occl_lights.empty() ||
                      bake_gather < 0 || bake_gather > DT_OCCL_MAX_AO_RAYS)) {
    fprintf(stderr, "usage: --bake-light SHAPE (>= 0) needs --bake-size WxH, --bake-out PREFIX, --occlusion-lights and "
                    "--bake-gather in 0..%d\n", DT_OCCL_MAX_AO_RAYS);
    return 2;
  }
  if (vis_asked && (vis_a < 0 || vis_b < 0 || bake_w < 1 || bake_h < 1 || vis_tw < 1 || vis_th < 1 || bake_prefix.empty())) {
    fprintf(stderr, "usage: --bake-visible SHAPE_A,SHAPE_B (>= 0) needs --bake-size WxH, --bake-target-size WxH and "
                    "--bake-out PREFIX\n");
    return 2;
  }
  if (peel_asked && (peel < 1 || peel > DT_MULTIHIT_MAX || peel_prefix.empty() || peel_samples < 1 ||
                     peel_samples > DT_CAMERA_RAYS_MAX_SAMPLES)) {
    fprintf(stderr, "usage: --peel K needs K in 1..%d, --peel-out PREFIX and --peel-samples in 1..%d\n", DT_MULTIHIT_MAX,
            DT_CAMERA_RAYS_MAX_SAMPLES);
    return 2;
  }
  if (denoise_variance && adaptive < 0.0) {
    fprintf(stderr, "usage: --denoise-variance needs --adaptive TOL (the variance comes from the adaptive sampler's sums)\n");
    return 2;
  }
  if (denoise_variance) denoise = 1;
  std::string scene = "final";
  float build_frame = 0;
  int frame = 0;
  char buf[256];
  if (mode.empty()) {
    g.xRes = 980; g.yRes = 540; g.antialias_samples = 2; g.brdf_samples = 2;
    frame = 30 * 8; build_frame = (float)frame;
    snprintf(buf, sizeof buf, "./frame.%04d.ppm", 30);
  } else if (mode == "final") {
    frame = arg * 8; build_frame = (float)frame;
    snprintf(buf, sizeof buf, "./final_frames/frame.%04d.ppm", arg);
  } else if (mode == "frame") {
    g.xRes = 400; g.yRes = 300; g.aperture = 0; g.antialias_samples = 1; g.reflect = 0;
    frame = arg * 8; build_frame = (float)frame;
    snprintf(buf, sizeof buf, "./preview_frames/frame.%04d.ppm", arg);
  } else if (mode == "nodistr") {
    g.antialias_samples = 6; g.brdf_samples = 2;
    frame = arg * 8; build_frame = (float)frame;
    snprintf(buf, sizeof buf, "./nodistr/frame.%04d.ppm", arg);
  } else if (mode == "perlin") {
    g.xRes = 640; g.yRes = 480; g.aperture = 0; g.antialias_samples = 1;
    snprintf(buf, sizeof buf, "./test_frames/perlin/frame.%04d.ppm", arg);
    if (W > 0) { g.xRes = W; g.yRes = H; }
    std::vector<float> img((size_t)3 * g.xRes * g.yRes, 0.0f);
    dt_stats st;
    int rc = dt_render_sky(&g, (float)arg, nullptr, img.data(), 0, nullptr, &st);
    if (rc) return die("dt_render_sky", rc);
    std::string fn = out.empty() ? std::string(buf) : out;
    rc = dt_write_ppm(fn.c_str(), g.xRes, g.yRes, img.data());
    if (rc) return die("dt_write_ppm", rc);
    printf("Finished perlin cloud frame %d in %.3f ms (kernel) -> %s\n", arg, st.kernel_ms, fn.c_str());
    return 0;
  } else if (mode == "spheres") {
    scene = "spheres";
    snprintf(buf, sizeof buf, "./spheres.ppm");
  } else if (mode == "prismcyl") {
    scene = "prismcyl";
    g.xRes = 640; g.yRes = 480;
    frame = arg; build_frame = (float)arg;
    snprintf(buf, sizeof buf, "./test_frames/prismcyl/frame.%04d.ppm", arg);
  } else {
    fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
  }
  dt_scene_desc* desc = nullptr;
  int rc = dt_build_scene(scene.c_str(), build_frame, &g, data_dir.c_str(), &desc);
  if (rc) return die("dt_build_scene", rc);
  if (scene == "spheres") { g.xRes = 256; g.yRes = 256; g.antialias_samples = 1; g.max_depth = 1; }
  if (spp > 0) g.antialias_samples = spp;
  if (depth > 0) g.max_depth = depth;
  if (nogloss) g.nogloss = 1;
  if (W > 0) { g.xRes = W; g.yRes = H; }
  if (pick_asked && (pick_x < 0 || pick_x >= g.xRes || pick_y < 0 || pick_y >= g.yRes)) {
    fprintf(stderr, "usage: --pick %d,%d: outside the %dx%d frame\n", pick_x, pick_y, g.xRes, g.yRes);
    return 2;
  }
  if (upsample && (upsample < 2 || upsample > 4 || g.xRes % upsample || g.yRes % upsample)) {
    fprintf(stderr, "usage: --upsample S needs S = 2, 3 or 4 and a resolution that S divides (%dx%d)\n", g.xRes, g.yRes);
    return 2;
  }
  if (bake_asked) {
    const int t = bake_shape < desc->n_shapes ? desc->shapes[bake_shape].type : 0;
    if (t != DT_SHAPE_RECTANGLE && t != DT_SHAPE_CHECKERBOARD && t != DT_SHAPE_TRIANGLE) {
      fprintf(stderr, "usage: --bake-occlusion %d: a rectangle, checkerboard or triangle of the scene's %d shapes is needed\n",
              bake_shape, desc->n_shapes);
      return 2;
    }
  }
  if (light_asked) {
    const int t = light_shape < desc->n_shapes ? desc->shapes[light_shape].type : 0;
    if (t != DT_SHAPE_RECTANGLE && t != DT_SHAPE_CHECKERBOARD && t != DT_SHAPE_TRIANGLE) {
      fprintf(stderr, "usage: --bake-light %d: a rectangle, checkerboard or triangle of the scene's %d shapes is needed\n",
              light_shape, desc->n_shapes);
      return 2;
    }
  }
  if (vis_asked)
    for (const int shape : {vis_a, vis_b}) {
      const int t = shape < desc->n_shapes ? desc->shapes[shape].type : 0;
      if (t != DT_SHAPE_RECTANGLE && t != DT_SHAPE_CHECKERBOARD && t != DT_SHAPE_TRIANGLE) {
        fprintf(stderr, "usage: --bake-visible %d: a rectangle, checkerboard or triangle of the scene's %d shapes is needed\n",
                shape, desc->n_shapes);
        return 2;
      }
    }
  dt_scene* s = nullptr;
  rc = dt_scene_create(desc, &g, &s);
  if (rc) return die("dt_scene_create", rc);
  std::vector<float> img((size_t)3 * g.xRes * g.yRes, 0.0f);
  dt_stats st;
  std::string fn = out.empty() ? std::string(buf) : out;
  const bool png = fn.size() > 4 && fn.compare(fn.size() - 4, 4, ".png") == 0;
  // <stem>.denoised.<ext> beside the frame
  const size_t slash = fn.find_last_of('/'), dot = fn.find_last_of('.');
  const bool has_ext = dot != std::string::npos && dot > (slash == std::string::npos ? 0 : slash + 1);
  const std::string dn_fn = has_ext ? fn.substr(0, dot) + ".denoised" + fn.substr(dot) : fn + ".denoised";
  const std::string up_fn = has_ext ? fn.substr(0, dot) + ".upsampled" + fn.substr(dot) : fn + ".upsampled";
  int samples_taken = (int)sqrt((double)g.antialias_samples);
  samples_taken *= samples_taken;
  if (adaptive >= 0.0) {
    // one-chunk windows over the live, unconverged pixels until a window traces none or all samples
    // are rendered; every pixel resolved with its own count
    const int n = (int)sqrt((double)g.antialias_samples), total = n * n;
    const int64_t n_acc = dt_accum_doubles(&g, nullptr), n_px = n_acc / 3;
    double *acc = nullptr, *acc2 = nullptr;
    uint32_t* cnt = nullptr;
    float* dimg = nullptr;
    if (hipMalloc((void**)&acc, n_acc * sizeof(double)) != hipSuccess || hipMalloc((void**)&acc2, n_acc * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&cnt, n_px * sizeof(uint32_t)) != hipSuccess || hipMalloc((void**)&dimg, n_acc * sizeof(float)) != hipSuccess ||
        hipMemset(acc, 0, n_acc * sizeof(double)) != hipSuccess || hipMemset(acc2, 0, n_acc * sizeof(double)) != hipSuccess ||
        hipMemset(cnt, 0, n_px * sizeof(uint32_t)) != hipSuccess) {
      fprintf(stderr, "adaptive buffers: hipMalloc failed\n");
      return 1;
    }
    dt_stats sum;
    memset(&sum, 0, sizeof sum);
    for (int begin = 0; begin < total;) {
      const int end = total < 64 || begin + 64 > total ? total : begin + 64;
      rc = dt_render_window_adaptive(s, &g, frame, nullptr, begin, end, acc, acc2, cnt, adaptive, min_samples, nullptr, &st);
      if (rc) return die("dt_render_window_adaptive", rc);
      sum.samples += st.samples;
      sum.kernel_ms += st.kernel_ms;
      printf("%d/%d: %llu pixels\n", end, total, (unsigned long long)st.pixels);
      fflush(stdout);
      begin = end;
      samples_taken = end;
      if (denoise) {
        rc = dt_resolve_adaptive(&g, nullptr, acc, cnt, dimg, 1, nullptr, nullptr);
        if (rc) return die("dt_resolve_adaptive", rc);
        if (hipMemcpy(img.data(), dimg, n_acc * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
          fprintf(stderr, "preview: hipMemcpy failed\n");
          return 1;
        }
        const adaptive_sums sums = {acc, acc2, cnt};
        if (write_denoised(s, g, frame, end, denoise_levels, img, dn_fn, png, denoise_variance ? &sums : nullptr)) return 1;
      }
      if (st.pixels == 0) break;
    }
    rc = dt_resolve_adaptive(&g, nullptr, acc, cnt, dimg, 1, nullptr, nullptr);
    if (rc) return die("dt_resolve_adaptive", rc);
    std::vector<uint32_t> hcnt((size_t)n_px);
    if (hipMemcpy(img.data(), dimg, n_acc * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hcnt.data(), cnt, n_px * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) {
      fprintf(stderr, "adaptive: hipMemcpy failed\n");
      return 1;
    }
    rc = png ? dt_write_png(fn.c_str(), g.xRes, g.yRes, img.data()) : dt_write_ppm(fn.c_str(), g.xRes, g.yRes, img.data());
    if (rc) return die("dt_write_ppm/png", rc);
    if (!counts_file.empty()) {   // count / spp as grey, in the image's pixel order
      std::vector<float> cimg((size_t)n_acc);
      for (int64_t q = 0; q < n_px; ++q)
        for (int k = 0; k < 3; ++k) cimg[3 * q + k] = 255.0f * (float)hcnt[q] / (float)total;
      rc = dt_write_png(counts_file.c_str(), g.xRes, g.yRes, cimg.data());
      if (rc) return die("dt_write_png (counts)", rc);
    }
    printf("adaptive tol %g: %.2f%% of %lld pixels x %d spp taken\n", adaptive,
           100.0 * (double)sum.samples / ((double)n_px * total), (long long)n_px, total);
    (void)hipFree(acc);
    (void)hipFree(acc2);
    (void)hipFree(cnt);
    (void)hipFree(dimg);
    st = sum;
  } else if (progressive > 0) {
    // windows of `progressive` chunks in ascending order onto a zeroed accumulator; every window's
    // preview (dt_resolve with the samples so far) overwrites the file, the last one is the frame
    const int n = (int)sqrt((double)g.antialias_samples), total = n * n;
    const int64_t n_acc = dt_accum_doubles(&g, nullptr);
    double* acc = nullptr;
    float* dimg = nullptr;
    if (hipMalloc((void**)&acc, n_acc * sizeof(double)) != hipSuccess || hipMalloc((void**)&dimg, n_acc * sizeof(float)) != hipSuccess ||
        hipMemset(acc, 0, n_acc * sizeof(double)) != hipSuccess) {
      fprintf(stderr, "accumulator: hipMalloc failed\n");
      return 1;
    }
    dt_stats sum;
    memset(&sum, 0, sizeof sum);
    for (int begin = 0; begin < total;) {
      const int end = total < 64 || begin + 64 * progressive > total ? total : begin + 64 * progressive;
      rc = dt_render_window(s, &g, frame, nullptr, begin, end, acc, nullptr, &st);
      if (rc) return die("dt_render_window", rc);
      sum.samples += st.samples;
      sum.kernel_ms += st.kernel_ms;
      rc = dt_resolve(&g, nullptr, acc, end, dimg, 1, nullptr, nullptr);
      if (rc) return die("dt_resolve", rc);
      if (hipMemcpy(img.data(), dimg, n_acc * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        fprintf(stderr, "preview: hipMemcpy failed\n");
        return 1;
      }
      rc = png ? dt_write_png(fn.c_str(), g.xRes, g.yRes, img.data()) : dt_write_ppm(fn.c_str(), g.xRes, g.yRes, img.data());
      if (rc) return die("dt_write_ppm/png", rc);
      if (denoise && write_denoised(s, g, frame, end, denoise_levels, img, dn_fn, png)) return 1;
      printf("%d/%d\n", end, total);
      fflush(stdout);
      begin = end;
    }
    (void)hipFree(acc);
    (void)hipFree(dimg);
    st = sum;
  } else {
    rc = dt_render(s, &g, frame, nullptr, img.data(), 0, nullptr, &st);
    if (rc) return die("dt_render", rc);
    rc = png ? dt_write_png(fn.c_str(), g.xRes, g.yRes, img.data()) : dt_write_ppm(fn.c_str(), g.xRes, g.yRes, img.data());
    if (rc) return die("dt_write_ppm/png", rc);
    if (denoise && write_denoised(s, g, frame, samples_taken, denoise_levels, img, dn_fn, png)) return 1;
  }
  if (upsample) {
    const int n = (int)sqrt((double)g.antialias_samples);
    if (int bad = write_upsampled(desc, s, g, frame, n * n, upsample, up_fn, png)) return bad;
  }
  if (!features_prefix.empty()) {
    const int n = (int)sqrt((double)g.antialias_samples);
    const size_t n_px = (size_t)g.xRes * g.yRes;
    std::vector<float> alb(3 * n_px, 0.0f), nrm(3 * n_px, 0.0f), dep(n_px, 0.0f), cov(n_px, 0.0f), pix(3 * n_px);
    dt_features f;
    memset(&f, 0, sizeof f);
    f.albedo = alb.data(); f.normal = nrm.data(); f.depth = dep.data(); f.coverage = cov.data();
    dt_stats fst;
    rc = render_guides(s, g, frame, n * n, &f, 0, &fst);
    if (rc) return die("dt_render_features", rc);
    float dmax = 0.0f;
    for (size_t q = 0; q < n_px; ++q) dmax = dep[q] > dmax ? dep[q] : dmax;
    for (int plane = 0; plane < 4; ++plane) {
      static const char* const names[4] = {"albedo", "normal", "depth", "coverage"};
      for (size_t q = 0; q < n_px; ++q)
        for (int k = 0; k < 3; ++k) {
          float v;
          if (plane == 0) v = alb[3 * q + k] * 255.0f;
          else if (plane == 1) v = (nrm[3 * q + k] * 0.5f + 0.5f * cov[q]) * 255.0f;
          else if (plane == 2) v = (dmax > 0.0f ? dep[q] / dmax : 0.0f) * 255.0f;
          else v = cov[q] * 255.0f;
          pix[3 * q + k] = v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v;   // (the PNG writer truncates to a byte)
        }
      const std::string pf = features_prefix + "." + names[plane] + ".png";
      rc = dt_write_png(pf.c_str(), g.xRes, g.yRes, pix.data());
      if (rc) return die("dt_write_png (features)", rc);
    }
    printf("features: %llu pixels in %.3f ms (kernel) -> %s.{albedo,normal,depth,coverage}.png\n",
           (unsigned long long)fst.pixels, fst.kernel_ms, features_prefix.c_str());
  }
  if (!mattes_prefix.empty()) {
    // one group per material signature, numbered in order of first appearance (shape_groups "material")
    typedef std::tuple<int, int, int, int, unsigned, int, double, double, double> Sig;
    std::map<Sig, int32_t> seen;
    std::vector<int32_t> group_of((size_t)desc->n_shapes);
    for (int i = 0; i < desc->n_shapes; ++i) {
      const dt_shape_desc& sh = desc->shapes[i];
      const Sig sig(sh.type == DT_SHAPE_TRIANGLE && (sh.flags & DT_F_MESH) ? 1 : 0, sh.model, sh.material, sh.emit,
                    sh.flags & (DT_F_LIGHT | DT_F_TEXTURE | DT_F_GLOSSY | DT_F_MESH), sh.tex_frame, sh.color[0],
                    sh.color[1], sh.color[2]);
      group_of[i] = seen.emplace(sig, (int32_t)seen.size()).first->second;
    }
    const int n = (int)sqrt((double)g.antialias_samples);
    const size_t n_px = (size_t)g.xRes * g.yRes;
    const int L = matte_layers;
    std::vector<int32_t> mid(n_px * (size_t)(L > 0 ? L : 1), -1);
    std::vector<float> mw(mid.size(), 0.0f), pix(3 * n_px, 0.0f);
    dt_mattes m;
    memset(&m, 0, sizeof m);
    m.id = mid.data(); m.weight = mw.data();
    dt_stats mst;
    uint64_t over = 0;
    rc = dt_render_mattes(s, &g, frame, nullptr, n * n, group_of.data(), desc->n_shapes, L, &m, 0, nullptr, &mst, &over);
    if (rc) return die("dt_render_mattes", rc);
    for (size_t q = 0; q < n_px; ++q)
      for (int j = 0; j < L; ++j) {
        const int32_t id = mid[L * q + j];
        if (id < 0) continue;
        uint32_t h = (uint32_t)id * 2654435761u + 0x9e3779b9u;   // a colour per group
        h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12;
        for (int k = 0; k < 3; ++k) pix[3 * q + k] += mw[L * q + j] * (float)(64 + ((h >> (8 * k)) & 0xFF) * 3 / 4);
      }
    for (float& v : pix) v = v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v;
    const std::string pf = mattes_prefix + ".matte.png";
    rc = dt_write_png(pf.c_str(), g.xRes, g.yRes, pix.data());
    if (rc) return die("dt_write_png (mattes)", rc);
    printf("mattes: %llu pixels, %d groups, %d layers, %llu overflow pixels in %.3f ms (kernel) -> %s\n",
           (unsigned long long)mst.pixels, (int)seen.size(), L, (unsigned long long)over, mst.kernel_ms, pf.c_str());
  }
  if (!occl_prefix.empty()) {
    dt_occlusion_params op;
    if (!occlusion_params(ao_rays, ao_radius, occl_lights, op)) return 2;
    const int n = (int)sqrt((double)g.antialias_samples);
    const size_t n_px = (size_t)g.xRes * g.yRes;
    std::vector<float> ao(n_px, 0.0f), lv(n_px * (size_t)(op.n_lights > 0 ? op.n_lights : 1), 0.0f);
    dt_occlusion o;
    memset(&o, 0, sizeof o);
    if (op.ao_rays != 0) o.ao = ao.data();
    if (op.n_lights > 0) o.light = lv.data();
    dt_stats ost;
    rc = dt_render_occlusion(s, &g, frame, nullptr, n * n, &op, &o, 0, nullptr, &ost);
    if (rc) return die("dt_render_occlusion", rc);
    rc = write_occlusion_pngs(occl_prefix, g.xRes, g.yRes, o.ao, lv.data(), op.n_lights);
    if (rc) return die("dt_write_png (occlusion)", rc);
    printf("occlusion: %llu pixels, %llu probes (%d ao rays of radius %g, %d lights) in %.3f ms (kernel) -> %s.*.png\n",
           (unsigned long long)ost.pixels, (unsigned long long)ost.shadow_rays, op.ao_rays, (double)op.ao_radius,
           op.n_lights, ost.kernel_ms, occl_prefix.c_str());
  }
  if (bake_shape >= 0) {
    dt_occlusion_params op;
    if (!occlusion_params(ao_rays, ao_radius, occl_lights, op)) return 2;
    const size_t n_tex = (size_t)bake_w * bake_h;
    std::vector<double> pts, nrms;
    std::vector<size_t> keep;   // texel v*W + u of every point
    if (!bake_texels(desc->shapes[bake_shape], bake_w, bake_h, pts, nrms, keep)) {
      fprintf(stderr, "usage: --bake-occlusion: shape %d has no area\n", bake_shape);
      return 2;
    }
    const int nl = op.n_lights;
    std::vector<float> pao(keep.size() + 1, 0.0f), plv(keep.size() * (size_t)(nl > 0 ? nl : 1) + 1, 0.0f);
    dt_occlusion o;
    memset(&o, 0, sizeof o);
    if (op.ao_rays != 0) o.ao = pao.data();
    if (nl > 0) o.light = plv.data();
    dt_stats bst;
    std::vector<float> ppao, pplv;   // --bake-through-glass: the pane planes
    if (bake_glass >= 0) {
      ppao.assign(pao.size(), 0.0f);
      pplv.assign(plv.size(), 0.0f);
      dt_occlusion_panes pn;
      memset(&pn, 0, sizeof pn);
      if (o.ao) pn.ao_panes = ppao.data();
      if (o.light) pn.light_panes = pplv.data();
      rc = dt_points_occlusion_glass(s, &g, frame, (int64_t)keep.size(), pts.data(), nrms.data(), bake_samples, &op,
                                     bake_glass, &o, &pn, 0, nullptr, &bst);
      if (rc) return die("dt_points_occlusion_glass", rc);
    } else {
      rc = dt_points_occlusion(s, &g, frame, (int64_t)keep.size(), pts.data(), nrms.data(), bake_samples, &op, &o, 0,
                               nullptr, &bst);
      if (rc) return die("dt_points_occlusion", rc);
    }
    std::vector<float> ao(n_tex, 0.0f), lv(n_tex * (size_t)(nl > 0 ? nl : 1), 0.0f);
    for (size_t i = 0; i < keep.size(); ++i) {
      ao[keep[i]] = pao[i];
      for (int j = 0; j < nl; ++j) lv[(size_t)nl * keep[i] + j] = plv[(size_t)nl * i + j];
    }
    rc = write_occlusion_pngs(bake_prefix, bake_w, bake_h, o.ao ? ao.data() : nullptr, lv.data(), nl);
    if (rc) return die("dt_write_png (bake)", rc);
    if (bake_glass >= 0) {
      std::fill(ao.begin(), ao.end(), 0.0f);
      std::fill(lv.begin(), lv.end(), 0.0f);
      for (size_t i = 0; i < keep.size(); ++i) {
        ao[keep[i]] = ppao[i];
        for (int j = 0; j < nl; ++j) lv[(size_t)nl * keep[i] + j] = pplv[(size_t)nl * i + j];
      }
      rc = write_occlusion_pngs(bake_prefix, bake_w, bake_h, o.ao ? ao.data() : nullptr, lv.data(), nl, true);
      if (rc) return die("dt_write_png (bake panes)", rc);
      printf("bake: probes pass through glass, at most %d panes\n", bake_glass);
    }
    printf("bake: shape %d, %dx%d texels, %llu points, %llu probes (%d samples, %d ao rays of radius %g, %d lights) in "
           "%.3f ms (kernel) -> %s.*.png\n",
           bake_shape, bake_w, bake_h, (unsigned long long)keep.size(), (unsigned long long)bst.shadow_rays, bake_samples,
           op.ao_rays, (double)op.ao_radius, nl, bst.kernel_ms, bake_prefix.c_str());
  }
  if (light_shape >= 0) {
    dt_occlusion_params op;
    if (!occlusion_params(0, -1.0, occl_lights, op)) return 2;
    dt_irradiance_params ip;
    memset(&ip, 0, sizeof ip);
    ip.n_lights = op.n_lights;
    for (int j = 0; j < op.n_lights; ++j) ip.light[j] = op.lights[j];
    ip.gather_rays = bake_gather;
    const size_t n_tex = (size_t)bake_w * bake_h;
    std::vector<double> pts, nrms;
    std::vector<size_t> keep;   // texel v*W + u of every point
    if (!bake_texels(desc->shapes[light_shape], bake_w, bake_h, pts, nrms, keep)) {
      fprintf(stderr, "usage: --bake-light: shape %d has no area\n", light_shape);
      return 2;
    }
    std::vector<float> pd(3 * keep.size() + 1, 0.0f), pi(3 * keep.size() + 1, 0.0f), ps(keep.size() + 1, 0.0f);
    dt_irradiance o;
    memset(&o, 0, sizeof o);
    o.direct_rgb = pd.data();
    if (bake_gather > 0) { o.indirect_rgb = pi.data(); o.sky = ps.data(); }
    dt_stats bst;
    rc = dt_points_irradiance(s, &g, frame, (int64_t)keep.size(), pts.data(), nrms.data(), bake_samples, &ip, &o, 0,
                              nullptr, &bst);
    if (rc) return die("dt_points_irradiance", rc);
    // RGB clamped to 0..1, times 255 (distraytracer_amd.irradiance_images restates it)
    const auto byte = [](float v) { return (v < 0.0f ? 0.0f : v > 1.0f ? 1.0f : v) * 255.0f; };
    std::vector<float> pix(3 * n_tex);
    const char* names[3] = {".direct.png", ".indirect.png", ".sky.png"};
    for (int plane = 0; plane < (bake_gather > 0 ? 3 : 1); ++plane) {
      std::fill(pix.begin(), pix.end(), 0.0f);
      for (size_t i = 0; i < keep.size(); ++i)
        for (int k = 0; k < 3; ++k)
          pix[3 * keep[i] + k] = byte(plane == 0 ? pd[3 * i + k] : plane == 1 ? pi[3 * i + k] : ps[i]);
      rc = dt_write_png((bake_prefix + names[plane]).c_str(), bake_w, bake_h, pix.data());
      if (rc) return die("dt_write_png (bake light)", rc);
    }
    printf("bake light: shape %d, %dx%d texels, %llu points, %llu shadow probes, %llu gather probes (%d samples, %d "
           "lights, %d gather rays) in %.3f ms (kernel) -> %s.*.png\n",
           light_shape, bake_w, bake_h, (unsigned long long)keep.size(), (unsigned long long)bst.shadow_rays,
           (unsigned long long)bst.rays, bake_samples, ip.n_lights, bake_gather, bst.kernel_ms, bake_prefix.c_str());
  }
  if (vis_asked) {
    std::vector<double> pa, na, pb, nb;
    std::vector<size_t> keep, keep_b;   // texel v*W + u of every source; of every target
    if (!bake_texels(desc->shapes[vis_a], bake_w, bake_h, pa, na, keep) ||
        !bake_texels(desc->shapes[vis_b], vis_tw, vis_th, pb, nb, keep_b)) {
      fprintf(stderr, "usage: --bake-visible: a shape has no area\n");
      return 2;
    }
    const std::vector<int32_t> skip(keep_b.size(), vis_b);   // the target shape hides none of its own texels
    std::vector<int32_t> seen(keep.size() + 1, 0);
    dt_visibility_params vp;
    dt_visibility_params_default(&vp);
    vp.skip_b = skip.data();
    dt_visibility o;
    memset(&o, 0, sizeof o);
    o.count_a = seen.data();
    dt_stats bst;
    rc = dt_points_visibility(s, &g, (int64_t)keep.size(), pa.data(), (int64_t)keep_b.size(), pb.data(), &vp, &o, 0,
                              nullptr, &bst);
    if (rc) return die("dt_points_visibility", rc);
    // the share of the targets seen, as float32, times 255 (distraytracer_amd.bake_visibility's `visible` image)
    std::vector<float> pix(3 * (size_t)bake_w * bake_h, 0.0f);
    for (size_t i = 0; i < keep.size(); ++i)
      for (int k = 0; k < 3; ++k) pix[3 * keep[i] + k] = (float)((double)seen[i] / (double)keep_b.size()) * 255.0f;
    rc = dt_write_png((bake_prefix + ".visible.png").c_str(), bake_w, bake_h, pix.data());
    if (rc) return die("dt_write_png (bake visible)", rc);
    printf("bake visible: shape %d, %dx%d texels, %llu sources against %llu targets of shape %d (%dx%d), %llu pairs traced "
           "in %.3f ms (kernel) -> %s.visible.png\n",
           vis_a, bake_w, bake_h, (unsigned long long)keep.size(), (unsigned long long)keep_b.size(), vis_b, vis_tw, vis_th,
           (unsigned long long)bst.shadow_rays, bst.kernel_ms, bake_prefix.c_str());
  }
  if (peel_asked) {
    const int K = peel, n = peel_samples;
    const int64_t rows = dt_camera_rays_rows(&g, nullptr, 0, n);
    if (rows < 0) return die("dt_camera_rays_rows", (int)rows);
    const size_t n_px = (size_t)g.xRes * g.yRes;
    std::vector<double> start((size_t)rows * 3, 0.0), dir((size_t)rows * 3, 0.0), alb((size_t)rows * K * 3, 0.0);
    std::vector<int32_t> shp((size_t)rows * K, -1);
    float cam_ms = 0;
    rc = dt_camera_rays(&g, frame, nullptr, 0, n, start.data(), dir.data(), 0, nullptr, &cam_ms);
    if (rc) return die("dt_camera_rays", rc);
    dt_ray_multihits mh;
    memset(&mh, 0, sizeof mh);
    mh.shape = shp.data(); mh.albedo = alb.data();
    dt_stats pst;
    rc = dt_trace_rays_multi(s, &g, rows, start.data(), dir.data(), K, &mh, 0, nullptr, &pst);
    if (rc) return die("dt_trace_rays_multi", rc);
    std::vector<double> aj((size_t)rows * 3);
    std::vector<int32_t> sj((size_t)rows);
    std::vector<float> plane(3 * n_px), pix(3 * n_px);
    for (int j = 0; j < K; ++j) {
      for (int64_t r = 0; r < rows; ++r) {
        sj[(size_t)r] = shp[(size_t)(r * K + j)];
        for (int k = 0; k < 3; ++k) aj[(size_t)(3 * r + k)] = alb[(size_t)(3 * (r * K + j) + k)];
      }
      rc = dt_rays_resolve(&g, nullptr, n, 3, aj.data(), sj.data(), DT_RESOLVE_MEAN, plane.data(), nullptr, 0, nullptr);
      if (rc) return die("dt_rays_resolve", rc);
      for (size_t e = 0; e < 3 * n_px; ++e) {
        const float v = plane[e] * 255.0f;
        pix[e] = v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v;   // (the PNG writer truncates to a byte)
      }
      const std::string pf = peel_prefix + ".layer" + std::to_string(j) + ".png";
      rc = dt_write_png(pf.c_str(), g.xRes, g.yRes, pix.data());
      if (rc) return die("dt_write_png (peel)", rc);
    }
    printf("peel: %lld rays (%d per pixel), %d layers: rays %.3f ms, hits %.3f ms (kernels) -> %s.layer<j>.png\n",
           (long long)rows, n, K, cam_ms, pst.kernel_ms, peel_prefix.c_str());
  }
  if (pick_asked) {
    const int64_t rows = dt_camera_rays_rows(&g, nullptr, 0, 1);
    if (rows < 0) return die("dt_camera_rays_rows", (int)rows);
    std::vector<double> start((size_t)rows * 3, 0.0), dir((size_t)rows * 3, 0.0);
    rc = dt_camera_rays(&g, frame, nullptr, 0, 1, start.data(), dir.data(), 0, nullptr, nullptr);
    if (rc) return die("dt_camera_rays", rc);
    const size_t q = (size_t)pick_y * g.xRes + pick_x;   // the pixel's slot: row 0 is the top row of the image
    const int K = pick_bounces;
    int32_t end = 0, segments = 0, seg_shape[DT_RAY_PATH_MAX_BOUNCES + 1];
    double length = 0, seg_point[3 * (DT_RAY_PATH_MAX_BOUNCES + 1)];
    dt_ray_paths rp;
    memset(&rp, 0, sizeof rp);
    rp.end = &end; rp.segments = &segments; rp.length = &length; rp.seg_shape = seg_shape; rp.seg_point = seg_point;
    rc = dt_trace_rays_path(s, &g, 1, &start[3 * q], &dir[3 * q], K, &rp, 0, nullptr, nullptr);
    if (rc) return die("dt_trace_rays_path", rc);
    for (int k = 0; k < segments; ++k) {
      const int h = seg_shape[k];
      if (h < 0) printf("pick %d,%d: segment %d shape -1 material -1 (no hit)\n", pick_x, pick_y, k);
      else printf("pick %d,%d: segment %d shape %d material %d point %.9g %.9g %.9g\n", pick_x, pick_y, k, h,
                  desc->shapes[h].material, seg_point[3 * k], seg_point[3 * k + 1], seg_point[3 * k + 2]);
    }
    static const char* const ends[4] = {"void", "miss", "surface", "cut"};
    if (end < DT_PATH_VOID || end > DT_PATH_CUT) {
      fprintf(stderr, "dt_trace_rays_path returned the end code %d\n", end);
      return 1;
    }
    printf("pick %d,%d: end %s L %.9g\n", pick_x, pick_y, ends[end], length);
  }
  double msps = st.samples / (st.kernel_ms * 1e-3) / 1e6;
  printf("Rendered %s frame %d: %dx%d, %d spp, depth %d in %.2f ms (kernel, %.1f Mpixel-samples/s) -> %s\n",
         scene.c_str(), frame, g.xRes, g.yRes, (int)st.samples / (g.xRes * g.yRes), g.max_depth, st.kernel_ms,
         msps, fn.c_str());
  dt_scene_destroy(s);
  dt_scene_desc_free(desc);
  return 0;
}
