"""distraytracer_amd — MI355X-native (gfx950) render loop of distraytracer.

Python mirror of the reference's host interface over the C-ABI (include/dt.h):

    reference (render_final_project.cpp / scene.h)      here
    renderImage(filename, frame, sceneBuilder)  :965    renderImage(filename, frame, builder, g)
    renderImageCloud(filename, frame)           :1224   renderImageCloud(filename, frame, g)
    buildFinal / buildSceneSpheres / ...  (scene.h)     build_scene("final" | "spheres" | ...)
    globals (:48-137)                                   Globals / globals_default()
    writePPM (helpers.h:174)                            write_ppm

Everything computes through libdt.so's HIP kernels; a missing library or a missing GPU is
an error (there is no CPU path in this package).
"""
import ctypes

from ._lib import (DATA_DIR, DT_KERNEL_AUTO, DT_KERNEL_DONATE, DT_KERNEL_PRODUCT, DT_OUT_IMAGE, DT_OUT_SLAB, AccelInfo, BVHNode, Camera, DenoiseParams, DenoiseVarParams, DTError, Globals, SceneDesc,
                   DT_PATH_CUT, DT_PATH_MISS, DT_PATH_SURFACE, DT_PATH_VOID,
                   SHAPE_TYPES, OcclusionParams, RayOrderParams, DT_RAY_ORDER_TILE, Stats, TemporalParams, Tiles, UpsampleParams, check, lib)

__all__ = ["Globals", "Tiles", "Stats", "DTError", "globals_default", "build_scene", "Scene",
           "render", "render_sky", "renderImage", "renderImageCloud", "write_ppm", "DATA_DIR",
           "DT_OUT_IMAGE", "DT_OUT_SLAB", "slab_floats", "slab_floats_max", "unpack_slabs", "tiles", "check", "lib",
           "accel_info", "DT_KERNEL_AUTO", "DT_KERNEL_PRODUCT", "DT_KERNEL_DONATE",
           "accum_doubles", "window_check", "render_window", "render_window_async", "resolve", "Progressive",
           "mean_abs_change", "adapt_converged", "render_window_adaptive", "resolve_adaptive", "adapt_select_ms",
           "AdaptiveProgressive", "render_features", "feature_images", "FEATURE_PLANES",
           "DenoiseParams", "denoise_params_default", "denoise", "denoised_filename",
           "DenoiseVarParams", "denoise_var_params_default", "variance",
           "Camera", "camera", "TemporalParams", "temporal_params_default", "reproject", "TemporalAccumulator",
           "trace_rays", "rays_occluded", "RAY_PLANES",
           "trace_rays_multi", "segment_through_glass", "RAY_MULTI_PLANES",
           "rays_transmittance", "RAY_TRANSMIT_PLANES",
           "trace_rays_path", "ray_polyline", "pick", "RAY_PATH_PLANES",
           "DT_PATH_VOID", "DT_PATH_MISS", "DT_PATH_SURFACE", "DT_PATH_CUT",
           "camera_rays", "camera_rays_rows", "rays_resolve", "peel_layers", "RESOLVE_MODES",
           "RayOrderParams", "RayOrder", "ray_order_params_default", "ray_order_key", "ray_order", "DT_RAY_ORDER_TILE",
           "render_mattes", "matte_mask", "shape_groups", "MATTE_PLANES",
           "UpsampleParams", "upsample_params_default", "upsample", "low_res_globals",
           "OcclusionParams", "occlusion_params_default", "render_occlusion", "occlusion_ao_ray", "occlusion_light_ray",
           "occlusion_images", "points_occlusion", "shape_texels", "bake_occlusion",
           "points_irradiance", "irradiance_gather_ray", "irradiance_cosine", "bake_irradiance", "irradiance_images",
           "IRRADIANCE_PLANES",
           "points_visibility", "visibility_matrix", "bake_visibility", "VISIBILITY_PLANES"]


def globals_default():
    """Fresh-process globals (render_final_project.cpp:48-137)."""
    g = Globals()
    lib.dt_globals_default(ctypes.byref(g))
    return g


def tiles(x0=0, y0=0, x1=0, y1=0, tile_w=32, tile_h=32, rank=0, world=1, layout=DT_OUT_IMAGE):
    return Tiles(x0, y0, x1, y1, tile_w, tile_h, rank, world, layout, 0)


class BuiltScene:
    """A dt_scene_desc owned by libdt (dt_build_scene)."""

    def __init__(self, ptr):
        self._ptr = ptr

    @property
    def desc(self):
        return self._ptr.contents

    def __del__(self):
        if getattr(self, "_ptr", None) and lib is not None:   # lib is None at interpreter exit
            lib.dt_scene_desc_free(self._ptr)
            self._ptr = None


def build_scene(name, frame, g, data_dir=DATA_DIR):
    """scene.h builders; mutates g as the reference builder mutates its globals."""
    out = ctypes.POINTER(SceneDesc)()
    check(lib.dt_build_scene(name.encode(), float(frame), ctypes.byref(g), data_dir.encode(), ctypes.byref(out)),
          "dt_build_scene(%s)" % name)
    return BuiltScene(out)


def accel_info(built, g):
    """The acceleration structures dt_scene_create would upload (trees, shadow grid), built on the
    host only: counts and content hashes (dt_accel_info_build). Build knobs are read from the
    environment (DT_SG_BLOCK, DT_SG_ORDER, DT_FAST_TREE, ...) at call time."""
    info = AccelInfo()
    desc = built._ptr if isinstance(built, BuiltScene) else ctypes.pointer(built)
    check(lib.dt_accel_info_build(desc, ctypes.byref(g), ctypes.byref(info)), "dt_accel_info_build")
    return info.as_dict()


def trace_build(built, g, frame):
    """The trace-kernel build dt_render launches for (built, g) at `frame` (automatic choice, host
    only, dt_trace_build): (kernel name, the scene's feature mask, the build's feature mask)."""
    name = ctypes.create_string_buffer(64)
    sf, bf = ctypes.c_uint32(), ctypes.c_uint32()
    desc = built._ptr if isinstance(built, BuiltScene) else ctypes.pointer(built)
    check(lib.dt_trace_build(desc, ctypes.byref(g), int(frame), name, 64, ctypes.byref(sf), ctypes.byref(bf)),
          "dt_trace_build")
    return name.value.decode(), sf.value, bf.value


class Scene:
    """Device-resident scene + reference-topology BVH (dt_scene_create). upload=False runs only the
    host half (dt_scene_prepare: no device work, safe beside a running render); upload() or the
    first render does the device half (dt_scene_upload)."""

    def __init__(self, built, g, upload=True):
        self._h = ctypes.c_void_p()
        desc = built._ptr if isinstance(built, BuiltScene) else ctypes.pointer(built)
        self._keep = built
        if upload:
            check(lib.dt_scene_create(desc, ctypes.byref(g), ctypes.byref(self._h)), "dt_scene_create")
        else:
            check(lib.dt_scene_prepare(desc, ctypes.byref(g), ctypes.byref(self._h)), "dt_scene_prepare")

    def upload(self):
        check(lib.dt_scene_upload(self._h), "dt_scene_upload")

    def set_kernel(self, kernel):
        """dt_scene_set_kernel: DT_KERNEL_AUTO (the DT_DONATE environment), DT_KERNEL_PRODUCT or
        DT_KERNEL_DONATE for this scene's renders"""
        check(lib.dt_scene_set_kernel(self._h, kernel), "dt_scene_set_kernel")

    @property
    def handle(self):
        return self._h

    def bvh(self):
        nn, ni = ctypes.c_int32(), ctypes.c_int32()
        check(lib.dt_scene_bvh(self._h, None, 0, None, 0, ctypes.byref(nn), ctypes.byref(ni)), "dt_scene_bvh")
        nodes = (BVHNode * max(nn.value, 1))()
        idx = (ctypes.c_int32 * max(ni.value, 1))()
        check(lib.dt_scene_bvh(self._h, nodes, nn.value, idx, ni.value, ctypes.byref(nn), ctypes.byref(ni)),
              "dt_scene_bvh")
        return list(nodes)[:nn.value], list(idx)[:ni.value]

    def close(self):
        if self._h:
            lib.dt_scene_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ptr(out):
    """(address, on_device) for a torch tensor or numpy array."""
    if hasattr(out, "data_ptr"):
        if out.dtype.__str__() != "torch.float32" or not out.is_contiguous():
            raise DTError("output must be a contiguous float32 tensor")
        return ctypes.c_void_p(out.data_ptr()), 1 if out.is_cuda else 0
    import numpy as np
    if out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"]:
        raise DTError("output must be a contiguous float32 array")
    return ctypes.c_void_p(out.ctypes.data), 0


def render(scene, g, frame, out, tile=None, stream=None):
    """renderImage's pixel loop into `out` (ppmOut layout, or slab layout per `tile`)."""
    st = Stats()
    p, dev = _ptr(out)
    check(lib.dt_render(scene.handle, ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None, p, dev,
                        ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)), "dt_render")
    return st


def render_async(scene, g, frame, out_device, tile=None, stream=None):
    p, dev = _ptr(out_device)
    if not dev:
        raise DTError("render_async needs a device output")
    check(lib.dt_render_async(scene.handle, ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None, p,
                              ctypes.c_void_p(stream) if stream else None), "dt_render_async")


def collect_stats(scene, stream=None):
    st = Stats()
    check(lib.dt_collect_stats(scene.handle, ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)),
          "dt_collect_stats")
    return st


def _ptr_typed(a, torch_dtype, np_dtype):
    if hasattr(a, "data_ptr"):
        if str(a.dtype) != torch_dtype or not a.is_contiguous():
            raise DTError("expected a contiguous %s tensor" % torch_dtype)
        return ctypes.c_void_p(a.data_ptr()), 1 if a.is_cuda else 0
    import numpy as np
    if a.dtype != np.dtype(np_dtype) or not a.flags["C_CONTIGUOUS"]:
        raise DTError("expected a contiguous %s array" % np_dtype)
    return ctypes.c_void_p(a.ctypes.data), 0


def intersect_primary(scene, g, frame, first_ray, hit_shape, hit_t, stream=None):
    """The intersection micro-benchmark: closest hit of primary rays first_ray ..
    first_ray + len(hit_shape) - 1 of the globals' camera (include/dt.h dt_intersect_primary).
    hit_shape: int32, hit_t: float32, both host or both device. Returns the kernel's ms."""
    sp, sdev = _ptr_typed(hit_shape, "torch.int32", "int32")
    tp, tdev = _ptr_typed(hit_t, "torch.float32", "float32")
    n = hit_shape.numel() if hasattr(hit_shape, "numel") else hit_shape.size
    nt = hit_t.numel() if hasattr(hit_t, "numel") else hit_t.size
    if sdev != tdev or n != nt:
        raise DTError("hit_shape and hit_t: same length, same side")
    ms = ctypes.c_float(0)
    check(lib.dt_intersect_primary(scene.handle, ctypes.byref(g), int(frame), int(first_ray), int(n), sp, tp, sdev,
                                   ctypes.c_void_p(stream) if stream else None, ctypes.byref(ms)),
          "dt_intersect_primary")
    return ms.value


def debug_vdiv(vectors, den):
    """The device's division of vectors[i] (n x 3 float64) by den[i] (include/dt.h dt_debug_vdiv): a dict of
    n x 3 arrays `divs_shared`, `divs_plain`, `normalized_shared`, `normalized_plain` and the counts
    `fallback_divs`, `fallback_normalized` of vectors whose shared path divided plainly."""
    import numpy as np
    v = np.ascontiguousarray(vectors, dtype=np.float64)
    s = np.ascontiguousarray(den, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3 or s.shape != (len(v),):
        raise DTError("debug_vdiv: vectors n x 3, den n")
    out = np.empty((4, len(v), 3), dtype=np.float64)
    fb = (ctypes.c_uint64 * 2)()
    PD = ctypes.POINTER(ctypes.c_double)
    check(lib.dt_debug_vdiv(v.ctypes.data_as(PD), s.ctypes.data_as(PD), out.ctypes.data_as(PD), fb, len(v)),
          "dt_debug_vdiv")
    return {"divs_shared": out[0], "divs_plain": out[1], "normalized_shared": out[2], "normalized_plain": out[3],
            "fallback_divs": int(fb[0]), "fallback_normalized": int(fb[1])}


FEATURE_PLANES = ("albedo", "normal", "depth", "coverage", "shape")
GUIDE_MAX_BOUNCES = 8   # DT_GUIDE_MAX_BOUNCES
GUIDE_STOP, GUIDE_REFLECT, GUIDE_REFRACT = 0, 1, 2


def guide_bounce(g, material, flags, inside, in_dir, normal, point):
    """The bounce rule of the specular-path feature buffers for one hit (include/dt.h dt_guide_bounce):
    (result, next_dir, next_start) with result GUIDE_STOP, GUIDE_REFLECT or GUIDE_REFRACT and the next
    segment's unnormalised direction and start as tuples of 3 floats (None, None for GUIDE_STOP). in_dir is
    the normalised ray, normal the fixNorm'ed normal, point the hit point."""
    D3 = ctypes.c_double * 3
    a, b, c = D3(*[float(v) for v in in_dir]), D3(*[float(v) for v in normal]), D3(*[float(v) for v in point])
    nd, ns = D3(), D3()
    rc = lib.dt_guide_bounce(ctypes.byref(g), int(material), int(flags), int(inside), a, b, c, nd, ns)
    if rc < 0:
        check(rc, "dt_guide_bounce")
    return (rc, tuple(nd), tuple(ns)) if rc else (rc, None, None)


def render_features(scene, g, frame, n_samples=None, tile=None, stream=None, planes=FEATURE_PLANES, out=None,
                    stats=None, specular_bounces=0):
    """First-hit feature buffers of the leading n_samples samples (None: spp) of every owned pixel
    (include/dt.h dt_render_features): a dict plane name -> tensor. albedo and normal hold
    accum_doubles(g, tile) float32 elements, indexed like render's output; depth and coverage
    (float32) and shape (int32) a third of that, entry q for the pixel at floats 3q..3q+2. `out`: a
    dict of planes to write into, all CUDA torch tensors or all host arrays (numpy, CPU tensors),
    where only owned pixels are written; without it, new CUDA tensors (zeros, shape -1). stats: a Stats
    to fill with the call's counts.
    specular_bounces=K (1..8): the specular-path feature buffers instead (dt_render_features_path): the guide
    ray follows up to K perfect specular bounces and the planes describe the surface it ends on; "bounces"
    (float32, one per pixel: the mean number of segments followed beyond the first) is then a legal plane."""
    n3 = accum_doubles(g, tile)
    n = _spp(g) if n_samples is None else int(n_samples)
    path = int(specular_bounces) != 0
    legal = FEATURE_PLANES + ("bounces",) if path else FEATURE_PLANES
    if out is None:
        import torch
        for name in planes:
            if name not in legal:
                raise DTError("render_features: unknown plane %r" % (name,))
        out = {name: (torch.full((n3 // 3,), -1, dtype=torch.int32, device="cuda") if name == "shape" else
                      torch.zeros(n3 if name in ("albedo", "normal") else n3 // 3, dtype=torch.float32, device="cuda"))
               for name in planes}
    from ._lib import Features
    f = Features()
    side = None
    bounces_p = None
    for name, a in out.items():
        if name not in legal:
            raise DTError("render_features: unknown plane %r" % (name,))
        p, dev = _ptr_typed(a, "torch.int32", "int32") if name == "shape" else _ptr(a)
        need = n3 if name in ("albedo", "normal") else n3 // 3
        have = a.numel() if hasattr(a, "numel") else a.size
        if have != need:
            raise DTError("render_features: plane %s holds %d elements, (g, tile) need %d" % (name, have, need))
        if side is not None and dev != side:
            raise DTError("render_features: the planes must all be on the same side")
        side = dev
        if name == "bounces":
            bounces_p = p
        else:
            setattr(f, name, p)
    st = stats if stats is not None else Stats()
    if path:
        check(lib.dt_render_features_path(scene.handle, ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None,
                                          n, int(specular_bounces), ctypes.byref(f), bounces_p, side or 0,
                                          ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)),
              "dt_render_features_path")
        return out
    check(lib.dt_render_features(scene.handle, ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None, n,
                                 ctypes.byref(f), side or 0, ctypes.c_void_p(stream) if stream else None,
                                 ctypes.byref(st)), "dt_render_features")
    return out


def occlusion_params_default():
    """dt_occlusion_params_default: ao_rays 4, ao_radius 1.0 (one world unit), no lights"""
    p = OcclusionParams()
    lib.dt_occlusion_params_default(ctypes.byref(p))
    return p


def occlusion_ao_ray(g, frame, pixel, sample, r, ao_radius, point, normal):
    """The direction of ambient-occlusion probe r of sample `sample` of pixel `pixel` (y*xRes + x) from a hit
    with the fixNorm'ed normal `normal` (include/dt.h dt_occlusion_ao_ray), as a tuple of 3 floats"""
    D3 = ctypes.c_double * 3
    out = D3()
    check(lib.dt_occlusion_ao_ray(g.seed, int(frame), int(pixel), int(sample), int(r), float(ao_radius),
                                  D3(*[float(v) for v in point]), D3(*[float(v) for v in normal]), out),
          "dt_occlusion_ao_ray")
    return tuple(out)


def occlusion_light_ray(g, frame, pixel, sample, j, light, point):
    """The direction of the probe of light slot j towards `light` (a LightDesc) from `point`
    (include/dt.h dt_occlusion_light_ray), as a tuple of 3 floats"""
    D3 = ctypes.c_double * 3
    out = D3()
    check(lib.dt_occlusion_light_ray(g.seed, int(frame), int(pixel), int(sample), int(j), ctypes.byref(light),
                                     D3(*[float(v) for v in point]), out), "dt_occlusion_light_ray")
    return tuple(out)


def render_occlusion(scene, g, frame, n_samples=None, ao_rays=4, ao_radius=None, lights=(), tile=None, stream=None,
                     out=None):
    """Occlusion feature buffers of the leading n_samples samples (None: spp) of every owned pixel
    (include/dt.h dt_render_occlusion): (dict(ao=..., light=...), stats). `ao` (one float32 per pixel, entry q as
    render_features' depth; only with ao_rays > 0) is the fraction of ambient-occlusion probes that found the
    ball of radius ao_radius resting on the surface visible (None: occlusion_params_default's constant, one
    world unit: a property of the shipped scenes' human scale, so a scene in other units needs ao_radius set
    explicitly); `light`
    (len(lights) per pixel, entry len(lights)*q + j; only with lights) the fraction of samples from which light
    lights[j] of the scene was visible. Both are premultiplied by coverage. `out`: a dict of the planes to write
    into, all CUDA torch tensors or all host arrays (numpy, CPU tensors), where only owned pixels are written;
    without it, new zeroed CUDA tensors."""
    from ._lib import Occlusion
    n1 = accum_doubles(g, tile) // 3
    n = _spp(g) if n_samples is None else int(n_samples)
    p = OcclusionParams()
    p.ao_rays, p.n_lights = int(ao_rays), len(lights)
    if len(lights) > len(p.lights):
        raise DTError("render_occlusion: %d lights, at most %d" % (len(lights), len(p.lights)))
    for j, l in enumerate(lights):
        p.lights[j] = int(l)
    if p.ao_rays > 0:
        p.ao_radius = occlusion_params_default().ao_radius if ao_radius is None else float(ao_radius)
    need = {"ao": n1, "light": n1 * len(lights)}
    if out is None:
        import torch
        out = {}
        if p.ao_rays > 0:
            out["ao"] = torch.zeros(n1, dtype=torch.float32, device="cuda")
        if lights:
            out["light"] = torch.zeros(n1 * len(lights), dtype=torch.float32, device="cuda")
    o = Occlusion()
    side = None
    for name, a in out.items():
        if name not in need:
            raise DTError("render_occlusion: unknown plane %r" % (name,))
        ptr, dev = _ptr(a)
        have = a.numel() if hasattr(a, "numel") else a.size
        if have != need[name] and need[name] > 0:
            raise DTError("render_occlusion: plane %s holds %d elements, (g, tile, lights) need %d"
                          % (name, have, need[name]))
        if side is not None and dev != side:
            raise DTError("render_occlusion: the planes must all be on the same side")
        side = dev
        setattr(o, name, ptr)
    st = Stats()
    check(lib.dt_render_occlusion(scene.handle, ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None, n,
                                  ctypes.byref(p), ctypes.byref(o), side or 0,
                                  ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)), "dt_render_occlusion")
    return out, st


def points_occlusion(scene, g, points, normals, frame=0, n_samples=16, ao_rays=4, ao_radius=None, lights=(),
                     stream=None, through_glass=None):
    """Occlusion at surface points the caller supplies (include/dt.h dt_points_occlusion), for baking: points and
    normals are float64, shaped (n, 3) or flat, numpy arrays or torch tensors, both on one side; a normal is
    used as given (unit length and pointing away from the surface is the caller's business). Point i takes
    n_samples samples of render_occlusion's probes with pixel = i: ao_rays ambient-occlusion probes (ao_radius
    None: occlusion_params_default's constant) and one probe per light of `lights`. Returns (dict(ao=...,
    light=...), stats) on the side of points: `ao` float32 (n,), only with ao_rays > 0; `light` float32
    (n, len(lights)), only with lights. A point with a non-finite component gets zeros. 64 consecutive points
    share a wave: keep neighbours in the arrays neighbours in space.
    through_glass: None, a glass shape shadows like a wall (dt_points_occlusion); an integer 0..8, the probes pass
    through glass (dt_points_occlusion_glass): a probe is unoccluded iff no other shape stops it and it crosses at
    most that many glass shapes, and the dict gains `ao_panes` and `light_panes`, shaped like ao and light: the
    panes the unoccluded probes crossed, summed and divided by the denominators of ao and light. 0 gives
    today's ao and light."""
    from ._lib import Occlusion
    n, pp, np_, side = _ray_arrays("points_occlusion", points, normals)
    p = OcclusionParams()
    p.ao_rays, p.n_lights = int(ao_rays), len(lights)
    if len(lights) > len(p.lights):
        raise DTError("points_occlusion: %d lights, at most %d" % (len(lights), len(p.lights)))
    for j, l in enumerate(lights):
        p.lights[j] = int(l)
    if p.ao_rays > 0:
        p.ao_radius = occlusion_params_default().ao_radius if ao_radius is None else float(ao_radius)
    out, o = {}, Occlusion()
    none = ctypes.cast(_NO_RAYS, ctypes.c_void_p)
    if p.ao_rays > 0:
        out["ao"] = _ray_new(points, (n,), "torch.float32", "float32")
        o.ao = _ptr(out["ao"])[0].value or none.value
    if lights:
        out["light"] = _ray_new(points, (n, len(lights)), "torch.float32", "float32")
        o.light = _ptr(out["light"])[0].value or none.value
    st = Stats()
    if through_glass is not None:
        from ._lib import OcclusionPanes
        if isinstance(through_glass, bool) or not isinstance(through_glass, int):
            raise DTError("points_occlusion: through_glass must be None or an integer, not %r" % (through_glass,))
        op = OcclusionPanes()
        if p.ao_rays > 0:
            out["ao_panes"] = _ray_new(points, (n,), "torch.float32", "float32")
            op.ao_panes = _ptr(out["ao_panes"])[0].value or none.value
        if lights:
            out["light_panes"] = _ray_new(points, (n, len(lights)), "torch.float32", "float32")
            op.light_panes = _ptr(out["light_panes"])[0].value or none.value
        check(lib.dt_points_occlusion_glass(scene.handle, ctypes.byref(g), int(frame), n, pp, np_, int(n_samples),
                                            ctypes.byref(p), through_glass, ctypes.byref(o), ctypes.byref(op), side,
                                            ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)),
              "dt_points_occlusion_glass")
        return out, st
    check(lib.dt_points_occlusion(scene.handle, ctypes.byref(g), int(frame), n, pp, np_, int(n_samples), ctypes.byref(p),
                                  ctypes.byref(o), side, ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)),
          "dt_points_occlusion")
    return out, st


def _shape_texels(desc, shape_index, width, height, side):
    """shape_texels' arrays and the indices v*width + u of the texels kept"""
    import numpy as np
    d = desc.desc if isinstance(desc, BuiltScene) else desc
    shape_index, width, height = int(shape_index), int(width), int(height)
    if not 0 <= shape_index < int(d.n_shapes):
        raise DTError("shape_texels: shape %d, the scene has %d shapes" % (shape_index, int(d.n_shapes)))
    if width < 1 or height < 1:
        raise DTError("shape_texels: width and height must be >= 1")
    RECTANGLE, CHECKERBOARD, TRIANGLE = 4, 6, 3
    s = d.shapes[shape_index]
    if s.type not in (RECTANGLE, CHECKERBOARD, TRIANGLE):
        raise DTError("shape_texels: shape %d is a %s; a rectangle, checkerboard or triangle is needed"
                      % (shape_index, SHAPE_TYPES.get(s.type, s.type)))
    A = np.array(s.v[0][:], np.float64)
    e1 = np.array(s.v[1][:], np.float64) - A
    e2 = np.array(s.v[2 if s.type == TRIANGLE else 3][:], np.float64) - A
    a = np.tile((np.arange(width) + 0.5) / width, height)
    b = np.repeat((np.arange(height) + 0.5) / height, width)
    keep = np.flatnonzero(a + b <= 1.0) if s.type == TRIANGLE else np.arange(width * height)
    a, b = a[keep], b[keep]
    points = (A[None, :] + a[:, None] * e1[None, :]) + b[:, None] * e2[None, :]
    # (each operation one rounded f64 one, in this order: dtrender --bake-occlusion computes the same bits)
    nrm = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    length = np.sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2])
    if not (np.isfinite(length) and length > 0):
        raise DTError("shape_texels: shape %d has no area" % shape_index)
    nrm = float(side) * (nrm / length)
    return np.ascontiguousarray(points), np.ascontiguousarray(np.tile(nrm, (len(keep), 1))), keep


def shape_texels(desc, shape_index, width, height, side=1):
    """The texel centres of a width x height lightmap over a DT_SHAPE_RECTANGLE, DT_SHAPE_CHECKERBOARD or
    DT_SHAPE_TRIANGLE shape of a scene descriptor (a BuiltScene or a SceneDesc), as points_occlusion takes them:
    (points, normals), float64 (n, 3), texel (u, v) at row v*width + u. With e1 = B - A and e2 = D - A (a
    triangle: C - A), the centre is A + ((u+0.5)/width)*e1 + ((v+0.5)/height)*e2 and the normal
    side * normalized(cross(e1, e2)); of a triangle only the texels whose centre lies inside it are kept, in the
    same order. Pure numpy, no device. Neighbouring rows are neighbouring texels, which is what the kernel's
    waves want."""
    return _shape_texels(desc, shape_index, width, height, side)[:2]


def bake_occlusion(scene, desc, g, shape_index, width, height, side=1, through_glass=None, **kw):
    """A lightmap of one shape: points_occlusion(scene, g, *shape_texels(desc, shape_index, width, height, side),
    **kw) as numpy images, (dict(ao=(height, width), light=(height, width, n_lights)), stats), row v, column u.
    A triangle's texels outside it are 0. through_glass as for points_occlusion: an integer adds the images
    ao_panes and light_panes, shaped like ao and light."""
    import numpy as np
    points, normals, keep = _shape_texels(desc, shape_index, width, height, side)
    planes, st = points_occlusion(scene, g, points, normals, through_glass=through_glass, **kw)
    out = {}
    for name, a in planes.items():
        img = np.zeros((int(height) * int(width),) + a.shape[1:], np.float32)
        img[keep] = a
        out[name] = img.reshape((int(height), int(width)) + a.shape[1:])
    return out, st


IRRADIANCE_PLANES = ("direct", "direct_rgb", "indirect_rgb", "sky")


def irradiance_gather_ray(g, frame, pixel, sample, r, point, normal):
    """Gather probe r of sample `sample` of point `pixel` of points_irradiance (include/dt.h
    dt_irradiance_gather_ray): (start, dir), two tuples of 3 floats; a void probe has dir (0, 0, 0)"""
    D3 = ctypes.c_double * 3
    start, dir = D3(), D3()
    check(lib.dt_irradiance_gather_ray(g.seed, int(frame), int(pixel), int(sample), int(r),
                                       D3(*[float(v) for v in point]), D3(*[float(v) for v in normal]), start, dir),
          "dt_irradiance_gather_ray")
    return tuple(start), tuple(dir)


def irradiance_cosine(normal, dir):
    """max(0, dot(normal, normalized(dir))) as points_irradiance weights a probe (include/dt.h
    dt_irradiance_cosine); 0.0 for a void dir"""
    D3 = ctypes.c_double * 3
    c = ctypes.c_double()
    check(lib.dt_irradiance_cosine(D3(*[float(v) for v in normal]), D3(*[float(v) for v in dir]), ctypes.byref(c)),
          "dt_irradiance_cosine")
    return c.value


def points_irradiance(scene, g, points, normals, frame=0, n_samples=16, lights=(), gather_rays=0, planes=None,
                      stream=None):
    """Irradiance at surface points the caller supplies (include/dt.h dt_points_irradiance), for light baking:
    points and normals as points_occlusion takes them. Per point the cosine-weighted visibility of each light of
    `lights` (`direct`, float32 (n, len(lights))), its sum with the lights' colours (`direct_rgb`, (n, 3)), one
    diffuse bounce gathered with gather_rays probes per sample (`indirect_rgb`, (n, 3); needs lights) and the share
    of gather probes that hit nothing (`sky`, (n,)). planes: the names wanted (None: every plane that lights and
    gather_rays allow); a plane that is not wanted costs no probes. Returns (dict, stats) on the side of points;
    stats.shadow_rays counts the shadow probes, stats.rays the gather probes. No distance falloff, one bounce,
    a specular surface met by a gather probe is shaded as diffuse."""
    from ._lib import Irradiance, IrradianceParams
    n, pp, np_, side = _ray_arrays("points_irradiance", points, normals)
    p = IrradianceParams()
    p.n_lights, p.gather_rays = len(lights), int(gather_rays)
    if len(lights) > len(p.light):
        raise DTError("points_irradiance: %d lights, at most %d" % (len(lights), len(p.light)))
    for j, l in enumerate(lights):
        p.light[j] = int(l)
    if planes is None:
        planes = tuple(name for name, ok in zip(IRRADIANCE_PLANES, (bool(lights), bool(lights),
                                                                    bool(lights) and p.gather_rays > 0,
                                                                    p.gather_rays > 0)) if ok)
    shapes = {"direct": (n, len(lights)), "direct_rgb": (n, 3), "indirect_rgb": (n, 3), "sky": (n,)}
    out, o = {}, Irradiance()
    none = ctypes.cast(_NO_RAYS, ctypes.c_void_p)
    for name in planes:
        if name not in shapes:
            raise DTError("points_irradiance: unknown plane %r" % (name,))
        out[name] = _ray_new(points, shapes[name], "torch.float32", "float32")
        setattr(o, name, _ptr(out[name])[0].value or none.value)
    st = Stats()
    check(lib.dt_points_irradiance(scene.handle, ctypes.byref(g), int(frame), n, pp, np_, int(n_samples),
                                   ctypes.byref(p), ctypes.byref(o), side, ctypes.c_void_p(stream) if stream else None,
                                   ctypes.byref(st)), "dt_points_irradiance")
    return out, st


def bake_irradiance(scene, desc, g, shape_index, width, height, side=1, **kw):
    """A lightmap of one shape: points_irradiance(scene, g, *shape_texels(desc, shape_index, width, height, side),
    **kw) as numpy images, row v, column u: direct (height, width, n_lights), direct_rgb and indirect_rgb (height,
    width, 3), sky (height, width). A triangle's texels outside it are 0."""
    import numpy as np
    points, normals, keep = _shape_texels(desc, shape_index, width, height, side)
    planes, st = points_irradiance(scene, g, points, normals, **kw)
    out = {}
    for name, a in planes.items():
        img = np.zeros((int(height) * int(width),) + a.shape[1:], np.float32)
        img[keep] = a
        out[name] = img.reshape((int(height), int(width)) + a.shape[1:])
    return out, st


VISIBILITY_PLANES = ("bits", "count_a", "count_b", "weight_a")


def points_visibility(scene, g, a, b, skip_b=None, normals_a=None, normals_b=None, falloff=False,
                      planes=("bits", "count_a", "count_b"), stream=None):
    """Which of the targets b can each of the sources a see (include/dt.h dt_points_visibility)? a and b are float64,
    shaped (n, 3) or flat, numpy arrays or torch tensors, all arrays of a call on one side. Pair (i, j) is answered
    as rays_occluded answers (a[i], b[j] - a[i], skip_b[j]): skip_b is int32 per target, the shape the target is or
    lies on (-1: none). Returns (dict, stats) on the side of a for the planes asked for: `bits` (n_a, ceil(n_b/32))
    uint32 in numpy, the same bits as int32 in torch (visibility_matrix unpacks them), `count_a` int32 (n_a,) the
    targets each source sees, `count_b` int32 (n_b,) the sources that see each target, `weight_a` float64 (n_a,)
    the sum over the visible targets of cos_a * cos_b (falloff: divided by the squared distance), which needs
    normals_a and normals_b (as given: not normalised) and has a fixed summation order. A point with a non-finite
    component sees nothing and is seen by nothing. 64 consecutive sources share a wave and walk towards one target
    at a time: keep both arrays spatially ordered."""
    from ._lib import Visibility, VisibilityParams
    sp, side = _ptr_typed(a, "torch.float64", "float64")
    tp, tside = _ptr_typed(b, "torch.float64", "float64")
    na3, nb3 = _numel_any(a), _numel_any(b)
    if na3 % 3 or nb3 % 3 or side != tside:
        raise DTError("points_visibility: a and b hold 3 doubles per point, on the same side")
    n_a, n_b = na3 // 3, nb3 // 3
    none = ctypes.cast(_NO_RAYS, ctypes.c_void_p)
    p = VisibilityParams()
    lib.dt_visibility_params_default(ctypes.byref(p))
    p.falloff = 1 if falloff else 0
    if skip_b is not None:
        p.skip_b = _ray_out("points_visibility", "skip_b", skip_b, n_b, 1, "torch.int32", "int32", side).value
    if "weight_a" in planes and (normals_a is None or normals_b is None):
        raise DTError("points_visibility: weight_a needs normals_a and normals_b")
    if normals_a is not None:
        p.normal_a = _ray_out("points_visibility", "normals_a", normals_a, n_a, 3, "torch.float64", "float64", side).value
    if normals_b is not None:
        p.normal_b = _ray_out("points_visibility", "normals_b", normals_b, n_b, 3, "torch.float64", "float64", side).value
    words = (n_b + 31) // 32
    types = {"bits": ((n_a, words), "torch.int32", "uint32"), "count_a": ((n_a,), "torch.int32", "int32"),
             "count_b": ((n_b,), "torch.int32", "int32"), "weight_a": ((n_a,), "torch.float64", "float64")}
    out, o = {}, Visibility()
    for name in planes:
        if name not in types:
            raise DTError("points_visibility: unknown plane %r" % (name,))
        out[name] = _ray_new(a, *types[name])
        setattr(o, name, _data_ptr(out[name]).value)
    st = Stats()
    check(lib.dt_points_visibility(scene.handle if scene is not None else None, ctypes.byref(g), n_a,
                                   sp if sp.value else none, n_b, tp if tp.value else none, ctypes.byref(p),
                                   ctypes.byref(o), side, ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)),
          "dt_points_visibility")
    return out, st


def visibility_matrix(bits, n_b):
    """The bool (n_a, n_b) matrix of points_visibility's `bits` (numpy uint32 or a torch int32 tensor, shaped
    (n_a, ceil(n_b/32))): entry (i, j) is bit (j & 31) of word j >> 5 of row i. numpy, on the host."""
    import numpy as np
    w = bits.cpu().numpy() if hasattr(bits, "data_ptr") else np.asarray(bits)
    n_b = int(n_b)
    words = (n_b + 31) // 32
    w = np.ascontiguousarray(w).view(np.uint32).reshape(-1, words) if words else np.zeros((w.shape[0], 0), np.uint32)
    shifts = np.arange(32, dtype=np.uint32)
    return (((w[:, :, None] >> shifts[None, None, :]) & np.uint32(1)) != 0).reshape(w.shape[0], words * 32)[:, :n_b]


def bake_visibility(scene, desc, g, shape_a, shape_b, width, height, target_size=(8, 8), side=1, **kw):
    """How much of shape_b does each texel of shape_a see? Sources are shape_texels(desc, shape_a, width, height,
    side), targets shape_texels(desc, shape_b, *target_size) with skip_b = shape_b (the target shape hides none of
    its own texels). Returns (dict, stats) of numpy images, row v, column u: `visible` float32 (height, width) =
    count_a / n_b, the share of shape_b's texels the texel sees, and with planes holding "weight_a" (normals are the
    texels') `weight` float64 (height, width). A triangle's texels outside it are 0. kw: falloff, planes, stream
    of points_visibility; count_a is always computed."""
    import numpy as np
    pa, na, keep = _shape_texels(desc, shape_a, width, height, side)
    pb, nb, _ = _shape_texels(desc, shape_b, int(target_size[0]), int(target_size[1]), 1)
    planes = tuple(kw.pop("planes", ("count_a",)))
    if "count_a" not in planes:
        planes += ("count_a",)
    got, st = points_visibility(scene, g, pa, pb, skip_b=np.full(len(pb), int(shape_b), np.int32), normals_a=na,
                                normals_b=nb, planes=planes, **kw)
    n_px = int(height) * int(width)
    vis = np.zeros(n_px, np.float32)
    vis[keep] = (got["count_a"].astype(np.float64) / float(len(pb))).astype(np.float32)
    out = {"visible": vis.reshape(int(height), int(width))}
    if "weight_a" in got:
        wgt = np.zeros(n_px, np.float64)
        wgt[keep] = got["weight_a"]
        out["weight"] = wgt.reshape(int(height), int(width))
    return out, st


def irradiance_images(g, planes):
    """The images `dtrender --bake-light` writes, as float32 arrays for write_png: {"direct": direct_rgb,
    "indirect": indirect_rgb, "sky": sky}, RGB clamped to 0..1, times 255. planes: full-frame image-layout planes
    of bake_irradiance (numpy); g.xRes x g.yRes is the lightmap's size."""
    import numpy as np
    n1 = g.xRes * g.yRes
    out = {}
    for name, key in (("direct", "direct_rgb"), ("indirect", "indirect_rgb")):
        if key in planes:
            v = np.asarray(planes[key], np.float32).reshape(n1 * 3)
            out[name] = np.minimum(np.maximum(v, np.float32(0)), np.float32(1)) * np.float32(255)
    if "sky" in planes:
        v = np.asarray(planes["sky"], np.float32).reshape(n1)
        out["sky"] = np.repeat(np.minimum(np.maximum(v, np.float32(0)), np.float32(1)) * np.float32(255), 3)
    return out


def occlusion_images(g, planes):
    """The images `dtrender --occlusion P` writes, as float32 arrays for write_png: {"ao": ..., "light<j>": ...},
    each plane times 255 in all three channels. planes: full-frame image-layout planes of render_occlusion
    (numpy)."""
    import numpy as np
    n1 = g.xRes * g.yRes
    out = {}
    if "ao" in planes:
        out["ao"] = np.repeat(np.asarray(planes["ao"], np.float32).reshape(n1) * np.float32(255), 3)
    if "light" in planes:
        v = np.asarray(planes["light"], np.float32).reshape(n1, -1)
        for j in range(v.shape[1]):
            out["light%d" % j] = np.repeat(np.ascontiguousarray(v[:, j]) * np.float32(255), 3)
    # the pane planes of through_glass (`dtrender --bake-through-glass`): 8 panes (DT_TRANSMIT_MAX_PANES) are white
    if "ao_panes" in planes:
        a = np.asarray(planes["ao_panes"], np.float32).reshape(n1)
        out["ao_panes"] = np.repeat((a / np.float32(8)) * np.float32(255), 3)
    if "light_panes" in planes:
        v = np.asarray(planes["light_panes"], np.float32).reshape(n1, -1)
        for j in range(v.shape[1]):
            out["light_panes%d" % j] = np.repeat((np.ascontiguousarray(v[:, j]) / np.float32(8)) * np.float32(255), 3)
    return out


MATTE_PLANES = ("id", "weight", "distinct")


def shape_groups(desc, by="material"):
    """A group per shape of a scene descriptor (a BuiltScene or a SceneDesc), as an int32 array for
    render_mattes: by="material" one group per distinct (mesh triangle?, model, material, emit, flags &
    (LIGHT | TEXTURE | GLOSSY | MESH), tex_frame, color) signature, numbered in order of first appearance
    (a mesh, or the cylinders of one skeleton, become one object); "shape" the identity; "type" the shape
    type."""
    import numpy as np
    d = desc.desc if isinstance(desc, BuiltScene) else desc
    n = int(d.n_shapes)
    if by == "shape":
        return np.arange(n, dtype=np.int32)
    if by == "type":
        return np.array([d.shapes[i].type for i in range(n)], dtype=np.int32)
    if by != "material":
        raise DTError("shape_groups: by is 'material', 'shape' or 'type', not %r" % (by,))
    F_LIGHT, F_TEXTURE, F_GLOSSY, F_MESH, TRIANGLE = 1, 4, 8, 32, 3
    seen, out = {}, np.empty(n, dtype=np.int32)
    for i in range(n):
        s = d.shapes[i]
        sig = (s.type == TRIANGLE and bool(s.flags & F_MESH), s.model, s.material, s.emit,
               s.flags & (F_LIGHT | F_TEXTURE | F_GLOSSY | F_MESH), s.tex_frame, tuple(s.color))
        out[i] = seen.setdefault(sig, len(seen))
    return out


def render_mattes(scene, g, frame, n_samples=None, groups=None, layers=4, tiles=None, planes=("id", "weight"), out=None,
                  stream=None, stats=None):
    """Object mattes (include/dt.h dt_render_mattes): for every owned pixel the `layers` groups that cover
    most of its leading n_samples samples (None: spp), ranked, from the render's own primary rays. groups:
    an int32 group per shape (shape_groups; None: every shape its own group). Returns a dict: id (int32, -1:
    no such layer) and weight (float32), shaped (yRes, xRes, layers) for a whole image (rows as render's
    output) and flat (layers per slot) for a slab; distinct (int32, (yRes, xRes) or flat) when asked for;
    "layers"; and "overflow_pixels", the owned pixels that met more than 64 groups. `out`: a dict of planes to
    write into instead (it decides the planes), all CUDA torch tensors or all host arrays, where only owned
    pixels are written; without it, new CUDA tensors (id -1, weight and distinct 0). `tiles`: a Tiles."""
    import numpy as np
    tile = tiles
    n1 = accum_doubles(g, tile) // 3
    n = _spp(g) if n_samples is None else int(n_samples)
    layers = int(layers)
    whole = tile is None or tile.layout == DT_OUT_IMAGE
    if out is None:
        import torch
        if not 1 <= layers <= 8:
            raise DTError("render_mattes: layers %d outside 1..8" % layers)
        out = {}
        for name in planes:
            if name not in MATTE_PLANES:
                raise DTError("render_mattes: unknown plane %r" % (name,))
            shape = ((g.yRes, g.xRes) if whole else (n1,)) if name == "distinct" else \
                ((g.yRes, g.xRes, layers) if whole else (n1 * layers,))
            out[name] = torch.zeros(shape, dtype=torch.float32, device="cuda") if name == "weight" else \
                torch.full(shape, -1 if name == "id" else 0, dtype=torch.int32, device="cuda")
    from ._lib import Mattes
    m = Mattes()
    side = None
    for name, a in out.items():
        if name not in MATTE_PLANES:
            raise DTError("render_mattes: unknown plane %r" % (name,))
        p, dev = _ptr(a) if name == "weight" else _ptr_typed(a, "torch.int32", "int32")
        need = n1 if name == "distinct" else n1 * layers
        if _numel_any(a) != need:
            raise DTError("render_mattes: plane %s holds %d elements, (g, tiles, layers) need %d"
                          % (name, _numel_any(a), need))
        if side is not None and dev != side:
            raise DTError("render_mattes: the planes must all be on the same side")
        side = dev
        setattr(m, name, p)
    built = scene._keep
    n_shapes = int((built.desc if isinstance(built, BuiltScene) else built).n_shapes)
    gp = None
    if groups is not None:
        gmap = np.ascontiguousarray(groups.cpu().numpy() if hasattr(groups, "data_ptr") else groups, dtype=np.int32)
        if gmap.size != n_shapes:
            raise DTError("render_mattes: groups holds %d entries, the scene has %d shapes" % (gmap.size, n_shapes))
        gp = ctypes.c_void_p(gmap.ctypes.data)
    st = stats if stats is not None else Stats()
    over = ctypes.c_uint64(0)
    check(lib.dt_render_mattes(scene.handle, ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None, n, gp,
                               n_shapes, layers, ctypes.byref(m), side or 0, ctypes.c_void_p(stream) if stream else None,
                               ctypes.byref(st), ctypes.byref(over)), "dt_render_mattes")
    res = dict(out)
    res["layers"] = layers
    res["overflow_pixels"] = over.value
    return res


def matte_mask(mattes, groups, out=None, stream=None):
    """The antialiased matte of a set of groups from render_mattes' id and weight planes (include/dt.h
    dt_matte_mask): per pixel the float32 sum, in layer order, of the weights of the layers whose group is in
    `groups` (an int, or 1..64 ints). Returns a float32 plane on the side of the planes, shaped like them
    without the layer axis (or `out`). On the device it is enqueued on `stream`."""
    import numpy as np
    ids, w = mattes["id"], mattes["weight"]
    layers = int(mattes["layers"]) if "layers" in mattes else int(ids.shape[-1])
    ip, idev = _ptr_typed(ids, "torch.int32", "int32")
    wp, wdev = _ptr(w)
    if idev != wdev or _numel_any(ids) != _numel_any(w) or layers < 1 or _numel_any(ids) % layers:
        raise DTError("matte_mask: id and weight hold `layers` entries per pixel, on the same side")
    n = _numel_any(ids) // layers
    gl = np.ascontiguousarray(np.atleast_1d(np.asarray(groups)).ravel(), dtype=np.int32)
    if out is None:
        shape = tuple(ids.shape[:-1]) if len(ids.shape) > 1 else (n,)
        out = _ray_new(ids, shape, "torch.float32", "float32")
    op, odev = _ptr(out)
    if odev != idev or _numel_any(out) != n:
        raise DTError("matte_mask: out holds one float32 per pixel, on the side of the planes")
    none = ctypes.cast(_NO_RAYS, ctypes.c_void_p)
    check(lib.dt_matte_mask(n, layers, ip if ip.value else none, wp if wp.value else none,
                            ctypes.c_void_p(gl.ctypes.data) if gl.size else none, int(gl.size), op if op.value else none,
                            idev, ctypes.c_void_p(stream) if stream else None), "dt_matte_mask")
    return out


RAY_PLANES = ("shape", "t", "point", "normal", "albedo")
# plane -> (torch dtype, numpy dtype, values per ray)
_RAY_PLANE_TYPES = {"shape": ("torch.int32", "int32", 1), "t": ("torch.float32", "float32", 1),
                    "point": ("torch.float64", "float64", 3), "normal": ("torch.float64", "float64", 3),
                    "albedo": ("torch.float64", "float64", 3)}
_NO_RAYS = (ctypes.c_double * 3)()   # stands in for the null data pointer of an empty array (n = 0 reads nothing)


def _numel_any(a):
    return a.numel() if hasattr(a, "numel") else a.size


def _ray_arrays(what, start, dir):
    """(n, start pointer, dir pointer, on_device) of two float64 arrays shaped (n, 3) or flat, on one side"""
    sp, sdev = _ptr_typed(start, "torch.float64", "float64")
    dp, ddev = _ptr_typed(dir, "torch.float64", "float64")
    ns, nd = _numel_any(start), _numel_any(dir)
    if ns % 3 or ns != nd or sdev != ddev:
        raise DTError("%s: start and dir hold 3 doubles per ray, the same number of rays, on the same side" % what)
    none = ctypes.cast(_NO_RAYS, ctypes.c_void_p)
    return ns // 3, sp if sp.value else none, dp if dp.value else none, sdev


def _ray_new(like, shape, torch_dtype, np_dtype):
    """a new array on the side of `like` (a CUDA or CPU tensor, or a numpy array)"""
    if hasattr(like, "data_ptr"):
        import torch
        return torch.zeros(shape, dtype=getattr(torch, torch_dtype.split(".")[1]), device=like.device)
    import numpy as np
    return np.zeros(shape, dtype=np_dtype)


def _ray_out(what, name, a, n, per, torch_dtype, np_dtype, side):
    p, dev = _ptr_typed(a, torch_dtype, np_dtype)
    if _numel_any(a) != n * per:
        raise DTError("%s: %s holds %d elements, %d rays need %d" % (what, name, _numel_any(a), n, n * per))
    if dev != side:
        raise DTError("%s: %s must be on the side of start" % (what, name))
    return p if p.value else ctypes.cast(_NO_RAYS, ctypes.c_void_p)


def ray_order_params_default():
    """dt_ray_order_params_default: origin_bits 5, dir_bits 6, origin-major, the box from the rays (a choice, not a
    measurement; for rays that all start on one lens use origin_bits=0, dir_bits=8)"""
    p = RayOrderParams()
    lib.dt_ray_order_params_default(ctypes.byref(p))
    return p


def ray_order_key(params, lo, hi, start, dir):
    """The sort key of one ray inside the box (lo, hi) (include/dt.h dt_ray_order_key), on the host."""
    from ._lib import D3
    key = ctypes.c_uint32()
    check(lib.dt_ray_order_key(ctypes.byref(params), D3(*[float(x) for x in lo]), D3(*[float(x) for x in hi]),
                               D3(*[float(x) for x in start]), D3(*[float(x) for x in dir]), ctypes.byref(key)),
          "dt_ray_order_key")
    return key.value


def _side(a):
    return 1 if hasattr(a, "data_ptr") and a.is_cuda else 0


def _data_ptr(a):
    p = a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
    return ctypes.c_void_p(p) if p else ctypes.cast(_NO_RAYS, ctypes.c_void_p)


def _is_contiguous(a):
    return a.is_contiguous() if hasattr(a, "data_ptr") else a.flags["C_CONTIGUOUS"]


class RayOrder:
    """What ray_order returns: `perm` (perm[i] is the caller's index of the ray that goes to place i; uint32 in
    numpy, the same bits as int32 in torch: entries are below 2^30), `keys` (in the caller's order, or None),
    `box` (lo and hi as used, six floats), `kernel_ms` (the device chain's HIP-event time, 0.0 on the host),
    and the two row permutations of dt_permute_rows on the side of perm."""

    def __init__(self, n, perm, keys, box, kernel_ms, stream):
        self.n, self.perm, self.keys, self.box, self.kernel_ms, self.stream = n, perm, keys, box, kernel_ms, stream

    def _permute(self, what, a, out, inverse):
        if _side(a) != _side(self.perm) or not _is_contiguous(a):
            raise DTError("RayOrder.%s: a contiguous array on the side of the order is needed" % what)
        nbytes = _numel_any(a) * (a.element_size() if hasattr(a, "data_ptr") else a.itemsize)
        if self.n == 0 and nbytes == 0:
            row = 1
        elif self.n == 0 or nbytes % self.n or not 1 <= nbytes // self.n <= 64:
            raise DTError("RayOrder.%s: %d bytes are not %d rows of 1..64 bytes" % (what, nbytes, self.n))
        else:
            row = nbytes // self.n
        if out is None:
            if hasattr(a, "data_ptr"):
                import torch
                out = torch.empty_like(a)
            else:
                import numpy as np
                out = np.empty_like(a)
        elif (_side(out) != _side(a) or not _is_contiguous(out) or out.dtype != a.dtype or
              _numel_any(out) != _numel_any(a)):
            raise DTError("RayOrder.%s: out must be a contiguous array like the input, on its side" % what)
        check(lib.dt_permute_rows(self.n, row, _data_ptr(self.perm), _data_ptr(a), _data_ptr(out), inverse,
                                  _side(a), ctypes.c_void_p(self.stream) if self.stream else None), "dt_permute_rows")
        return out

    def apply(self, a, out=None):
        """rows in sorted order: out[i] = a[perm[i]] (a: n rows of 1..64 bytes, such as start, dir, skip_shape)"""
        return self._permute("apply", a, out, 0)

    def restore(self, a, out=None):
        """answers back in the caller's order: out[perm[i]] = a[i]"""
        return self._permute("restore", a, out, 1)


def ray_order(start, dir, params=None, keys=False, stream=None):
    """The order that sorts rays into coherent waves (include/dt.h dt_ray_order): start and dir as for trace_rays.
    Returns a RayOrder whose perm is the stable ascending order of the rays' keys, numpy's argsort(keys,
    kind="stable"); on the device a radix sort enqueued on `stream` (the call waits for it: box and kernel_ms
    come back). One order serves every query on the same rays: order.apply(start), order.apply(dir), the
    query, order.restore(answer) -- or trace_rays(..., order=order)."""
    n, sp, dp, side = _ray_arrays("ray_order", start, dir)
    p = params if params is not None else ray_order_params_default()
    perm = _ray_new(start, (n,), "torch.int32", "uint32")
    k = _ray_new(start, (n,), "torch.int32", "uint32") if keys else None
    work = None
    if side and n:
        import torch
        work = torch.empty(int(lib.dt_ray_order_workspace_bytes(n)), dtype=torch.uint8, device=start.device)
    box = (ctypes.c_double * 6)()
    ms = ctypes.c_float(0.0)
    check(lib.dt_ray_order(n, sp, dp, ctypes.byref(p), _data_ptr(perm), _data_ptr(k) if keys else None, box,
                           _data_ptr(work) if work is not None else (ctypes.cast(_NO_RAYS, ctypes.c_void_p) if side else None),
                           side, ctypes.c_void_p(stream) if stream else None, ctypes.byref(ms)), "dt_ray_order")
    return RayOrder(n, perm, k, tuple(box), float(ms.value), stream)


def _order_for(what, order, start, dir, n, side, stream):
    if order is True:
        order = ray_order(start, dir, stream=stream)
    if not isinstance(order, RayOrder) or order.n != n or _side(order.perm) != side:
        raise DTError("%s: order must be True or a RayOrder of these %d rays, on their side" % (what, n))
    return order


def trace_rays(scene, g, start, dir, planes=RAY_PLANES, out=None, stream=None, order=None):
    """Closest hits of caller-supplied rays (include/dt.h dt_trace_rays): start and dir are float64, shaped
    (n, 3) or flat, numpy arrays or torch tensors, both on one side. Returns (hits, stats): hits is a dict
    plane name -> array on the side of start for the planes asked for: shape (int32, -1: none), t (float32
    along the unnormalised dir, FLT_MAX: none), point, normal and albedo (float64, (n, 3); zeros on a miss).
    `out`: a dict of planes to write into instead (it decides the planes). 64 consecutive rays share a
    wave: keep neighbours in the arrays neighbours in space, or pass `order` (True, or a RayOrder of these
    rays from ray_order): the rays are gathered into sorted order, traced, and every answer is put back in
    the caller's order -- the same bits. g: the globals of the scene's renders."""
    n, sp, dp, side = _ray_arrays("trace_rays", start, dir)
    if out is None:
        for name in planes:
            if name not in RAY_PLANES:
                raise DTError("trace_rays: unknown plane %r" % (name,))
        out = {name: _ray_new(start, (n,) if _RAY_PLANE_TYPES[name][2] == 1 else (n, 3), *_RAY_PLANE_TYPES[name][:2])
               for name in planes}
    from ._lib import RayHits
    h = RayHits()
    for name, a in out.items():
        if name not in RAY_PLANES:
            raise DTError("trace_rays: unknown plane %r" % (name,))
        tt, nt, per = _RAY_PLANE_TYPES[name]
        setattr(h, name, _ray_out("trace_rays", name, a, n, per, tt, nt, side))
    if order is not None:
        order = _order_for("trace_rays", order, start, dir, n, side, stream)
        tmp = {name: _ray_new(start, tuple(a.shape), *_RAY_PLANE_TYPES[name][:2]) for name, a in out.items()}
        _, st = trace_rays(scene, g, order.apply(start), order.apply(dir), out=tmp, stream=stream)
        for name, a in out.items():
            order.restore(tmp[name], out=a)
        return out, st
    st = Stats()
    check(lib.dt_trace_rays(scene.handle, ctypes.byref(g), n, sp, dp, ctypes.byref(h), side,
                            ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)), "dt_trace_rays")
    return out, st


def rays_occluded(scene, g, start, dir, skip_shape=None, out=None, stream=None, order=None):
    """Is start + dir hidden from start (include/dt.h dt_rays_occluded)? start and dir as for trace_rays;
    skip_shape: optional int32 per ray on the same side, the shape the test leaves out (-1: none), such as
    the shape a light is. Returns (occluded, stats): uint8 per ray (1 or 0) on the side of start, or `out`.
    A wave is served in groups of equal skip_shape: group the rays by it where it varies. `order` as for
    trace_rays: the rays and skip_shape are gathered into sorted order and the answer is put back."""
    n, sp, dp, side = _ray_arrays("rays_occluded", start, dir)
    kp = None
    if skip_shape is not None:
        kp = _ray_out("rays_occluded", "skip_shape", skip_shape, n, 1, "torch.int32", "int32", side)
    if out is None:
        out = _ray_new(start, (n,), "torch.uint8", "uint8")
    op = _ray_out("rays_occluded", "out", out, n, 1, "torch.uint8", "uint8", side)
    if order is not None:
        order = _order_for("rays_occluded", order, start, dir, n, side, stream)
        tmp, st = rays_occluded(scene, g, order.apply(start), order.apply(dir),
                                skip_shape=order.apply(skip_shape) if skip_shape is not None else None, stream=stream)
        order.restore(tmp, out=out)
        return out, st
    st = Stats()
    check(lib.dt_rays_occluded(scene.handle, ctypes.byref(g), n, sp, dp, kp, op, side,
                               ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)), "dt_rays_occluded")
    return out, st


RAY_MULTI_PLANES = ("count", "shape", "t", "point", "normal", "albedo")
DT_MAT_GLASS = 1   # include/dt.h


def _restore_wide(order, tmp, out):
    """out[perm[i]] = tmp[i] for rows wider than dt_permute_rows takes (64 bytes), by the arrays' own indexing"""
    if hasattr(tmp, "data_ptr"):
        out.index_copy_(0, order.perm.long(), tmp)
    else:
        import numpy as np
        out[order.perm.astype(np.int64)] = tmp
    return out


def trace_rays_multi(scene, g, start, dir, k=4, planes=("count", "shape", "t"), order=None, stream=None):
    """The k nearest surfaces along caller-supplied rays (include/dt.h dt_trace_rays_multi): start and dir as for
    trace_rays, k in 1..8. Returns (hits, stats): hits is a dict plane name -> array on the side of start for
    the planes asked for: count (int32, (n,): hits recorded, 0..k), shape (int32, (n, k): the shape ranked j,
    -1 beyond count), t (float32, (n, k), FLT_MAX beyond count), point, normal and albedo (float64, (n, k, 3),
    zeros beyond count). Every gathered shape is tested on its own and gives at most one hit, its first
    intersection; hits are ranked by t, equal t by shape index. `order` as for trace_rays (True, or a RayOrder of
    these rays): the rays are gathered into sorted order, traced, and every answer is put back in the caller's
    order, the same bits -- by dt_permute_rows where a ray's row has at most 64 bytes, by the arrays' own
    indexing where it is wider (point, normal and albedo for k >= 3)."""
    what = "trace_rays_multi"
    n, sp, dp, side = _ray_arrays(what, start, dir)
    from ._lib import DT_MULTIHIT_MAX, RayMultiHits
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= DT_MULTIHIT_MAX:
        raise DTError("%s: k must be an integer in 1..%d, not %r" % (what, DT_MULTIHIT_MAX, k))
    for name in planes:
        if name not in RAY_MULTI_PLANES:
            raise DTError("%s: unknown plane %r" % (what, name))

    def new(name):
        if name == "count":
            return _ray_new(start, (n,), "torch.int32", "int32")
        tt, nt, per = _RAY_PLANE_TYPES[name]
        return _ray_new(start, (n, k) if per == 1 else (n, k, 3), tt, nt)

    out = {name: new(name) for name in planes}
    if order is not None:
        order = _order_for(what, order, start, dir, n, side, stream)
        tmp, st = trace_rays_multi(scene, g, order.apply(start), order.apply(dir), k=k, planes=planes, stream=stream)
        for name, a in out.items():
            row = _numel_any(a) * (a.element_size() if hasattr(a, "data_ptr") else a.itemsize) // n if n else 1
            if row <= 64:
                order.restore(tmp[name], out=a)
            else:
                _restore_wide(order, tmp[name], a)
        return out, st
    h = RayMultiHits()
    for name, a in out.items():
        setattr(h, name, _data_ptr(a))
    st = Stats()
    check(lib.dt_trace_rays_multi(scene.handle, ctypes.byref(g), n, sp, dp, k, ctypes.byref(h), side,
                                  ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)), "dt_trace_rays_multi")
    return out, st


RAY_TRANSMIT_PLANES = ("panes", "pane_shape")


def rays_transmittance(scene, g, start, dir, skip_shape=None, k=0, order=None, planes=RAY_TRANSMIT_PLANES,
                       stream=None):
    """rays_occluded with probes that pass through glass (include/dt.h dt_rays_transmittance): start, dir and
    skip_shape as for rays_occluded, k in 0..8. Returns (dict(panes=..., pane_shape=...), stats) on the side of
    start: `panes` int32 (n,), -1 where a shape that is not glass stops the probe, else the number of glass
    shapes it crosses (0: clear), so that (panes != 0) is rays_occluded's answer; `pane_shape` int32 (n, k), the
    k smallest indices of those glass shapes, ascending, -1 beyond (and all -1 for a blocked ray). With k = 0
    pane_shape is an empty (n, 0) array and no list is kept on the device. planes: which of the two to compute.
    `order` as for rays_occluded: the same bits."""
    what = "rays_transmittance"
    n, sp, dp, side = _ray_arrays(what, start, dir)
    from ._lib import DT_TRANSMIT_MAX_PANES, RayTransmittance
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= DT_TRANSMIT_MAX_PANES:
        raise DTError("%s: k must be an integer in 0..%d, not %r" % (what, DT_TRANSMIT_MAX_PANES, k))
    for name in planes:
        if name not in RAY_TRANSMIT_PLANES:
            raise DTError("%s: unknown plane %r" % (what, name))
    kp = None
    if skip_shape is not None:
        kp = _ray_out(what, "skip_shape", skip_shape, n, 1, "torch.int32", "int32", side)
    out = {}
    if "panes" in planes:
        out["panes"] = _ray_new(start, (n,), "torch.int32", "int32")
    if "pane_shape" in planes:
        out["pane_shape"] = _ray_new(start, (n, k), "torch.int32", "int32")
    if order is not None:
        order = _order_for(what, order, start, dir, n, side, stream)
        tmp, st = rays_transmittance(scene, g, order.apply(start), order.apply(dir),
                                     skip_shape=order.apply(skip_shape) if skip_shape is not None else None, k=k,
                                     planes=planes, stream=stream)
        for name, a in out.items():
            if _numel_any(a):
                order.restore(tmp[name], out=a)
        return out, st
    h = RayTransmittance()
    if "panes" in out:
        h.panes = _data_ptr(out["panes"])
    if "pane_shape" in out and k > 0:
        h.pane_shape = _data_ptr(out["pane_shape"])
    st = Stats()
    check(lib.dt_rays_transmittance(scene.handle, ctypes.byref(g), n, sp, dp, kp, k, ctypes.byref(h), side,
                                    ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)),
          "dt_rays_transmittance")
    return out, st


RAY_PATH_PLANES = ("end", "segments", "shape", "length", "point", "normal", "albedo", "last_start", "last_dir",
                   "seg_shape", "seg_point")
# plane -> (torch dtype, numpy dtype, values per entry, per segment)
_RAY_PATH_TYPES = {"end": ("torch.int32", "int32", 1, False), "segments": ("torch.int32", "int32", 1, False),
                   "shape": ("torch.int32", "int32", 1, False), "length": ("torch.float64", "float64", 1, False),
                   "point": ("torch.float64", "float64", 3, False), "normal": ("torch.float64", "float64", 3, False),
                   "albedo": ("torch.float64", "float64", 3, False),
                   "last_start": ("torch.float64", "float64", 3, False),
                   "last_dir": ("torch.float64", "float64", 3, False),
                   "seg_shape": ("torch.int32", "int32", 1, True), "seg_point": ("torch.float64", "float64", 3, True)}


def trace_rays_path(scene, g, start, dir, max_bounces=4, planes=("end", "segments", "shape", "point"), order=None,
                    stream=None):
    """Caller-supplied rays followed through mirrors and glass (include/dt.h dt_trace_rays_path): start and dir as
    for trace_rays, max_bounces in 0..8. Every ray runs render_features' specular-path chain (guide_bounce) with
    itself as segment 0. Returns (paths, stats): paths is a dict plane name -> array on the side of start for the
    planes asked for: end (int32: DT_PATH_VOID, _MISS, _SURFACE, _CUT), segments (int32, the segments traced),
    shape (int32, the shape the path ended on, -1: none), length (float64, the whole path's), point, normal,
    albedo (float64 (n, 3): the terminal hit's, zeros unless the path ended on a shape), last_start, last_dir
    (float64 (n, 3): the ray of the last segment traced), and per segment seg_shape (int32 (n, max_bounces+1),
    -1: not traced or a miss) and seg_point (float64 (n, max_bounces+1, 3)). paths["start"] is the caller's start
    as (n, 3), for ray_polyline. `order` as for trace_rays (True, or a RayOrder of these rays): the same bits.
    Geometry only: glossy reflectors (nogloss = 0) stop the chain, glass follows transmission, no Fresnel weights."""
    what = "trace_rays_path"
    n, sp, dp, side = _ray_arrays(what, start, dir)
    from ._lib import DT_RAY_PATH_MAX_BOUNCES, RayPaths
    K = max_bounces
    if isinstance(K, bool) or not isinstance(K, int) or not 0 <= K <= DT_RAY_PATH_MAX_BOUNCES:
        raise DTError("%s: max_bounces must be an integer in 0..%d, not %r" % (what, DT_RAY_PATH_MAX_BOUNCES, K))
    for name in planes:
        if name not in RAY_PATH_PLANES:
            raise DTError("%s: unknown plane %r" % (what, name))

    def new(name):
        tt, nt, per, seg = _RAY_PATH_TYPES[name]
        return _ray_new(start, (n,) + ((K + 1,) if seg else ()) + ((3,) if per == 3 else ()), tt, nt)

    out = {name: new(name) for name in planes}
    if order is not None:
        order = _order_for(what, order, start, dir, n, side, stream)
        tmp, st = trace_rays_path(scene, g, order.apply(start), order.apply(dir), max_bounces=K, planes=planes,
                                  stream=stream)
        for name, a in out.items():
            row = _numel_any(a) * (a.element_size() if hasattr(a, "data_ptr") else a.itemsize) // n if n else 1
            if row <= 64:
                order.restore(tmp[name], out=a)
            else:
                _restore_wide(order, tmp[name], a)
    else:
        h = RayPaths()
        for name, a in out.items():
            setattr(h, name, _data_ptr(a))
        st = Stats()
        check(lib.dt_trace_rays_path(scene.handle, ctypes.byref(g), n, sp, dp, K, ctypes.byref(h), side,
                                     ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)),
              "dt_trace_rays_path")
    out["start"] = start.reshape(n, 3)
    return out, st


def ray_polyline(paths, i):
    """The vertices of ray i of trace_rays_path's answer (which must hold seg_shape and seg_point): its start,
    then the hit point of every segment that hit a shape, in order -- a float64 numpy array (m, 3), m >= 1. A
    path that ended as a miss leaves along paths["last_dir"] from its last vertex."""
    import numpy as np
    for name in ("seg_shape", "seg_point", "start"):
        if name not in paths:
            raise DTError("ray_polyline: paths holds no %r (ask trace_rays_path for seg_shape and seg_point)" % name)

    def host(a):
        return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)

    shape, point = host(paths["seg_shape"][i]), host(paths["seg_point"][i])
    return np.concatenate([host(paths["start"][i]).reshape(1, 3), point[shape >= 0].reshape(-1, 3)]).astype(np.float64)


def pick(scene, g, frame, x, y, max_bounces=4):
    """What the pixel (x, y) of the frame shows, mirrors and panes followed: sample 0's camera ray of the pixel
    (camera_rays; x from the left, y from the top, as in the written images) through trace_rays_path with every
    plane. Returns (paths, stats) of that one ray: paths["shape"][0] is the shape seen, ray_polyline(paths, 0) the
    way there. Only that pixel's camera ray is made (a one-pixel window of camera_rays; the arrays it fills are
    the frame's)."""
    x, y = int(x), int(y)
    if not (0 <= x < g.xRes and 0 <= y < g.yRes):
        raise DTError("pick: pixel (%d, %d) outside the %d x %d frame" % (x, y, g.xRes, g.yRes))
    py = g.yRes - 1 - y   # the window counts rows from the bottom, the image's slots from the top
    start, dir = camera_rays(g, frame, samples=(0, 1), tile=tiles(x0=x, y0=py, x1=x + 1, y1=py + 1))
    q = y * g.xRes + x
    return trace_rays_path(scene, g, start[q, 0].reshape(1, 3).contiguous(), dir[q, 0].reshape(1, 3).contiguous(),
                           max_bounces=max_bounces, planes=RAY_PATH_PLANES)


def segment_through_glass(scene, desc, g, start, dir, k=8):
    """Is the segment start .. start + dir clear but for glass? Over trace_rays_multi(k): per ray `clear` (every
    recorded hit with t < 1 is on a DT_MAT_GLASS shape of desc), `panes` (how many such hits on glass) and
    `truncated` (count == k and all k hits are glass with t < 1: more surfaces may follow on the segment, so
    clear and panes are a lower bound only; ask again with a larger k, up to 8). Returns ({clear, panes,
    truncated}, stats) as numpy arrays (bool, int32, bool).
    For callers that want light or line of sight through the panes of a scene, which rays_occluded cannot give
    (a pane shadows like a wall there). It is not the light loop's test, and differs from rays_occluded: no
    1e-3 offset of the start, the shapes' intersect and not intersectShadow, no skip_shape, and every shape
    counts once (its first intersection; the far side of a glass sphere is not a second pane).
    rays_transmittance is the light loop's test with the glass filter, on the device: intersectShadow from the
    1e-3 offset up to t_max, skip_shape, never truncated (panes is a full count, blocked is exact), and usable
    inside points_occlusion(through_glass=...). This function stays for callers that want the closest-hit
    distances' view of the segment (t < 1 along the unnormalised dir)."""
    import numpy as np
    hits, st = trace_rays_multi(scene, g, start, dir, k=k, planes=("count", "shape", "t"))
    shape, t, count = hits["shape"], hits["t"], hits["count"]
    if hasattr(shape, "data_ptr"):
        shape, t, count = shape.cpu().numpy(), t.cpu().numpy(), count.cpu().numpy()
    glass = np.array([desc.shapes[i].material == DT_MAT_GLASS for i in range(desc.n_shapes)] + [False], bool)
    on_seg = (np.arange(k)[None, :] < count[:, None]) & (t < np.float32(1))
    is_glass = glass[shape]   # -1 (no hit) reads the appended False
    return {"clear": ~(on_seg & ~is_glass).any(axis=1),
            "panes": (on_seg & is_glass).sum(axis=1).astype(np.int32),
            "truncated": (count == k) & (on_seg & is_glass).all(axis=1)}, st


RESOLVE_MODES = {"mean": 0, "hit_mean": 1}   # DT_RESOLVE_MEAN, DT_RESOLVE_HIT_MEAN


def _sample_range(what, samples):
    try:
        b, e = (int(v) for v in samples)
    except (TypeError, ValueError):
        raise DTError("%s: samples must be a pair (begin, end), not %r" % (what, samples))
    return b, e


def camera_rays_rows(g, samples=(0, 1), tile=None):
    """Rows of camera_rays' arrays for (g, tile, samples): accum_doubles(g, tile) // 3 * (end - begin)."""
    b, e = _sample_range("camera_rays_rows", samples)
    n = int(lib.dt_camera_rays_rows(ctypes.byref(g), ctypes.byref(tile) if tile else None, b, e))
    if n < 0:
        raise DTError("camera_rays_rows: %s" % lib.dt_last_error().decode(errors="replace"))
    return n


def camera_rays(g, frame=0, samples=(0, 1), tile=None, out=None, stream=None, host=False):
    """The render's own camera rays as arrays (include/dt.h dt_camera_rays): for the samples begin .. end-1 of
    every owned pixel the ray render() starts that sample from, bit for bit. Returns (start, dir), float64,
    shaped (slots, ns, 3): slot q is the pixel whose colour sits at floats 3q..3q+2 of render's output (image
    or slab layout per `tile`), ns = end - begin. CUDA tensors by default, numpy arrays with host=True, zero-filled
    so that the rows of pixels the tile share does not own are void rays for the ray queries. `out`: a pair
    (start, dir) to write into instead, where only owned rows are written. No scene is needed. Only the
    thin-lens perspective camera of the renders; the motion-blur re-trace of frames >= frame_prism is not
    reproduced. Pass the arrays (reshaped to (-1, 3) or as they are) to trace_rays, rays_occluded,
    trace_rays_multi, and the answers to rays_resolve."""
    b, e = _sample_range("camera_rays", samples)
    ns = e - b
    rows = camera_rays_rows(g, (b, e), tile)
    if out is None:
        if host:
            import numpy as np
            out = (np.zeros((rows // ns, ns, 3), np.float64), np.zeros((rows // ns, ns, 3), np.float64))
        else:
            import torch
            out = (torch.zeros((rows // ns, ns, 3), dtype=torch.float64, device="cuda"),
                   torch.zeros((rows // ns, ns, 3), dtype=torch.float64, device="cuda"))
    start, dir = out
    sp, sdev = _ptr_typed(start, "torch.float64", "float64")
    dp, ddev = _ptr_typed(dir, "torch.float64", "float64")
    if sdev != ddev or _numel_any(start) != 3 * rows or _numel_any(dir) != 3 * rows:
        raise DTError("camera_rays: start and dir hold 3 doubles for each of the %d rows, on the same side" % rows)
    check(lib.dt_camera_rays(ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None, b, e, sp, dp, sdev,
                             ctypes.c_void_p(stream) if stream else None, None), "dt_camera_rays")
    return start, dir


def rays_resolve(g, values, n_samples, shape=None, mode="mean", tile=None, coverage=False, out=None, stream=None):
    """Per-ray answers back to per-pixel planes (include/dt.h dt_rays_resolve): values holds `width` (1..3)
    float64 per row in camera_rays' row order with n_samples rows per slot -- shaped (slots, n_samples, width),
    (rows, width) or, for width 1, (rows,). Per owned pixel and component the f64 sum of its rows, left to right,
    divided by n_samples (mode "mean") or by the number of rows that count ("hit_mean", 0 where none does);
    `shape` (int32 per row, such as trace_rays' shape plane): rows with shape < 0 add nothing and do not count.
    Returns the float32 plane shaped (slots, width), or (plane, coverage) with coverage=True (the rows that
    count / n_samples, float32 per slot), on the side of values (numpy, or the tensor's device); unowned pixels
    stay 0, or as they came in `out` (a plane, or a pair with coverage=True). f64 rows only."""
    what = "rays_resolve"
    n = int(n_samples)
    slots = accum_doubles(g, tile) // 3
    vp, side = _ptr_typed(values, "torch.float64", "float64")
    total = _numel_any(values)
    if n < 1 or slots * n == 0 or total % (slots * n) or not 1 <= total // (slots * n) <= 3:
        raise DTError("%s: values holds %d doubles, not 1..3 for each of %d slots x %d samples" % (what, total, slots, n))
    width = total // (slots * n)
    if mode not in RESOLVE_MODES:
        raise DTError("%s: mode must be one of %s, not %r" % (what, sorted(RESOLVE_MODES), mode))
    hp = _ray_out(what, "shape", shape, slots * n, 1, "torch.int32", "int32", side) if shape is not None else None
    plane, cov = (out if coverage else (out, None)) if out is not None else (None, None)
    if plane is None:
        plane = _ray_new(values, (slots, width), "torch.float32", "float32")
    if coverage and cov is None:
        cov = _ray_new(values, (slots,), "torch.float32", "float32")
    pp = _ray_out(what, "out", plane, slots, width, "torch.float32", "float32", side)
    cp = _ray_out(what, "coverage", cov, slots, 1, "torch.float32", "float32", side) if coverage else None
    check(lib.dt_rays_resolve(ctypes.byref(g), ctypes.byref(tile) if tile else None, n, width, vp, hp,
                              RESOLVE_MODES[mode], pp, cp, side, ctypes.c_void_p(stream) if stream else None), "dt_rays_resolve")
    return (plane, cov) if coverage else plane


def peel_layers(scene, g, frame, k=4, n_samples=1, planes=("albedo",)):
    """Depth peeling of the render's own view, a worked consumer of camera_rays -> trace_rays_multi ->
    rays_resolve: layer j is what the camera's rays meet as their (j+1)-th surface. Returns a dict of numpy
    arrays in image row order (row 0 is the top row, as in the written images): for each plane asked for
    ("albedo", "normal") an array (k, yRes, xRes, 3), the mean over the pixel's n_samples rays of the rank-j
    hit's value, a ray with fewer than j+1 hits adding nothing (coverage-premultiplied); and "coverage"
    (k, yRes, xRes), the fraction of the pixel's rays with a rank-j hit. Whole frames."""
    import torch
    for name in planes:
        if name not in ("albedo", "normal"):
            raise DTError("peel_layers: unknown plane %r" % (name,))
    n = int(n_samples)
    start, dir = camera_rays(g, frame, samples=(0, n))
    hits, _ = trace_rays_multi(scene, g, start.view(-1, 3), dir.view(-1, 3), k=k, planes=("shape",) + tuple(planes))
    W, H = g.xRes, g.yRes
    out = {name: torch.zeros((k, H * W, 3), dtype=torch.float32, device="cuda") for name in planes}
    cov = torch.zeros((k, H * W), dtype=torch.float32, device="cuda")
    for j in range(k):
        shape_j = hits["shape"][:, j].contiguous()
        for name in planes:
            rays_resolve(g, hits[name][:, j, :].contiguous(), n, shape=shape_j, out=(out[name][j], cov[j]), coverage=True)
        if not planes:
            rays_resolve(g, torch.zeros(H * W * n, dtype=torch.float64, device="cuda"), n, shape=shape_j,
                         out=(torch.zeros((H * W, 1), dtype=torch.float32, device="cuda"), cov[j]), coverage=True)
    res = {name: a.cpu().numpy().reshape(k, H, W, 3) for name, a in out.items()}
    res["coverage"] = cov.cpu().numpy().reshape(k, H, W)
    return res


def feature_images(g, feats):
    """The four 8-bit feature images as `dtrender --features` writes them, from full-frame image-layout
    planes (numpy float32): {"albedo": albedo*255, "normal": (normal*0.5 + 0.5*coverage)*255,
    "depth": depth / the frame's largest depth * 255 (grey), "coverage": coverage*255 (grey)}, each
    3 floats per pixel for write_png, clamped to 0..255. float32 arithmetic in this order."""
    import numpy as np
    f32 = np.float32
    cov = np.ascontiguousarray(feats["coverage"], dtype=f32)
    dep = np.ascontiguousarray(feats["depth"], dtype=f32)
    dmax = dep.max() if dep.size else f32(0)
    grey_d = (dep / dmax if dmax > 0 else np.zeros_like(dep)) * f32(255)
    img = {"albedo": np.ascontiguousarray(feats["albedo"], dtype=f32) * f32(255),
           "normal": (np.ascontiguousarray(feats["normal"], dtype=f32) * f32(0.5) + np.repeat(f32(0.5) * cov, 3)) * f32(255),
           "depth": np.repeat(grey_d, 3), "coverage": np.repeat(cov * f32(255), 3)}
    return {k: np.clip(v, f32(0), f32(255)) for k, v in img.items()}


def denoise_params_default():
    """dt_denoise_params_default: levels 5, demodulate 1 and the sigmas chosen in BASELINE.md."""
    from ._lib import DenoiseParams
    p = DenoiseParams()
    lib.dt_denoise_params_default(ctypes.byref(p))
    return p


def denoise_var_params_default():
    """dt_denoise_var_params_default: levels 5, demodulate 1 and the values chosen in BASELINE.md."""
    p = DenoiseVarParams()
    lib.dt_denoise_var_params_default(ctypes.byref(p))
    return p


_denoise_work = {}   # side (0 host, 1 + device index) -> the workspace last allocated there


def _denoise_workspace(n, dev, like):
    key = 0 if not dev else 1 + like.device.index
    w = _denoise_work.get(key)
    if w is None or (w.numel() if dev else w.size) < n:
        if dev:
            import torch
            w = torch.empty(n, dtype=torch.float32, device=like.device)
        else:
            import numpy as np
            w = np.empty(n, np.float32)
        _denoise_work[key] = w
    return w


def denoise(g, colour, feats, params=None, out=None, stream=None, variance=None):
    """The edge-avoiding a-trous filter of include/dt.h dt_denoise on a whole frame of g.xRes x g.yRes:
    colour (3 floats per pixel, as render / Progressive.image give it) and feats, a dict with the albedo,
    normal and depth planes of render_features (other planes are ignored), all numpy float32 arrays (the
    host loop) or all CUDA float32 tensors (the kernels, enqueued on `stream`). A tile share or a slab
    lacks its neighbours: gather the frame first. params: a DenoiseParams (None: denoise_params_default()).
    With variance, the plane variance() gives (3 floats per pixel, on the side of colour), the filter is
    dt_denoise_var, whose colour width follows every pixel's own noise, and params is a DenoiseVarParams
    (None: denoise_var_params_default()).
    Returns out (a new array or tensor unless given). The workspace is allocated once per side and kept;
    calls on one side must not overlap."""
    n_px = int(g.xRes) * int(g.yRes)
    cp, side = _ptr(colour)
    if variance is not None:
        if params is not None and not isinstance(params, DenoiseVarParams):
            raise DTError("denoise: with a variance plane params must be a DenoiseVarParams")
        vp, vdev = _ptr(variance)
        have = variance.numel() if hasattr(variance, "numel") else variance.size
        if have != 3 * n_px:
            raise DTError("denoise: variance holds %d elements, %dx%d needs %d" % (have, g.xRes, g.yRes, 3 * n_px))
        if vdev != side:
            raise DTError("denoise: colour and the variance plane must be on the same side")
    elif isinstance(params, DenoiseVarParams):
        raise DTError("denoise: a DenoiseVarParams needs a variance plane")
    from ._lib import Features
    f = Features()
    for name, need in (("albedo", 3 * n_px), ("normal", 3 * n_px), ("depth", n_px)):
        if name not in feats:
            raise DTError("denoise: the %s plane is missing" % name)
        a = feats[name]
        p, dev = _ptr(a)
        have = a.numel() if hasattr(a, "numel") else a.size
        if have != need:
            raise DTError("denoise: plane %s holds %d elements, %dx%d needs %d" % (name, have, g.xRes, g.yRes, need))
        if dev != side:
            raise DTError("denoise: colour and the planes must all be on the same side")
        setattr(f, name, p)
    have = colour.numel() if hasattr(colour, "numel") else colour.size
    if have != 3 * n_px:
        raise DTError("denoise: colour holds %d elements, %dx%d needs %d" % (have, g.xRes, g.yRes, 3 * n_px))
    if out is None:
        if side:
            import torch
            out = torch.empty_like(colour)
        else:
            import numpy as np
            out = np.empty(3 * n_px, np.float32)
    op, odev = _ptr(out)
    if odev != side or (out.numel() if hasattr(out, "numel") else out.size) != 3 * n_px:
        raise DTError("denoise: out must hold %d elements on the side of colour" % (3 * n_px))
    st = ctypes.c_void_p(stream) if stream else None
    if variance is not None:
        params = params if params is not None else denoise_var_params_default()
        n_work = int(lib.dt_denoise_var_workspace_floats(g.xRes, g.yRes, ctypes.byref(params)))
        if n_work < 0:
            check(n_work, "dt_denoise_var_workspace_floats")
        wp, _ = _ptr(_denoise_workspace(n_work, side, colour))
        check(lib.dt_denoise_var(g.xRes, g.yRes, cp, vp, ctypes.byref(f), ctypes.byref(params), op, wp, side, st, None),
              "dt_denoise_var")
        return out
    params = params if params is not None else denoise_params_default()
    n_work = int(lib.dt_denoise_workspace_floats(g.xRes, g.yRes, ctypes.byref(params)))
    if n_work < 0:
        check(n_work, "dt_denoise_workspace_floats")
    work = _denoise_workspace(n_work, side, colour)
    wp, _ = _ptr(work)
    check(lib.dt_denoise(g.xRes, g.yRes, cp, ctypes.byref(f), ctypes.byref(params), op, wp, side,
                         ctypes.c_void_p(stream) if stream else None, None), "dt_denoise")
    return out


_denoise = denoise   # (renderImage's denoise argument hides the name)


def upsample_params_default():
    """dt_upsample_params_default: factor 2, demodulate 1 and the sigmas chosen in BASELINE.md."""
    p = UpsampleParams()
    lib.dt_upsample_params_default(ctypes.byref(p))
    return p


def low_res_globals(g, factor):
    """A copy of g with xRes and yRes divided by factor (DTError if they do not divide); everything else,
    the seed and `aspect` included, unchanged: low-resolution pixel (x, y) covers exactly the factor x factor
    full-resolution pixels from (factor*x, factor*y)."""
    factor = int(factor)
    if factor < 1 or g.xRes % factor or g.yRes % factor:
        raise DTError("low_res_globals: %dx%d is not a multiple of factor %d" % (g.xRes, g.yRes, factor))
    lo = g.copy()
    lo.xRes, lo.yRes = g.xRes // factor, g.yRes // factor
    return lo


def upsample(g_hi, colour_lo, feats_lo, feats_hi, params=None, out=None, stream=None):
    """The guided upsampling of include/dt.h dt_upsample to a whole frame of g_hi.xRes x g_hi.yRes: colour_lo
    (3 floats per pixel, as render / denoise give it) and feats_lo at the resolution of
    low_res_globals(g_hi, params.factor), feats_hi at g_hi's; each feats a dict with the albedo, normal and
    depth planes of render_features (other planes are ignored). All numpy float32 arrays (the host loop) or
    all CUDA float32 tensors (the kernel, enqueued on `stream`). params: an UpsampleParams (None:
    upsample_params_default()). Returns out (a new array or tensor unless given)."""
    params = params if params is not None else upsample_params_default()
    s = int(params.factor)
    W, H = int(g_hi.xRes), int(g_hi.yRes)
    if s < 2 or s > 4:
        raise DTError("upsample: factor outside 2..4")
    if W < 1 or H < 1 or W % s or H % s:   # (the plane sizes below divide by s)
        raise DTError("upsample: %dx%d is not a multiple of factor %d" % (W, H, s))
    n_hi, n_lo = W * H, (W // s) * (H // s)
    cp, side = _ptr(colour_lo)
    from ._lib import Features
    fl, fh = Features(), Features()
    for f, feats, which, n_px in ((fl, feats_lo, "feats_lo", n_lo), (fh, feats_hi, "feats_hi", n_hi)):
        for name, need in (("albedo", 3 * n_px), ("normal", 3 * n_px), ("depth", n_px)):
            if name not in feats:
                raise DTError("upsample: the %s plane of %s is missing" % (name, which))
            a = feats[name]
            p, dev = _ptr(a)
            if _numel_any(a) != need:
                raise DTError("upsample: plane %s of %s holds %d elements, needs %d" % (name, which, _numel_any(a), need))
            if dev != side:
                raise DTError("upsample: colour_lo and the planes must all be on the same side")
            setattr(f, name, p)
    if _numel_any(colour_lo) != 3 * n_lo:
        raise DTError("upsample: colour_lo holds %d elements, %dx%d needs %d" % (_numel_any(colour_lo), W // s, H // s, 3 * n_lo))
    if out is None:
        if side:
            import torch
            out = torch.empty(3 * n_hi, dtype=torch.float32, device=colour_lo.device)
        else:
            import numpy as np
            out = np.empty(3 * n_hi, np.float32)
    op, odev = _ptr(out)
    if odev != side or _numel_any(out) != 3 * n_hi:
        raise DTError("upsample: out must hold %d elements on the side of colour_lo" % (3 * n_hi))
    check(lib.dt_upsample(W, H, cp, ctypes.byref(fl), ctypes.byref(fh), ctypes.byref(params), op, side,
                          ctypes.c_void_p(stream) if stream else None, None), "dt_upsample")
    return out


_upsample = upsample   # (renderImage's upsample argument hides the name)


def camera(g):
    """dt_camera_get: the camera the renders of g use, as a Camera record (host only)."""
    c = Camera()
    check(lib.dt_camera_get(ctypes.byref(g), ctypes.byref(c)), "dt_camera_get")
    return c


def temporal_params_default():
    """dt_temporal_params_default: demodulate 1 and the values chosen in BASELINE.md."""
    p = TemporalParams()
    lib.dt_temporal_params_default(ctypes.byref(p))
    return p


def _numel(a):
    return a.numel() if hasattr(a, "numel") else a.size


def _new_like(like, n, side):
    if side:
        import torch
        return torch.empty(n, dtype=torch.float32, device=like.device)
    import numpy as np
    return np.empty(n, np.float32)


def reproject(cur_cam, colour, feats, prev_cam, prev_feats, history, params=None, variance=None, stream=None,
              out=None, out_history=None, out_var=None, timed=False):
    """include/dt.h dt_reproject, one call per frame: the current frame (its Camera, colour, the albedo, normal
    and depth planes of render_features in the dict feats, optionally shape, optionally the variance plane) is
    blended with the history found by reprojecting every pixel into the previous frame (prev_cam, the dict
    prev_feats with albedo, normal, depth and optionally shape, and the dict `history` with colour, len and, iff
    variance is given, var: what the previous call returned). prev_cam, prev_feats and history all None: the
    first frame of a sequence. Whole frames; all numpy float32 arrays (the host loop) or all CUDA float32
    tensors (the kernel, enqueued on `stream`). Returns (out, history', out_var): out_var is None without
    variance. out, out_history, out_var: buffers to write into (new ones otherwise); nothing may alias an
    input. timed: the kernel is timed with events, the call synchronises and returns a fourth value, its ms."""
    from ._lib import Features, History
    W, H = int(cur_cam.xRes), int(cur_cam.yRes)
    n_px = W * H
    cp, side = _ptr(colour)

    def plane(a, need, what, shape=False):
        p, dev = _ptr_typed(a, "torch.int32", "int32") if shape else _ptr(a)
        if _numel(a) != need:
            raise DTError("reproject: %s holds %d elements, %dx%d needs %d" % (what, _numel(a), W, H, need))
        if dev != side:
            raise DTError("reproject: colour and %s must be on the same side" % what)
        return p

    plane(colour, 3 * n_px, "colour")
    vp = plane(variance, 3 * n_px, "variance") if variance is not None else None

    def features(d, names, what):
        f = Features()
        for name in names:
            if name not in d:
                raise DTError("reproject: %s lacks the %s plane" % (what, name))
            setattr(f, name, plane(d[name], n_px if name == "depth" else 3 * n_px, "%s[%s]" % (what, name)))
        if d.get("shape") is not None:
            f.shape = plane(d["shape"], n_px, "%s[shape]" % what, shape=True)
        return f

    def record(d, what):
        h = History()
        for name in ("colour", "len") + (("var",) if variance is not None else ()):
            if d.get(name) is None:
                raise DTError("reproject: %s lacks the %s plane" % (what, name))
            setattr(h, name, plane(d[name], n_px if name == "len" else 3 * n_px, "%s[%s]" % (what, name)))
        return h

    f = features(feats, ("albedo", "normal", "depth"), "feats")
    given = [prev_cam is not None, prev_feats is not None, history is not None]
    if any(given) and not all(given):
        raise DTError("reproject: prev_cam, prev_feats and history go together (all None: the first frame)")
    pf = features(prev_feats, ("albedo", "normal", "depth"), "prev_feats") if given[0] else None
    hin = record(history, "history") if given[0] else None
    if out is None:
        out = _new_like(colour, 3 * n_px, side)
    if out_history is None:
        out_history = {"colour": _new_like(colour, 3 * n_px, side), "len": _new_like(colour, n_px, side)}
        if variance is not None:
            out_history["var"] = _new_like(colour, 3 * n_px, side)
    if variance is not None and out_var is None:
        out_var = _new_like(colour, 3 * n_px, side)
    op = plane(out, 3 * n_px, "out")
    ovp = plane(out_var, 3 * n_px, "out_var") if variance is not None else None
    hout = record(out_history, "out_history")
    params = params if params is not None else temporal_params_default()
    ms = ctypes.c_float(0)
    check(lib.dt_reproject(ctypes.byref(cur_cam), cp, vp, ctypes.byref(f),
                           ctypes.byref(prev_cam) if given[0] else None, ctypes.byref(pf) if given[0] else None,
                           ctypes.byref(hin) if given[0] else None, ctypes.byref(params), op, ovp, ctypes.byref(hout),
                           side, ctypes.c_void_p(stream) if stream else None, ctypes.byref(ms) if timed else None),
          "dt_reproject")
    res = (out, out_history, out_var if variance is not None else None)
    return res + (ms.value,) if timed else res


class TemporalAccumulator:
    """Carries the history of dt_reproject from frame to frame: the two ping-ponged history records, the
    previous frame's camera and its albedo, normal, depth and shape planes (copies: the caller may reuse its buffers).

        acc = TemporalAccumulator()
        for each frame, in order:  out = acc.push(g, prog.image(), prog.features())
                                   clean = denoise(g, out, feats)

    push(g, colour, feats, variance=None) returns the accumulated frame (a new array or tensor), or
    (out, out_var) with a variance plane; the first push, a push after reset(), one at another resolution, on
    the other side or with / without variance where the last one differed starts a new sequence.
    history_length(): the float plane of frames accumulated per pixel (None before the first push)."""

    def __init__(self, params=None):
        self.params = params if params is not None else temporal_params_default()
        self.reset()

    def reset(self):
        self._cam = self._feats = self._hist = self._spare = None

    def history_length(self):
        return None if self._hist is None else self._hist["len"]

    @staticmethod
    def _copy(a):
        return a.clone() if hasattr(a, "clone") else a.copy()

    def push(self, g, colour, feats, variance=None, stream=None):
        cam = camera(g)
        side = 1 if getattr(colour, "is_cuda", False) else 0
        key = (cam.xRes, cam.yRes, side, variance is not None)
        if self._cam is not None and self._key != key:
            self.reset()
        self._key = key
        if self._spare is not None and ("var" in self._spare) != (variance is not None):
            self._spare = None
        out, hist, out_var = reproject(cam, colour, feats, self._cam, self._feats, self._hist, self.params,
                                       variance=variance, stream=stream, out_history=self._spare)
        self._spare, self._hist = self._hist, hist
        self._cam = cam
        self._feats = {k: self._copy(feats[k]) for k in ("albedo", "normal", "depth", "shape") if feats.get(k) is not None}
        return (out, out_var) if variance is not None else out


def render_sky(g, frame, out, tile=None, stream=None):
    """renderImageCloud's pixel loop (sky only) into `out`."""
    st = Stats()
    p, dev = _ptr(out)
    check(lib.dt_render_sky(ctypes.byref(g), float(frame), ctypes.byref(tile) if tile else None, p, dev,
                            ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)), "dt_render_sky")
    return st


def slab_floats(g, tile):
    return int(lib.dt_slab_floats(ctypes.byref(g), ctypes.byref(tile)))


def slab_floats_max(g, tile):
    return int(lib.dt_slab_floats_max(ctypes.byref(g), ctypes.byref(tile)))


def unpack_slabs(g, tile, world, slabs, image, stream=None):
    sp, sdev = _ptr(slabs)
    ip, idev = _ptr(image)
    if sdev != idev:
        raise DTError("slabs and image must be on the same side")
    check(lib.dt_unpack_slabs(ctypes.byref(g), ctypes.byref(tile), int(world), sp, ip, idev,
                              ctypes.c_void_p(stream) if stream else None), "dt_unpack_slabs")


def _spp(g):
    """sampled_n = int(sqrt(antialias_samples))^2 (cpp:1046,1061; host_flatten.cpp fill_params)"""
    import math
    n = int(math.sqrt(float(g.antialias_samples)))
    return n * n


def accum_doubles(g, tile=None):
    """Length of the f64 accumulator of window renders for (g, tile): one double per float of the
    output, in its layout (dt_accum_doubles)."""
    n = int(lib.dt_accum_doubles(ctypes.byref(g), ctypes.byref(tile) if tile else None))
    if n < 0:
        raise DTError("dt_accum_doubles: invalid globals or tiles")
    return n


def window_check(g, begin, end):
    """Raise DTError unless [begin, end) is a sample window (include/dt.h dt_window_check)."""
    check(lib.dt_window_check(ctypes.byref(g), int(begin), int(end)), "dt_window_check")


def _accum_ptr(accum, g, tile):
    if not hasattr(accum, "data_ptr") or str(accum.dtype) != "torch.float64" or not accum.is_cuda \
            or not accum.is_contiguous():
        raise DTError("the accumulator must be a contiguous CUDA torch.float64 tensor")
    if accum.numel() < accum_doubles(g, tile):
        raise DTError("the accumulator holds %d doubles, (g, tile) need %d" % (accum.numel(), accum_doubles(g, tile)))
    return ctypes.c_void_p(accum.data_ptr())


def render_window(scene, g, frame, accum, begin, end, tile=None, stream=None):
    """Add the samples [begin, end) of every owned pixel onto `accum`, in sample order
    (dt_render_window). The caller orders the windows: ascending, gap-free, from 0 on a zeroed
    accumulator reproduces dt_render's sums bit for bit. Returns the window's Stats."""
    st = Stats()
    check(lib.dt_render_window(scene.handle, ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None,
                               int(begin), int(end), _accum_ptr(accum, g, tile),
                               ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)), "dt_render_window")
    return st


def render_window_async(scene, g, frame, accum, begin, end, tile=None, stream=None):
    """render_window, enqueue only (collect_stats then reports the window)."""
    check(lib.dt_render_window_async(scene.handle, ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None,
                                     int(begin), int(end), _accum_ptr(accum, g, tile),
                                     ctypes.c_void_p(stream) if stream else None), "dt_render_window_async")


def resolve(g, accum, n_samples, out, tile=None, stream=None):
    """out[i] = clamp01(float32(accum[i] / n_samples)) * 255 (dt_resolve): torch CUDA tensors (a
    kernel) or host numpy / torch arrays (a loop), both on the same side. Returns the number of
    pixels with a NaN channel."""
    ap, adev = _ptr_typed(accum, "torch.float64", "float64")
    op, odev = _ptr(out)
    if adev != odev:
        raise DTError("accum and out must be on the same side")
    need = accum_doubles(g, tile)
    for a in (accum, out):
        if (a.numel() if hasattr(a, "numel") else a.size) < need:
            raise DTError("resolve: (g, tile) need %d elements" % need)
    nan = ctypes.c_uint64(0)
    check(lib.dt_resolve(ctypes.byref(g), ctypes.byref(tile) if tile else None, ap, int(n_samples), op, adev,
                         ctypes.c_void_p(stream) if stream else None, ctypes.byref(nan)), "dt_resolve")
    return nan.value


class Progressive:
    """A frame rendered in sample windows: a zeroed f64 accumulator on the device (24 B per pixel of
    the output layout) and the count of samples added so far.

        p = Progressive(scene, g, frame)
        while not p.done:
            p.step()              # the next 64-sample chunk of every pixel
            preview = p.image()   # the mean of the samples so far, as dt_render would store it

    After the last step image() is dt_render's output bit for bit. state() / restore() carry a frame
    across processes."""

    _STATE_INTS = ("samples_done", "frame", "seed", "xRes", "yRes", "spp")
    _TILE_FIELDS = ("x0", "y0", "x1", "y1", "tile_w", "tile_h", "rank", "world", "layout")

    def __init__(self, scene, g, frame, tile=None):
        import torch
        self.scene, self.g, self.frame = scene, g.copy(), int(frame)
        self.tile = tile if tile is not None else tiles()
        self.spp = _spp(g)
        self.samples_done = 0
        self.accum = torch.zeros(max(accum_doubles(self.g, self.tile), 1), dtype=torch.float64, device="cuda")

    @property
    def done(self):
        return self.samples_done >= self.spp

    def step(self, n_chunks=1):
        """Render the next window: n_chunks 64-sample chunks (the rest of the frame if fewer are
        left; with spp < 64 the one window [0, spp)). Returns the window's Stats."""
        if self.done:
            raise DTError("Progressive.step: all %d samples are rendered" % self.spp)
        if n_chunks < 1:
            raise DTError("Progressive.step: n_chunks < 1")
        begin = self.samples_done
        end = min(begin + 64 * int(n_chunks), self.spp)
        st = render_window(self.scene, self.g, self.frame, self.accum, begin, end, self.tile)
        self.samples_done = end
        return st

    def image(self, out=None):
        """The resolved preview: the mean of the samples rendered so far (a CUDA float32 tensor in
        the output layout; `out` to reuse one)."""
        import torch
        if self.samples_done < 1:
            raise DTError("Progressive.image: no window rendered yet")
        if out is None:
            out = torch.empty(self.accum.numel(), dtype=torch.float32, device="cuda")
        self.nan_pixels = resolve(self.g, self.accum, self.samples_done, out, self.tile)
        return out

    def features(self, planes=FEATURE_PLANES, specular_bounces=0):
        """The first-hit feature buffers of the samples rendered so far (render_features of the leading
        samples_done samples of every owned pixel, in the accumulator's layout; with adaptive sampling
        of every pixel alike, whether or not it has stopped). specular_bounces=K: the specular-path
        buffers of those samples, as render_features takes it."""
        if self.samples_done < 1:
            raise DTError("Progressive.features: no window rendered yet")
        return render_features(self.scene, self.g, self.frame, self.samples_done, self.tile, planes=planes,
                               specular_bounces=specular_bounces)

    def occlusion(self, ao_rays=4, ao_radius=None, lights=()):
        """The occlusion feature buffers of the samples rendered so far (render_occlusion of the leading
        samples_done samples of every owned pixel, in the accumulator's layout), as features() covers them:
        (planes, stats)."""
        if self.samples_done < 1:
            raise DTError("Progressive.occlusion: no window rendered yet")
        return render_occlusion(self.scene, self.g, self.frame, self.samples_done, ao_rays, ao_radius, lights, self.tile)

    def mattes(self, groups=None, layers=4):
        """The object mattes of the samples rendered so far (render_mattes of the leading samples_done
        samples of every owned pixel, in the accumulator's layout), as features() covers them."""
        if self.samples_done < 1:
            raise DTError("Progressive.mattes: no window rendered yet")
        return render_mattes(self.scene, self.g, self.frame, self.samples_done, groups, layers, self.tile)

    def _variance_plane(self):
        raise DTError("Progressive.denoised(variance=True): the sums of squares live in AdaptiveProgressive; "
                      "with min_samples >= spp it never stops a pixel and renders this frame's bits")

    def denoised(self, params=None, out=None, variance=False):
        """The denoised preview: image() and features() of the samples so far through denoise(), on the
        device (a CUDA float32 tensor like image()). Whole frames only: a tile share or a slab lacks the
        neighbours the filter reads. The accumulator is not touched. variance=True (AdaptiveProgressive
        only: it keeps the sums of squares) filters with the per-pixel colour width of dt_denoise_var on
        variance(); params is then a DenoiseVarParams or None."""
        vplane = self._variance_plane() if variance else None
        t = self.tile
        if t.layout != DT_OUT_IMAGE or t.world != 1 or t.x0 != 0 or t.y0 != 0 \
                or (t.x1 > 0 and t.x1 < self.g.xRes) or (t.y1 > 0 and t.y1 < self.g.yRes):
            raise DTError("Progressive.denoised: needs the whole frame (DT_OUT_IMAGE, world 1, no window)")
        return denoise(self.g, self.image(), self.features(planes=("albedo", "normal", "depth")), params, out,
                       variance=vplane)

    def run(self, until=None, n_chunks=1):
        """step() until done, or until until(self) returns true after a step."""
        while not self.done:
            self.step(n_chunks)
            if until is not None and until(self):
                break
        return self

    def state(self):
        """Host copy of the frame so far: numpy f64 accumulator and ints (samples done, frame, seed,
        xRes, yRes, spp, the tile fields)."""
        d = {"accum": self.accum.cpu().numpy().copy(), "samples_done": int(self.samples_done),
             "frame": self.frame, "seed": int(self.g.seed), "xRes": int(self.g.xRes), "yRes": int(self.g.yRes),
             "spp": int(self.spp)}
        for f in self._TILE_FIELDS:
            d["tile_" + f] = int(getattr(self.tile, f))
        return d

    @classmethod
    def restore(cls, scene, g, state):
        """Continue the frame of state() on `scene` (a scene of the same description) with globals g:
        seed, resolution, spp and the tile must be the state's."""
        import numpy as np
        import torch
        tile = tiles(**{f: int(state["tile_" + f]) for f in cls._TILE_FIELDS})
        p = cls.__new__(cls)
        p.scene, p.g, p.frame, p.tile = scene, g.copy(), int(state["frame"]), tile
        p.spp = _spp(g)
        for k, have in (("seed", g.seed), ("xRes", g.xRes), ("yRes", g.yRes), ("spp", p.spp)):
            if int(state[k]) != int(have):
                raise DTError("Progressive.restore: %s is %d, the state was rendered with %d" % (k, have, state[k]))
        done = int(state["samples_done"])
        if done < 0 or done > p.spp or (done < p.spp and done % 64):
            raise DTError("Progressive.restore: samples_done %d is no window boundary" % done)
        acc = np.ascontiguousarray(state["accum"], dtype=np.float64).reshape(-1)
        if acc.size != max(accum_doubles(p.g, tile), 1):
            raise DTError("Progressive.restore: the accumulator holds %d doubles, (g, tile) need %d"
                          % (acc.size, accum_doubles(p.g, tile)))
        p.samples_done = done
        p.accum = torch.from_numpy(acc).to("cuda")
        return p


def adapt_converged(s1, s2, count, tol, min_samples=64):
    """The convergence rule of adaptive sampling on host values (dt_adapt_converged): s1, s2 the
    pixel's three sums of sample colours and of their squares, count the samples in them."""
    a = (ctypes.c_double * 3)(*[float(v) for v in s1])
    b = (ctypes.c_double * 3)(*[float(v) for v in s2])
    rc = lib.dt_adapt_converged(a, b, int(count), float(tol), int(min_samples))
    if rc < 0:
        check(rc, "dt_adapt_converged")
    return bool(rc)


def _count_ptr(count, g, tile):
    if not hasattr(count, "data_ptr") or str(count.dtype) != "torch.int32" or not count.is_cuda \
            or not count.is_contiguous():
        raise DTError("the sample counts must be a contiguous CUDA torch.int32 tensor (read as uint32)")
    if 3 * count.numel() < accum_doubles(g, tile):
        raise DTError("the sample counts hold %d entries, (g, tile) need %d" % (count.numel(), accum_doubles(g, tile) // 3))
    return ctypes.c_void_p(count.data_ptr())


def render_window_adaptive(scene, g, frame, accum, accum2, count, begin, end, tol, min_samples=64, tile=None,
                           stream=None):
    """render_window over the pixels that are live (count == begin) and have not converged
    (dt_render_window_adaptive): accum2 the sums of squared sample colours (float64, like accum),
    count the samples per pixel (int32 tensor, read as uint32). Returns the window's Stats: pixels is
    the number of pixels traced."""
    st = Stats()
    check(lib.dt_render_window_adaptive(scene.handle, ctypes.byref(g), int(frame), ctypes.byref(tile) if tile else None,
                                        int(begin), int(end), _accum_ptr(accum, g, tile), _accum_ptr(accum2, g, tile),
                                        _count_ptr(count, g, tile), float(tol), int(min_samples),
                                        ctypes.c_void_p(stream) if stream else None, ctypes.byref(st)),
          "dt_render_window_adaptive")
    return st


def adapt_select_ms(scene):
    """Device time of the selection kernels of the scene's last adaptive window launch."""
    ms = ctypes.c_float(0)
    check(lib.dt_adapt_select_ms(scene.handle, ctypes.byref(ms)), "dt_adapt_select_ms")
    return ms.value


def resolve_adaptive(g, accum, count, out, tile=None, stream=None):
    """out[3q+k] = clamp01(float32(accum[3q+k] / count[q])) * 255, 0 where count[q] is 0
    (dt_resolve_adaptive): all three on the same side; count int32 (torch) or uint32 / int32 (numpy).
    Returns the number of pixels with a NaN channel."""
    ap, adev = _ptr_typed(accum, "torch.float64", "float64")
    if hasattr(count, "data_ptr"):
        cp, cdev = _ptr_typed(count, "torch.int32", "int32")
    else:
        cp, cdev = _ptr_typed(count, "", "int32" if str(count.dtype) == "int32" else "uint32")
    op, odev = _ptr(out)
    if not adev == cdev == odev:
        raise DTError("accum, count and out must be on the same side")
    need = accum_doubles(g, tile)
    for a, k in ((accum, 1), (out, 1), (count, 3)):
        if k * (a.numel() if hasattr(a, "numel") else a.size) < need:
            raise DTError("resolve_adaptive: (g, tile) need %d elements" % (need // k))
    nan = ctypes.c_uint64(0)
    check(lib.dt_resolve_adaptive(ctypes.byref(g), ctypes.byref(tile) if tile else None, ap, cp, op, adev,
                                  ctypes.c_void_p(stream) if stream else None, ctypes.byref(nan)), "dt_resolve_adaptive")
    return nan.value


def variance(g, accum, accum2, count, out=None, tile=None, stream=None):
    """The variance of the mean of every channel's sample colours, in grey levels squared of the 0..255
    output (dt_variance): 0 where a pixel has fewer than two samples. accum, accum2 (float64) and count
    (int32 for torch, uint32 / int32 for numpy) as render_window_adaptive keeps them, all numpy arrays (a
    loop) or all CUDA tensors (a kernel, enqueued on `stream`). Returns out (float32, indexed like the
    accumulator and the colour image; a new array or tensor unless given)."""
    ap, adev = _ptr_typed(accum, "torch.float64", "float64")
    bp, bdev = _ptr_typed(accum2, "torch.float64", "float64")
    if hasattr(count, "data_ptr"):
        cp, cdev = _ptr_typed(count, "torch.int32", "int32")
    else:
        cp, cdev = _ptr_typed(count, "", "int32" if str(count.dtype) == "int32" else "uint32")
    need = accum_doubles(g, tile)
    if out is None:
        if adev:
            import torch
            out = torch.empty(max(need, 1), dtype=torch.float32, device=accum.device)
        else:
            import numpy as np
            out = np.empty(need, np.float32)
    op, odev = _ptr(out)
    if not adev == bdev == cdev == odev:
        raise DTError("variance: accum, accum2, count and out must be on the same side")
    for a, k in ((accum, 1), (accum2, 1), (out, 1), (count, 3)):
        if k * (a.numel() if hasattr(a, "numel") else a.size) < need:
            raise DTError("variance: (g, tile) need %d elements" % (need // k))
    check(lib.dt_variance(ctypes.byref(g), ctypes.byref(tile) if tile else None, ap, bp, cp, op, adev,
                          ctypes.c_void_p(stream) if stream else None), "dt_variance")
    return out


_variance = variance   # (denoised's variance argument hides the name)


class AdaptiveProgressive(Progressive):
    """Progressive with adaptive sampling: between windows, pixels whose mean has converged stop.

        p = AdaptiveProgressive(scene, g, frame, tol=0.5)
        p.run()
        img = p.image()             # every pixel the mean of its own samples
        share = p.samples_taken / (p.sample_counts().numel() * p.spp)

    tol is the standard error of a pixel's mean allowed, in grey levels of the 0..255 output; a pixel
    may stop once it has min_samples (and at least 64) samples. The state is three device buffers:
    accum, accum2 (sums of squares) and count (samples per pixel), 52 B per pixel; a pixel is live at
    a window iff its count is the window's begin. A pixel that never stops has the one-shot render's
    bits. done: a step traced no pixel, or all spp samples are rendered."""

    def __init__(self, scene, g, frame, tol, min_samples=64, tile=None):
        import torch
        super().__init__(scene, g, frame, tile)
        self.tol, self.min_samples = float(tol), int(min_samples)
        self.accum2 = torch.zeros_like(self.accum)
        self.count = torch.zeros(max(self.accum.numel() // 3, 1), dtype=torch.int32, device="cuda")
        self.active_pixels = None
        self._idle = False

    @property
    def done(self):
        return self._idle or self.samples_done >= self.spp

    def step(self, n_chunks=1):
        """Render the next window over the live, unconverged pixels. Returns the window's Stats."""
        if self.done:
            raise DTError("AdaptiveProgressive.step: the frame is done")
        if n_chunks < 1:
            raise DTError("AdaptiveProgressive.step: n_chunks < 1")
        begin = self.samples_done
        end = min(begin + 64 * int(n_chunks), self.spp)
        st = render_window_adaptive(self.scene, self.g, self.frame, self.accum, self.accum2, self.count, begin, end,
                                    self.tol, self.min_samples, self.tile)
        self.samples_done = end
        self.active_pixels = int(st.pixels)
        self._idle = st.pixels == 0
        return st

    def sample_counts(self):
        """The samples added per pixel so far (the count tensor: int32, in the accumulator's pixel order)."""
        return self.count

    @property
    def samples_taken(self):
        import torch
        return int(self.count.sum(dtype=torch.int64).item())

    def image(self, out=None):
        """The resolved image: every pixel the mean of its own samples (0 where it has none)."""
        import torch
        if self.samples_done < 1:
            raise DTError("AdaptiveProgressive.image: no window rendered yet")
        if out is None:
            out = torch.empty(self.accum.numel(), dtype=torch.float32, device="cuda")
        self.nan_pixels = resolve_adaptive(self.g, self.accum, self.count, out, self.tile)
        return out

    def variance(self, out=None):
        """The variance of the mean of every pixel's samples so far, per channel, in grey levels squared
        (variance(): a CUDA float32 tensor indexed like image(); 0 where a pixel has fewer than two samples)."""
        if self.samples_done < 1:
            raise DTError("AdaptiveProgressive.variance: no window rendered yet")
        return _variance(self.g, self.accum, self.accum2, self.count, out, self.tile)

    def _variance_plane(self):
        return self.variance()

    def state(self):
        d = super().state()
        d.update({"accum2": self.accum2.cpu().numpy().copy(), "count": self.count.cpu().numpy().copy(),
                  "tol": self.tol, "min_samples": self.min_samples})
        return d

    @classmethod
    def restore(cls, scene, g, state):
        import numpy as np
        import torch
        p = super().restore(scene, g, state)
        acc2 = np.ascontiguousarray(state["accum2"], dtype=np.float64).reshape(-1)
        cnt = np.ascontiguousarray(state["count"], dtype=np.int32).reshape(-1)
        if acc2.size != p.accum.numel() or cnt.size != max(p.accum.numel() // 3, 1):
            raise DTError("AdaptiveProgressive.restore: accum2 / count do not match the accumulator")
        p.accum2 = torch.from_numpy(acc2).to("cuda")
        p.count = torch.from_numpy(cnt).to("cuda")
        p.tol, p.min_samples = float(state["tol"]), int(state["min_samples"])
        p.active_pixels = None
        p._idle = False
        return p


def mean_abs_change(a, b):
    """Mean absolute difference of two resolved images (torch): an early-stop measure for
    Progressive.run(until=...)."""
    return float((a - b).abs().mean())


def write_ppm(filename, g, values):
    import numpy as np
    v = np.ascontiguousarray(values, dtype=np.float32)
    check(lib.dt_write_ppm(filename.encode(), g.xRes, g.yRes, ctypes.c_void_p(v.ctypes.data)), "dt_write_ppm")


def write_png(filename, g, values):
    import numpy as np
    v = np.ascontiguousarray(values, dtype=np.float32)
    check(lib.dt_write_png(filename.encode(), g.xRes, g.yRes, ctypes.c_void_p(v.ctypes.data)), "dt_write_png")


def denoised_filename(filename):
    """<stem>.denoised.<ext> beside the frame file (as `dtrender --denoise` names it)"""
    import os
    stem, ext = os.path.splitext(filename)
    return stem + ".denoised" + ext


def _render_image_upsampled(filename, frame, built, g, how, denoise, guide_bounces=0):
    """renderImage(..., upsample=how) after the scene is built: g is the full resolution"""
    import torch
    params = how if isinstance(how, UpsampleParams) else upsample_params_default()
    if not isinstance(how, UpsampleParams):
        params.factor = int(how)
    g_lo = low_res_globals(g, params.factor)
    names = ("albedo", "normal", "depth")
    scene = Scene(built, g_lo)
    lo = torch.zeros(3 * g_lo.xRes * g_lo.yRes, dtype=torch.float32, device="cuda")
    st = render(scene, g_lo, frame, lo)
    feats_lo = render_features(scene, g_lo, frame, planes=names, specular_bounces=guide_bounces)
    if denoise:
        lo = _denoise(g_lo, lo, feats_lo, None if denoise is True else denoise)
    scene.close()
    scene = Scene(built, g)
    feats_hi = render_features(scene, g, frame, planes=names, specular_bounces=guide_bounces)
    scene.close()
    img = _upsample(g, lo, feats_lo, feats_hi, params).cpu().numpy()
    if filename:
        (write_png if filename.endswith(".png") else write_ppm)(filename, g, img)
    return img, st


def renderImage(filename, frame, sceneBuilder, g=None, builder_frame=None, progressive=None, adaptive=None,
                features=None, denoise=None, upsample=None, guide_bounces=0, occlusion=None, ao_rays=4,
                ao_radius=None, occlusion_lights=()):
    """render_final_project.cpp:965: build (sceneBuilder names a scene.h builder), render the
    frame on the current GPU, write the PPM. Returns (image, stats). progressive=callback renders in
    one-chunk sample windows (Progressive) and calls callback(image, samples_done) with the resolved
    preview (numpy) after every window; the image returned is the same bits, stats the last window's.
    adaptive=tol renders with adaptive sampling (AdaptiveProgressive at that tolerance, in grey levels):
    converged pixels stop between windows, every pixel is the mean of its own samples; a progressive
    callback is called after every window as well. features=prefix also writes the first-hit feature images
    of all spp samples, prefix.albedo.png, prefix.normal.png, prefix.depth.png and prefix.coverage.png
    (feature_images), as `dtrender --features` does. denoise=True or a DenoiseParams also writes the
    denoised frame (denoise() of the image and the feature planes of the samples taken) to
    denoised_filename(filename), as `dtrender --denoise` does; the frame file's bytes are unchanged.
    denoise="variance" or a DenoiseVarParams filters with the per-pixel colour width of dt_denoise_var on the
    adaptive sampler's variance, as `dtrender --denoise-variance` does; it needs adaptive (DTError without). A
    scene with a RectPrismWithCylinder has no feature planes: DTError (DT_E_UNSUPPORTED).
    upsample=s (2, 3 or 4) or an UpsampleParams renders a mixed-resolution preview instead, as
    `dtrender --upsample s` computes it: the frame at low_res_globals(g, s), the albedo, normal and depth
    planes at both resolutions (the full-resolution ones from a second Scene), then upsample(); the
    full-resolution result is written under filename and returned, with the stats of the low-resolution
    render. With denoise=True or a DenoiseParams the low-resolution frame is denoised first. Not with
    progressive, adaptive, features or denoising by variance (DTError). Without upsample nothing changes.
    guide_bounces=K (1..8) takes the specular-path feature buffers (render_features(specular_bounces=K)) for
    the feature images, both denoisers and the upsampler, as `dtrender --guide-bounces K` does: the guides
    then describe what mirrors and glass show. With 0 nothing changes.
    occlusion=prefix also writes the occlusion feature images of all spp samples (render_occlusion with ao_rays,
    ao_radius and occlusion_lights; occlusion_images), prefix.ao.png and prefix.light<j>.png, as
    `dtrender --occlusion` does; not with upsample (DTError). The frame file's bytes are unchanged."""
    import numpy as np
    by_variance = isinstance(denoise, DenoiseVarParams) or (isinstance(denoise, str) and denoise == "variance")
    if by_variance and adaptive is None:
        raise DTError("renderImage: denoise by variance needs adaptive=tol (the sums of squares are adaptive sampling's)")
    g = g if g is not None else globals_default()
    if upsample and (progressive is not None or adaptive is not None or features or by_variance or occlusion):
        raise DTError("renderImage: upsample renders one low-resolution frame: not with progressive, adaptive, "
                      "features, occlusion or denoising by variance")
    built = build_scene(sceneBuilder, frame if builder_frame is None else builder_frame, g)
    if upsample:
        return _render_image_upsampled(filename, frame, built, g, upsample, denoise, guide_bounces)
    scene = Scene(built, g)
    img = np.zeros(3 * g.xRes * g.yRes, dtype=np.float32)
    if adaptive is not None:
        p = AdaptiveProgressive(scene, g, frame, tol=adaptive)
        while not p.done:
            st = p.step()
            if progressive is not None:
                progressive(p.image().cpu().numpy(), p.samples_done)
        img = p.image().cpu().numpy()
    elif progressive is not None:
        p = Progressive(scene, g, frame)
        while not p.done:
            st = p.step()
            img = p.image().cpu().numpy()
            progressive(img, p.samples_done)
    else:
        st = render(scene, g, frame, img)
    if filename:
        (write_png if filename.endswith(".png") else write_ppm)(filename, g, img)
    if features:
        planes = render_features(scene, g, frame, planes=("albedo", "normal", "depth", "coverage"),
                                 specular_bounces=guide_bounces)
        for name, v in feature_images(g, {k: t.cpu().numpy() for k, t in planes.items()}).items():
            write_png("%s.%s.png" % (features, name), g, v)
    if occlusion:
        planes, _ = render_occlusion(scene, g, frame, ao_rays=ao_rays, ao_radius=ao_radius, lights=occlusion_lights)
        for name, v in occlusion_images(g, {k: t.cpu().numpy() for k, t in planes.items()}).items():
            write_png("%s.%s.png" % (occlusion, name), g, v)
    if denoise and filename:
        import torch
        n = p.samples_done if adaptive is not None else None
        planes = render_features(scene, g, frame, n, planes=("albedo", "normal", "depth"),
                                 specular_bounces=guide_bounces)
        if by_variance:
            clean = _denoise(g, torch.from_numpy(img).to("cuda"), planes, None if denoise == "variance" else denoise,
                             variance=p.variance())
        else:
            clean = _denoise(g, torch.from_numpy(img).to("cuda"), planes, None if denoise is True else denoise)
        dn = denoised_filename(filename)
        (write_png if dn.endswith(".png") else write_ppm)(dn, g, clean.cpu().numpy())
    scene.close()
    return img, st


def renderImageCloud(filename, frame, g=None):
    """render_final_project.cpp:1224 (sky/cloud only)."""
    import numpy as np
    g = g if g is not None else globals_default()
    img = np.zeros(3 * g.xRes * g.yRes, dtype=np.float32)
    st = render_sky(g, frame, img)
    if filename:
        write_ppm(filename, g, img)
    return img, st
