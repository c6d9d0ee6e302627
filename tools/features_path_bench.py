"""Specular-path feature buffers (include/dt.h dt_render_features_path, dt_features_path_kernel): cost and
what the guides buy, on final(240) (the C3 camera) with nogloss 0 and 1 and on `spheres` (its own camera).
Prints one JSON line per scene and part.

  (a) kernel ms (HIP events; a warm-up, then K launches: median, min, max) at 1920x1080, 64 spp, of
      dt_render_features and of dt_render_features_path at max_bounces 0, 1, 2 and 8, with the segments traced
      per sample (stats.rays / stats.samples).
  (b) at 320x180: the mean squared error (over the 0..255 floats, all channels) against the converged frame
      (the tool's own 4096-spp render, the same Progressive run continued) of the 64-spp preview as it is,
      denoised with first-hit guides and denoised with path guides (max_bounces 8, default parameters), over
      the pixels whose `bounces` plane is > 0.5 and over the rest.

    python tools/features_path_bench.py [K] [--scene final|final-nogloss|spheres] [--part a|b]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402, F401

import bench  # noqa: E402
import distraytracer_amd as dt  # noqa: E402

SCENES = ("final", "final-nogloss", "spheres")


def build(name):
    if name == "spheres":
        g = dt.globals_default()
        built = dt.build_scene("spheres", 0, g)
        return g, built, 0
    g, built = bench.build_globals(dt, "c3")
    g.nogloss = 1 if name == "final-nogloss" else 0
    return g, built, 240


def timed(k, call):
    call()   # warm-up
    ms, st = [], None
    for _ in range(k):
        st = call()
        ms.append(st.kernel_ms)
    ms.sort()
    return {"kernel_ms_median": round(ms[len(ms) // 2], 4), "kernel_ms_min": round(ms[0], 4),
            "kernel_ms_max": round(ms[-1], 4), "segments_per_sample": round(st.rays / st.samples, 4)}


def part_a(name, k):
    g, built, frame = build(name)
    g.xRes, g.yRes, g.antialias_samples = 1920, 1080, 64
    scene = dt.Scene(built, g)
    out = dt.render_features(scene, g, frame)   # uploads, primary lists; the planes are reused
    out_p = dict(out, bounces=torch.zeros_like(out["depth"]))

    def first():
        st = dt.Stats()
        dt.render_features(scene, g, frame, out=out, stats=st)
        return st

    def path(kb):
        def call():
            st = dt.Stats()
            if kb:
                dt.render_features(scene, g, frame, out=out_p, stats=st, specular_bounces=kb)
            else:   # max_bounces = 0 through the new kernel
                import ctypes
                from distraytracer_amd._lib import Features
                f = Features(*[out[n].data_ptr() for n in ("albedo", "normal", "depth", "coverage", "shape")])
                dt.check(dt.lib.dt_render_features_path(scene.handle, ctypes.byref(g), frame, None, 64, 0, ctypes.byref(f),
                                                        ctypes.c_void_p(out_p["bounces"].data_ptr()), 1, None,
                                                        ctypes.byref(st)), "dt_render_features_path")
            return st
        return call

    res = {"bench": "features_path_cost_1080p_64spp", "scene": name, "reps": k, "dt_render_features": timed(k, first)}
    for kb in (0, 1, 2, 8):
        res["max_bounces_%d" % kb] = timed(k, path(kb))
    res["bounced_pixels"] = round(float((out_p["bounces"] > 0.5).float().mean()), 4)
    scene.close()
    print(json.dumps(res), flush=True)


def part_b(name):
    g, built, frame = build(name)
    g.xRes, g.yRes, g.antialias_samples = 320, 180, 4096
    scene = dt.Scene(built, g)
    p = dt.Progressive(scene, g, frame)
    p.step()
    raw = p.image().clone()
    names = ("albedo", "normal", "depth")
    first = p.features(planes=names)
    path = p.features(planes=names + ("bounces",), specular_bounces=8)
    bounced = (path.pop("bounces") > 0.5).cpu().numpy()
    img = {"raw": raw, "first_hit_guides": dt.denoise(g, raw, first), "path_guides": dt.denoise(g, raw, path)}
    img = {k: v.cpu().numpy().astype(np.float64).reshape(-1, 3) for k, v in img.items()}
    p.run()
    full = p.image().cpu().numpy().astype(np.float64).reshape(-1, 3)
    scene.close()
    res = {"bench": "features_path_quality_320x180_64_of_4096spp", "scene": name, "max_bounces": 8,
           "bounced_pixels": int(bounced.sum()), "other_pixels": int((~bounced).sum())}
    for k, v in img.items():
        e = (v - full) ** 2
        res["mse_" + k] = {"bounced": round(float(e[bounced].mean()), 3) if bounced.any() else None,
                           "rest": round(float(e[~bounced].mean()), 3) if (~bounced).any() else None}
    print(json.dumps(res), flush=True)


def main():
    args = sys.argv[1:]
    scenes, parts, k = SCENES, ("a", "b"), 7
    while args:
        a = args.pop(0)
        if a == "--scene":
            scenes = (args.pop(0),)
        elif a == "--part":
            parts = (args.pop(0),)
        else:
            k = int(a)
    for name in scenes:
        if "a" in parts:
            part_a(name, k)
        if "b" in parts:
            part_b(name)


if __name__ == "__main__":
    main()
