"""Occlusion feature buffers (include/dt.h dt_render_occlusion, dt_occlusion_kernel): what the planes cost, on
final(240) (the C3 camera) at 1920x1080, 64 spp. Prints one JSON line.

Kernel ms (HIP events; a warm-up, then K launches: median, min, max) of dt_render_features on the same commit
(the primary hit alone, the floor under every figure here), of dt_render_occlusion at ao_rays 1, 4 and 8 with no
lights, and with every light of the scene (at most 8) and ao_rays 0; with each the probes tested
(stats.shadow_rays) and the cost per probe derived from them: (kernel ms - dt_render_features' ms) / probes, in
nanoseconds (of the whole GPU's time, not of one lane's).

    python tools/occlusion_bench.py [K] [--ao-radius R]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402, F401

import bench  # noqa: E402
import distraytracer_amd as dt  # noqa: E402


def timed(k, call):
    call()   # warm-up
    ms, st = [], None
    for _ in range(k):
        st = call()
        ms.append(st.kernel_ms)
    ms.sort()
    return {"kernel_ms_median": round(ms[len(ms) // 2], 4), "kernel_ms_min": round(ms[0], 4),
            "kernel_ms_max": round(ms[-1], 4)}, st


def main():
    args = sys.argv[1:]
    k, radius = 7, None
    while args:
        a = args.pop(0)
        if a == "--ao-radius":
            radius = float(args.pop(0))
        else:
            k = int(a)
    g, built = bench.build_globals(dt, "c3")
    g.xRes, g.yRes, g.antialias_samples = 1920, 1080, 64
    scene = dt.Scene(built, g)
    feats = dt.render_features(scene, g, 240)   # uploads, primary lists; the planes are reused
    radius = dt.occlusion_params_default().ao_radius if radius is None else radius
    lights = tuple(range(min(built.desc.n_lights, 8)))

    def first():
        st = dt.Stats()
        dt.render_features(scene, g, 240, out=feats, stats=st)
        return st

    def occl(ao_rays, ls):
        out, _ = dt.render_occlusion(scene, g, 240, ao_rays=ao_rays, ao_radius=radius, lights=ls)

        def call():
            return dt.render_occlusion(scene, g, 240, ao_rays=ao_rays, ao_radius=radius, lights=ls, out=out)[1]
        return call, out

    res = {"bench": "occlusion_cost_1080p_64spp", "scene": "final(240) c3", "reps": k, "ao_radius": round(radius, 4),
           "n_lights": len(lights)}
    res["dt_render_features"], _ = timed(k, first)
    base = res["dt_render_features"]["kernel_ms_median"]
    for name, ao_rays, ls in (("ao_rays_1", 1, ()), ("ao_rays_4", 4, ()), ("ao_rays_8", 8, ()),
                              ("all_lights_ao_rays_0", 0, lights)):
        call, out = occl(ao_rays, ls)
        r, st = timed(k, call)
        r["probes"] = int(st.shadow_rays)
        r["ns_per_probe"] = round((r["kernel_ms_median"] - base) * 1e6 / max(st.shadow_rays, 1), 4)
        r["mean"] = round(float(out["ao" if ao_rays else "light"].mean()), 4)
        res[name] = r
    scene.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
