"""Irradiance queries at surface points (include/dt.h dt_points_irradiance, dt_points_irr_kernel): what the cosine
weighting costs over dt_points_occlusion's probes, and what a gather probe costs, on final(240) (the C3 camera).
Prints one JSON line.

The points are tools/points_occlusion_bench.py's: the first hits of the 1920x1080 camera's sample-0 rays, in
camera order, as device arrays. 1 sample per point, every light of the scene (at most 8). In one process, the
calls alternating per repetition:

    occlusion_lights   dt_points_occlusion, the light plane alone (the same shadow walks, counted as integers)
    direct             dt_points_irradiance, direct and direct_rgb (those walks, a normalise and a dot per probe)
    gather_1, gather_4 dt_points_irradiance, indirect_rgb and sky alone with 1 and 4 gather probes per sample: per
                       probe one closest-hit walk and, from a hit that is no emitter, one shadow walk per light

Kernel ms (HIP events; a warm-up, then K launches: median, min, max), the walks (stats.shadow_rays + stats.rays)
and kernel ms / walks in nanoseconds of the whole GPU's time.

    python tools/points_irradiance_bench.py [K]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import distraytracer_amd as dt  # noqa: E402
from points_occlusion_bench import H, W, camera_points  # noqa: E402


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    g, built = bench.build_globals(dt, "c3")
    g.xRes, g.yRes, g.antialias_samples = W, H, 64
    scene = dt.Scene(built, g)
    pts, nrm = camera_points(scene, g)
    lights = tuple(range(min(built.desc.n_lights, 8)))
    calls = {
        "occlusion_lights": lambda: dt.points_occlusion(scene, g, pts, nrm, frame=240, n_samples=1, ao_rays=0, lights=lights),
        "direct": lambda: dt.points_irradiance(scene, g, pts, nrm, frame=240, n_samples=1, lights=lights,
                                               planes=("direct", "direct_rgb")),
        "gather_1": lambda: dt.points_irradiance(scene, g, pts, nrm, frame=240, n_samples=1, lights=lights,
                                                 gather_rays=1, planes=("indirect_rgb", "sky")),
        "gather_4": lambda: dt.points_irradiance(scene, g, pts, nrm, frame=240, n_samples=1, lights=lights,
                                                 gather_rays=4, planes=("indirect_rgb", "sky")),
    }
    ms = {name: [] for name in calls}
    st, mean = {}, {}
    for rep in range(k + 1):   # rep 0: the warm-up; the calls alternate
        for name, call in calls.items():
            out, s = call()
            if rep:
                ms[name].append(s.kernel_ms)
            st[name] = s
            mean[name] = {p: round(float(a.mean()), 4) for p, a in out.items()}
    scene.close()
    res = {"bench": "points_irradiance_1080p_first_hits", "scene": "final(240) c3", "reps": k, "points": int(pts.shape[0]),
           "n_samples": 1, "n_lights": len(lights)}
    for name, v in ms.items():
        v.sort()
        walks = int(st[name].shadow_rays + st[name].rays)
        res[name] = {"kernel_ms_median": round(v[len(v) // 2], 4), "kernel_ms_min": round(v[0], 4),
                     "kernel_ms_max": round(v[-1], 4), "shadow_probes": int(st[name].shadow_rays),
                     "gather_probes": int(st[name].rays), "ns_per_walk": round(v[len(v) // 2] * 1e6 / max(walks, 1), 4),
                     "mean": mean[name]}
    res["direct_over_occlusion"] = round(res["direct"]["kernel_ms_median"] / res["occlusion_lights"]["kernel_ms_median"], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
