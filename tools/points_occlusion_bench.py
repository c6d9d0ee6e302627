"""Occlusion queries at surface points (include/dt.h dt_points_occlusion, dt_points_occl_kernel): what a probe
costs, and what the order of the points is worth, on final(240) (the C3 camera). Prints one JSON line.

The points are the first hits of the 1920x1080 camera's sample-0 rays (the oracle's or_primary_ray, traced by
dt_trace_rays on device arrays; the misses are left out), in camera order: pixel y*xRes + x, the same surface
points dt_render_occlusion probes from, so tools/occlusion_bench.py run in the same session gives the per-probe
cost of the same probes reached from the camera. The same points are also run in one fixed random permutation
(seed 1): 64 consecutive points share a wave, which walks the union of its probes' nodes.

Each order runs 1 sample x 4 AO probes (no lights) and 1 sample x every light of the scene (at most 8, no AO).
Kernel ms (HIP events; a warm-up, then K launches: median, min, max), the probes tested (stats.shadow_rays) and
kernel ms / probes in nanoseconds (of the whole GPU's time, not of one lane's). The orders alternate inside
one process.

    python tools/points_occlusion_bench.py [K]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import distraytracer_amd as dt  # noqa: E402
from oracle import geom as G  # noqa: E402

W, H = 1920, 1080
CHUNK = 1 << 17   # pixels per or_primary_ray call (8 rays each, of which sample 0 is kept)


def camera_points(scene, g):
    """(points, normals) on the device, float64 (n, 3): the hits of sample 0 of every pixel, in pixel order"""
    pts, nrm = [], []
    for p0 in range(0, W * H, CHUNK):
        n = min(CHUNK, W * H - p0)
        start, ray = G.or_primary_ray(g, 240, p0 * 8, n * 8)   # ray (pixel * 8 + sample) for samples 0..7
        s = torch.from_numpy(np.ascontiguousarray(start[::8])).cuda()
        d = torch.from_numpy(np.ascontiguousarray(ray[::8])).cuda()
        hits, _ = dt.trace_rays(scene, g, s, d, planes=("shape", "point", "normal"))
        keep = hits["shape"] >= 0
        pts.append(hits["point"][keep])
        nrm.append(hits["normal"][keep])
    return torch.cat(pts).contiguous(), torch.cat(nrm).contiguous()


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    g, built = bench.build_globals(dt, "c3")
    g.xRes, g.yRes, g.antialias_samples = W, H, 64
    scene = dt.Scene(built, g)
    pts, nrm = camera_points(scene, g)
    n = pts.shape[0]
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()
    orders = {"camera_order": (pts, nrm), "random_order": (pts[perm].contiguous(), nrm[perm].contiguous())}
    lights = tuple(range(min(built.desc.n_lights, 8)))
    radius = dt.occlusion_params_default().ao_radius
    res = {"bench": "points_occlusion_1080p_first_hits", "scene": "final(240) c3", "reps": k, "points": int(n),
           "of_pixels": W * H, "n_samples": 1, "ao_radius": round(radius, 4), "n_lights": len(lights)}
    for name, kw in (("ao_rays_4", dict(ao_rays=4, ao_radius=radius)), ("all_lights_ao_rays_0", dict(ao_rays=0, lights=lights))):
        ms = {o: [] for o in orders}
        st, mean = {}, {}
        for rep in range(k + 1):   # rep 0: the warm-up; the orders alternate
            for o, (p, nn) in orders.items():
                out, s = dt.points_occlusion(scene, g, p, nn, frame=240, n_samples=1, **kw)
                if rep:
                    ms[o].append(s.kernel_ms)
                st[o], mean[o] = s, float(out["ao" if "ao" in out else "light"].mean())
        res[name] = {}
        for o, v in ms.items():
            v.sort()
            res[name][o] = {"kernel_ms_median": round(v[len(v) // 2], 4), "kernel_ms_min": round(v[0], 4),
                            "kernel_ms_max": round(v[-1], 4), "probes": int(st[o].shadow_rays),
                            "ns_per_probe": round(v[len(v) // 2] * 1e6 / max(st[o].shadow_rays, 1), 4),
                            "mean": round(mean[o], 4)}
    scene.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
