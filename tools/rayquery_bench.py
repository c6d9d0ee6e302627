"""Ray queries (include/dt.h dt_trace_rays, dt_rays_occluded; dt_rayq_kernel, dt_rayq_occl_kernel): what handing
the tracer explicit rays costs beside the camera's own, and what their order in memory is worth. Single
process, the C3 scene (final(240), 1920x1080), the 2^24 primary rays of the intersection micro-benchmark.
One JSON line: HIP-event kernel ms (min, median, max over the repetitions) of

    isect            dt_intersect_primary: the rays built in the kernel, primary lists
    explicit         the same rays from memory (or_primary_ray's), dt_trace_rays with shape and t only
    permuted         the same rays in one fixed random permutation: every wave's 64 rays scattered over the frame
    all_planes       the rays in order, every plane (point, normal, albedo as well)
    occluded         dt_rays_occluded from the hit points to the first light's centre

after one warm-up of each, the repetitions alternating between the five (tools/temporal_bench.py --cost), and
whether the explicit and the permuted answers are dt_intersect_primary's in every bit.

    python tools/rayquery_bench.py [--rays 16777216] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    n = args.rays

    import numpy as np
    import torch

    import bench
    import distraytracer_amd as dt
    from oracle import geom as G   # the ray generator only (or_primary_ray)
    if not torch.cuda.is_available():
        sys.exit("rayquery_bench.py needs a GPU")
    torch.cuda.set_device(0)
    g, built = bench.build_globals(dt, "c3")
    scene = dt.Scene(built, g)
    start_h, dir_h = G.or_primary_ray(g, 240, 0, n)
    start, dir = torch.from_numpy(start_h).cuda(), torch.from_numpy(dir_h).cuda()
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()
    start_p, dir_p = start[perm].contiguous(), dir[perm].contiguous()
    del start_h, dir_h

    ishape = torch.empty(n, dtype=torch.int32, device="cuda")
    it = torch.empty(n, dtype=torch.float32, device="cuda")
    two = {"shape": torch.empty_like(ishape), "t": torch.empty_like(it)}
    two_p = {"shape": torch.empty_like(ishape), "t": torch.empty_like(it)}
    full = {"shape": torch.empty_like(ishape), "t": torch.empty_like(it),
            **{k: torch.empty(n, 3, dtype=torch.float64, device="cuda") for k in ("point", "normal", "albedo")}}
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")

    def t_isect():
        return dt.intersect_primary(scene, g, 240, 0, ishape, it)

    def t_explicit():
        return dt.trace_rays(scene, g, start, dir, out=two)[1].kernel_ms

    def t_permuted():
        return dt.trace_rays(scene, g, start_p, dir_p, out=two_p)[1].kernel_ms

    def t_full():
        return dt.trace_rays(scene, g, start, dir, out=full)[1].kernel_ms

    t_full()   # the hit points of the visibility segments
    light = built.desc.lights[0]
    centre = torch.tensor(list(light.center), dtype=torch.float64, device="cuda")
    seg = (centre[None, :] - full["point"]).contiguous()
    skip = torch.full((n,), int(light.shape_index), dtype=torch.int32, device="cuda")

    def t_occluded():
        return dt.rays_occluded(scene, g, full["point"], seg, skip_shape=skip, out=occ)[1].kernel_ms

    runs = {"isect": t_isect, "explicit": t_explicit, "permuted": t_permuted, "all_planes": t_full,
            "occluded": t_occluded}
    for f in runs.values():   # warm-up
        f()
    ms = {k: [] for k in runs}
    for _ in range(args.reps):   # alternating
        for k, f in runs.items():
            ms[k].append(f())
    same = bool(torch.equal(two["shape"], ishape) and torch.equal(two["t"].view(torch.int32), it.view(torch.int32)))
    same_p = bool(torch.equal(two_p["shape"], ishape[perm]) and
                  torch.equal(two_p["t"].view(torch.int32), it[perm].view(torch.int32)))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"bench": "rayquery_c3", "rays": n, "reps": args.reps,
           "kernel_ms": {k: {"min": round(min(v), 4), "median": round(med[k], 4), "max": round(max(v), 4)}
                         for k, v in ms.items()},
           "mrays_per_s": {k: round(n / (med[k] / 1e3) / 1e6, 1) for k in ms},
           "explicit_over_isect": round(med["explicit"] / med["isect"], 4),
           "permuted_over_explicit": round(med["permuted"] / med["explicit"], 4),
           "all_planes_over_explicit": round(med["all_planes"] / med["explicit"], 4),
           "hit_fraction": round(float((ishape >= 0).float().mean()), 4),
           "occluded_fraction": round(float(occ.float().mean()), 4),
           "explicit_equals_isect": same, "permuted_equals_isect": same_p}
    scene.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
