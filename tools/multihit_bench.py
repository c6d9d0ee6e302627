"""Multi-hit ray queries (include/dt.h dt_trace_rays_multi; dt_rayq_multi_kernel): what the k nearest surfaces
cost beside the closest one. Single process, the C3 scene (final(240), 1920x1080), the 2^24 primary rays of
tools/rayquery_bench.py in camera order and in its fixed random permutation. One JSON line: HIP-event kernel
ms (min, median, max over the repetitions) of

    closest          dt_trace_rays with shape and t
    k1, k2, k4, k8   dt_trace_rays_multi with count, shape and t (the list capacities 1, 2, 4, 8)

each in camera order and permuted (suffix _p), after one warm-up of each, the repetitions alternating between
the ten; the spread of a figure is its (max - min) / median. Also the mean number of hits recorded per ray, and
whether k1's shape and t are dt_trace_rays's in every bit (they need not be: include/dt.h, the tie and
edge-on rules; the number of rays that differ is reported).

    python tools/multihit_bench.py [--rays 16777216] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n = args.rays
    if args.reps < 3:
        sys.exit("multihit_bench.py: at least 3 timed runs")

    import numpy as np
    import torch

    import bench
    import distraytracer_amd as dt
    from oracle import geom as G   # the ray generator only (or_primary_ray)
    if not torch.cuda.is_available():
        sys.exit("multihit_bench.py needs a GPU")
    torch.cuda.set_device(0)
    g, built = bench.build_globals(dt, "c3")
    scene = dt.Scene(built, g)
    start_h, dir_h = G.or_primary_ray(g, 240, 0, n)
    start, dir = torch.from_numpy(start_h).cuda(), torch.from_numpy(dir_h).cuda()
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()
    rays = {"": (start, dir), "_p": (start[perm].contiguous(), dir[perm].contiguous())}
    del start_h, dir_h

    one = {sfx: {"shape": torch.empty(n, dtype=torch.int32, device="cuda"),
                 "t": torch.empty(n, dtype=torch.float32, device="cuda")} for sfx in rays}
    last = {}

    def closest(sfx):
        return lambda: dt.trace_rays(scene, g, *rays[sfx], out=one[sfx])[1].kernel_ms

    def multi(k, sfx):
        def run():
            last[(k, sfx)], st = dt.trace_rays_multi(scene, g, *rays[sfx], k=k, planes=("count", "shape", "t"))
            return st.kernel_ms
        return run

    runs = {}
    for sfx in rays:
        runs["closest" + sfx] = closest(sfx)
        for k in KS:
            runs["k%d%s" % (k, sfx)] = multi(k, sfx)
    for f in runs.values():   # warm-up
        f()
    ms = {name: [] for name in runs}
    for _ in range(args.reps):   # alternating
        for name, f in runs.items():
            ms[name].append(f())
    med = {name: statistics.median(v) for name, v in ms.items()}
    differ = {}
    for sfx in rays:
        m = last[(1, sfx)]
        differ["k1%s_vs_closest" % sfx] = int(((m["shape"][:, 0] != one[sfx]["shape"]) |
                                               (m["t"][:, 0].view(torch.int32) != one[sfx]["t"].view(torch.int32))).sum())
    same_order = bool(torch.equal(last[(8, "_p")]["shape"], last[(8, "")]["shape"][perm]) and
                      torch.equal(last[(8, "_p")]["t"].view(torch.int32), last[(8, "")]["t"][perm].view(torch.int32)))
    out = {"bench": "multihit_c3", "rays": n, "reps": args.reps,
           "kernel_ms": {name: {"min": round(min(v), 4), "median": round(med[name], 4), "max": round(max(v), 4),
                                "spread": round((max(v) - min(v)) / med[name], 4)} for name, v in ms.items()},
           "mrays_per_s": {name: round(n / (med[name] / 1e3) / 1e6, 1) for name in ms},
           "over_closest": {name: round(med[name] / med["closest" + ("_p" if name.endswith("_p") else "")], 4)
                            for name in ms},
           "mean_hits_recorded": {"k%d" % k: round(float(last[(k, "")]["count"].float().mean()), 4) for k in KS},
           "rays_differing": differ, "k8_permuted_equals_k8": same_order}
    scene.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
