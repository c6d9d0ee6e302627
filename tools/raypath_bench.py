"""Path ray queries (include/dt.h dt_trace_rays_path; dt_rayq_path_kernel): what following caller-supplied rays
through mirrors and glass costs beside their first hit, and beside the feature kernel that runs the same chain on
its own camera samples. Single process, the C3 scene (final(240), 1920x1080) with nogloss = 1 (its doors, floor
and checker cylinder are then mirrors), the camera rays of the samples 0 .. S-1 of every pixel (dt_camera_rays).
One JSON line: HIP-event kernel ms (min, median, max over the repetitions) of

    trace_rays       dt_trace_rays on those rays, shape and point
    path_K           dt_trace_rays_path at max_bounces = K (0, 1, 2, 8), end, segments, shape and point
    path_K_all       ... with every plane (K = 2 only)
    features_path_K  dt_render_features_path at max_bounces = K over all spp samples of every pixel (its window rule
                     takes no fewer), every plane

after one warm-up of each, the repetitions alternating between them; per K the ratio to trace_rays (for K = 0 the
whole overhead of the new call), the segments traced, and the time per traced segment of the query and of the
feature kernel (the same chain, but the feature kernel makes its rays itself, takes segment 0 through the
primary-ray lists and writes per pixel).

    python tools/raypath_bench.py [--samples 4] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (0, 1, 2, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    ns = args.samples

    import torch

    import bench
    import distraytracer_amd as dt
    if not torch.cuda.is_available():
        sys.exit("raypath_bench.py needs a GPU")
    torch.cuda.set_device(0)
    g, built = bench.build_globals(dt, "c3")
    g.nogloss = 1
    scene = dt.Scene(built, g)
    start, dir = dt.camera_rays(g, 240, samples=(0, ns))
    start, dir = start.view(-1, 3), dir.view(-1, 3)
    n = start.shape[0]
    segments = {}

    def t_trace():
        return dt.trace_rays(scene, g, start, dir, planes=("shape", "point"))[1].kernel_ms

    def t_path(K, planes=("end", "segments", "shape", "point")):
        def run():
            st = dt.trace_rays_path(scene, g, start, dir, max_bounces=K, planes=planes)[1]
            segments["path_%d" % K] = int(st.rays)
            return st.kernel_ms
        return run

    def t_feat(K):
        def run():
            st = dt.Stats()
            dt.render_features(scene, g, 240, planes=dt.FEATURE_PLANES + ("bounces",), stats=st, specular_bounces=K)
            segments["features_path_%d" % K] = int(st.rays)
            return st.kernel_ms
        return run

    runs = {"trace_rays": t_trace}
    for K in KS:
        runs["path_%d" % K] = t_path(K)
    runs["path_2_all"] = t_path(2, dt.RAY_PATH_PLANES)
    for K in KS[1:]:
        runs["features_path_%d" % K] = t_feat(K)
    for f in runs.values():   # warm-up
        f()
    ms = {k: [] for k in runs}
    for _ in range(args.reps):   # alternating
        for k, f in runs.items():
            ms[k].append(f())
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"bench": "raypath_c3_nogloss", "rays": n, "samples": ns, "reps": args.reps,
           "kernel_ms": {k: {"min": round(min(v), 4), "median": round(med[k], 4), "max": round(max(v), 4)}
                         for k, v in ms.items()},
           "segments": segments,
           "path_over_trace_rays": {str(K): round(med["path_%d" % K] / med["trace_rays"], 4) for K in KS},
           "all_planes_over_path_2": round(med["path_2_all"] / med["path_2"], 4),
           "ns_per_segment": {k: round(med[k] * 1e6 / segments[k], 3) for k in segments},
           "trace_rays_ns_per_ray": round(med["trace_rays"] * 1e6 / n, 3)}
    scene.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
