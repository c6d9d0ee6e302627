"""First-hit feature buffers (include/dt.h dt_render_features, dt_features_kernel): the call at
1920x1080, 64 spp, on final(240) (the C3 camera), all five planes on the device. Prints one JSON line:
kernel ms (HIP events) of K launches after a warm-up, their median, min and max, Mrays/s, and beside it
dt_intersect_primary (tools/isect_bench.py's kernel) over the same number of primary rays
(1920*1080*64), the closest hit alone, and the ratio of the two medians.

    python tools/features_bench.py [K]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import distraytracer_amd as dt  # noqa: E402


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    g, built = bench.build_globals(dt, "c3")
    g.xRes, g.yRes, g.antialias_samples = 1920, 1080, 64
    n_rays = g.xRes * g.yRes * 64
    scene = dt.Scene(built, g)
    out = dt.render_features(scene, g, 240)   # warm-up (uploads, primary lists); the planes are reused
    ms = []
    for _ in range(k):
        st = dt.Stats()
        dt.render_features(scene, g, 240, out=out, stats=st)
        ms.append(st.kernel_ms)
    ms.sort()
    med = ms[len(ms) // 2]
    res = {"bench": "features_c3_1080p_64spp", "rays": n_rays, "kernel": "dt_features_kernel", "reps": k,
           "kernel_ms_median": round(med, 4), "kernel_ms_min": round(ms[0], 4), "kernel_ms_max": round(ms[-1], 4),
           "mrays_per_s": round(n_rays / (med / 1e3) / 1e6, 1),
           "coverage_mean": round(float(out["coverage"].mean()), 4), "tex_fetches": int(st.tex_fetches)}
    del out
    shape = torch.empty(n_rays, dtype=torch.int32, device="cuda")
    t = torch.empty(n_rays, dtype=torch.float32, device="cuda")
    dt.intersect_primary(scene, g, 240, 0, shape, t)
    ims = sorted(dt.intersect_primary(scene, g, 240, 0, shape, t) for _ in range(k))
    imed = ims[len(ims) // 2]
    res["isect_same_rays"] = {"kernel": "dt_isect_kernel", "kernel_ms_median": round(imed, 4),
                              "kernel_ms_min": round(ims[0], 4), "kernel_ms_max": round(ims[-1], 4),
                              "mrays_per_s": round(n_rays / (imed / 1e3) / 1e6, 1)}
    res["features_over_isect"] = round(med / imed, 3)
    scene.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
