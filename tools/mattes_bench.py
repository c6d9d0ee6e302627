"""Object mattes (include/dt.h dt_render_mattes, dt_mattes_kernel): the call at 1920x1080, 64 samples, 4 layers,
material groups (shape_groups), on final(240) (the C3 camera), id, weight and distinct on the device. Beside it,
in the same run and alternating with it launch by launch, dt_render_features with all five planes: the same
primary rays, f64 column sums in the place of the ballots. Prints one JSON line: kernel ms (HIP events) of K
launches of each after a warm-up of both, their median, min and max, the ratio of the medians, and the
frame's overflow_pixels and distinct-group statistics.

    python tools/mattes_bench.py [K]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401

import bench  # noqa: E402
import distraytracer_amd as dt  # noqa: E402


def _summary(ms):
    ms = sorted(ms)
    return {"kernel_ms_median": round(ms[len(ms) // 2], 4), "kernel_ms_min": round(ms[0], 4),
            "kernel_ms_max": round(ms[-1], 4)}


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    g, built = bench.build_globals(dt, "c3")
    g.xRes, g.yRes, g.antialias_samples = 1920, 1080, 64
    n_rays = g.xRes * g.yRes * 64
    groups = dt.shape_groups(built)
    scene = dt.Scene(built, g)
    # warm-up of both (uploads, primary lists, code objects); the planes are reused
    feats = dt.render_features(scene, g, 240)
    m = dt.render_mattes(scene, g, 240, groups=groups, layers=4, planes=dt.MATTE_PLANES)
    planes = {name: m[name] for name in dt.MATTE_PLANES}
    for _ in range(2):
        dt.render_features(scene, g, 240, out=feats)
        dt.render_mattes(scene, g, 240, groups=groups, layers=4, out=planes)
    fms, mms = [], []
    for _ in range(k):
        st = dt.Stats()
        dt.render_features(scene, g, 240, out=feats, stats=st)
        fms.append(st.kernel_ms)
        st = dt.Stats()
        m = dt.render_mattes(scene, g, 240, groups=groups, layers=4, out=planes, stats=st)
        mms.append(st.kernel_ms)
    f, mm = _summary(fms), _summary(mms)
    distinct = planes["distinct"]
    res = {"bench": "mattes_c3_1080p_64spp_4layers", "rays": n_rays, "reps": k, "groups": int(groups.max()) + 1,
           "shapes": int(groups.size),
           "mattes": dict(mm, kernel="dt_mattes_kernel", mrays_per_s=round(n_rays / (mm["kernel_ms_median"] / 1e3) / 1e6, 1)),
           "features": dict(f, kernel="dt_features_kernel",
                            mrays_per_s=round(n_rays / (f["kernel_ms_median"] / 1e3) / 1e6, 1)),
           "mattes_over_features": round(mm["kernel_ms_median"] / f["kernel_ms_median"], 3),
           "overflow_pixels": int(m["overflow_pixels"]), "distinct_max": int(distinct.max()),
           "pixels_with_2_or_more_groups": int((distinct >= 2).sum())}
    scene.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
