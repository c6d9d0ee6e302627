"""Mutual visibility of two point sets (include/dt.h dt_points_visibility, dt_points_vis_kernel) beside
dt_rays_occluded on the same pairs, on final(240) (the C3 camera). Prints one JSON line.

Sources: the first hits of a coarse grid of the 1920x1080 camera's sample-0 rays (every stride-th hit in camera
order, 2560 of them: 40 waves). Targets: the 64x64 texel centres of the scene's rectangle light, skip_b the light's
own shape. 2560 x 4096 = 10.49 M pairs, the 10.4 M segments of tools/transmittance_bench.py. In one process, the
calls alternating per repetition, everything on the device:

    bits        dt_points_visibility, the bits plane alone
    all_planes  dt_points_visibility, bits, count_a, count_b and weight_a (falloff on)
    occluded    dt_rays_occluded on the pairs materialised target-major (ray j*n_a + i = pair (i, j), so that a wave
                of 64 rays is a wave of the new kernel: 64 consecutive sources towards one target)

Kernel ms (HIP events; a warm-up, then K launches: min, median, max), ns per pair of the whole GPU's time, the bytes
each call reads and writes, and whether the bits are dt_rays_occluded's answers in every pair.

    python tools/points_visibility_bench.py [K]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SOURCES, TW, TH = 2560, 64, 64
RECT_LIGHT = 3   # include/dt.h DT_LIGHT_RECT


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    import torch

    import bench
    import distraytracer_amd as dt
    if not torch.cuda.is_available():
        sys.exit("points_visibility_bench.py needs a GPU")
    torch.cuda.set_device(0)
    g, built = bench.build_globals(dt, "c3")
    scene = dt.Scene(built, g)
    start, dir = dt.camera_rays(g, 240, samples=(0, 1))
    hits, _ = dt.trace_rays(scene, g, start.reshape(-1, 3), dir.reshape(-1, 3), planes=("shape", "point", "normal"))
    hit = hits["shape"] >= 0
    p, nrm = hits["point"][hit], hits["normal"][hit]
    del start, dir, hits
    stride = len(p) // N_SOURCES
    a, na = p[::stride][:N_SOURCES].contiguous(), nrm[::stride][:N_SOURCES].contiguous()
    light = next(built.desc.lights[i] for i in range(built.desc.n_lights) if built.desc.lights[i].type == RECT_LIGHT)
    tb, tn = dt.shape_texels(built, light.shape_index, TW, TH)
    b, nb = torch.from_numpy(tb).cuda(), torch.from_numpy(tn).cuda()
    n_a, n_b = len(a), len(b)
    skip_b = torch.full((n_b,), int(light.shape_index), dtype=torch.int32, device="cuda")
    # the pairs, target-major
    org = a.repeat(n_b, 1).contiguous()
    seg = (b.repeat_interleave(n_a, dim=0) - org).contiguous()
    skip = torch.full((n_a * n_b,), int(light.shape_index), dtype=torch.int32, device="cuda")
    occ = torch.empty(n_a * n_b, dtype=torch.uint8, device="cuda")
    res = {}

    def t_vis(name, planes):
        res[name], st = dt.points_visibility(scene, g, a, b, skip_b=skip_b, normals_a=na, normals_b=nb, falloff=True,
                                             planes=planes)
        res[name + "_traced"] = int(st.shadow_rays)
        return st.kernel_ms

    def t_occluded():
        st = dt.rays_occluded(scene, g, org, seg, skip_shape=skip, out=occ)[1]
        res["occluded_traced"] = int(st.shadow_rays)
        return st.kernel_ms

    runs = {"bits": lambda: t_vis("bits", ("bits",)),
            "all_planes": lambda: t_vis("all", ("bits", "count_a", "count_b", "weight_a")),
            "occluded": t_occluded}
    for f in runs.values():   # warm-up
        f()
    ms = {name: [] for name in runs}
    for _ in range(k):   # alternating
        for name, f in runs.items():
            ms[name].append(f())
    # the bits against dt_rays_occluded's answers (a void ray is "not occluded" in both)
    words = res["bits"]["bits"]
    j = torch.arange(n_b, device="cuda")
    vis = ((words[:, j >> 5] >> (j & 31)[None, :]) & 1) != 0
    same = bool(torch.equal(vis, occ.view(n_b, n_a).t() == 0))
    same_all = bool(torch.equal(res["all"]["bits"], words) and
                    torch.equal(res["all"]["count_a"].long(), vis.sum(dim=1)) and
                    torch.equal(res["all"]["count_b"].long(), vis.sum(dim=0)))
    pairs = n_a * n_b
    n_words = (n_b + 31) // 32
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {"bench": "points_visibility_c3", "scene": "final(240) c3", "reps": k, "sources": n_a, "targets": n_b,
           "pairs": pairs, "work_items": ((n_a + 63) // 64) * ((n_b + 255) // 256),
           "kernel_ms": {name: {"min": round(min(v), 4), "median": round(med[name], 4), "max": round(max(v), 4)}
                         for name, v in ms.items()},
           "ns_per_pair": {name: round(med[name] * 1e6 / pairs, 4) for name in ms},
           "bytes": {"bits": {"in": 24 * (n_a + n_b) + 4 * n_b, "out": 4 * n_a * n_words},
                     "all_planes": {"in": 48 * (n_a + n_b) + 4 * n_b, "out": 4 * n_a * n_words + 12 * n_a + 4 * n_b},
                     "occluded": {"in": 52 * pairs, "out": pairs}},
           "traced": {"bits": res["bits_traced"], "all_planes": res["all_traced"], "occluded": res["occluded_traced"]},
           "visible_fraction": round(float(vis.float().mean()), 4),
           "bits_over_occluded": round(med["bits"] / med["occluded"], 4),
           "all_planes_over_bits": round(med["all_planes"] / med["bits"], 4),
           "bits_equal_rays_occluded": same, "all_planes_consistent": same_all}
    scene.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
