"""Transmittance queries (include/dt.h dt_rays_transmittance, dt_points_occlusion_glass; dt_rayq_transmit_kernel,
dt_points_occl_glass_kernel): what the glass filter costs beside the any-hit queries it is built on. Single
process, the C3 scene (final(240), 1920x1080; it holds no glass, so this is the cost of the walk and the
bookkeeping alone). The rays: the first hits of the C3 camera (sample 0 of every pixel) towards the centres of the
scene's five lights, the light's own shape skipped, in camera order (light-major) and in one fixed random
permutation. One JSON line: HIP-event kernel ms (min, median, max over the repetitions) of

    occluded             dt_rays_occluded
    transmit_k0          dt_rays_transmittance, k = 0, panes only (no list)
    transmit_k8          dt_rays_transmittance, k = 8, panes and pane_shape
    *_permuted           the same three on the permuted rays
    points               dt_points_occlusion at the first hits of every 16th pixel, 4 samples, 4 AO probes, 5 lights
    points_glass         dt_points_occlusion_glass(max_panes = 8) on the same points, pane planes included

after one warm-up of each, the repetitions alternating between them, the ratios of the medians, and whether
(panes != 0) is dt_rays_occluded's answer in every ray and the max_panes = 0 planes dt_points_occlusion's in every bit.

    python tools/transmittance_bench.py [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    import distraytracer_amd as dt
    if not torch.cuda.is_available():
        sys.exit("transmittance_bench.py needs a GPU")
    torch.cuda.set_device(0)
    g, built = bench.build_globals(dt, "c3")
    scene = dt.Scene(built, g)
    start, dir = dt.camera_rays(g, 240, samples=(0, 1))
    start, dir = start.reshape(-1, 3), dir.reshape(-1, 3)
    hits, _ = dt.trace_rays(scene, g, start, dir, planes=("shape", "point", "normal"))
    hit = hits["shape"] >= 0
    p, nrm = hits["point"][hit].contiguous(), hits["normal"][hit].contiguous()
    del start, dir
    lights = [built.desc.lights[i] for i in range(built.desc.n_lights)]
    org = p.repeat(len(lights), 1).contiguous()
    seg = torch.cat([torch.tensor(list(L.center), dtype=torch.float64, device="cuda")[None, :] - p for L in lights]).contiguous()
    skip = torch.cat([torch.full((len(p),), int(L.shape_index), dtype=torch.int32, device="cuda") for L in lights]).contiguous()
    n = len(org)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()
    org_p, seg_p, skip_p = org[perm].contiguous(), seg[perm].contiguous(), skip[perm].contiguous()
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    occ_p = torch.empty_like(occ)
    res = {}

    def t_occluded(o=org, s=seg, k=skip, out=occ):
        return dt.rays_occluded(scene, g, o, s, skip_shape=k, out=out)[1].kernel_ms

    def t_transmit(kk, name, o=org, s=seg, k=skip):
        res[name], st = dt.rays_transmittance(scene, g, o, s, skip_shape=k, k=kk,
                                              planes=("panes", "pane_shape") if kk else ("panes",))
        return st.kernel_ms

    pp, pn = p[::16].contiguous(), nrm[::16].contiguous()
    pkw = dict(frame=240, n_samples=4, ao_rays=4, lights=tuple(range(len(lights))))

    def t_points(tg, name):
        res[name], st = dt.points_occlusion(scene, g, pp, pn, through_glass=tg, **pkw)
        return st.kernel_ms

    runs = {"occluded": t_occluded,
            "transmit_k0": lambda: t_transmit(0, "k0"),
            "transmit_k8": lambda: t_transmit(8, "k8"),
            "occluded_permuted": lambda: t_occluded(org_p, seg_p, skip_p, occ_p),
            "transmit_k0_permuted": lambda: t_transmit(0, "k0p", org_p, seg_p, skip_p),
            "transmit_k8_permuted": lambda: t_transmit(8, "k8p", org_p, seg_p, skip_p),
            "points": lambda: t_points(None, "points"),
            "points_glass": lambda: t_points(8, "points_glass")}
    for f in runs.values():   # warm-up
        f()
    ms = {k: [] for k in runs}
    for _ in range(args.reps):   # alternating
        for k, f in runs.items():
            ms[k].append(f())
    same = bool(torch.equal(res["k0"]["panes"] != 0, occ != 0) and torch.equal(res["k8"]["panes"], res["k0"]["panes"]) and
                torch.equal(res["k0p"]["panes"] != 0, occ_p != 0))
    zero, _ = dt.points_occlusion(scene, g, pp, pn, through_glass=0, **pkw)
    same_pts = all(bool(torch.equal(zero[k].view(torch.int32), res["points"][k].view(torch.int32))) for k in ("ao", "light"))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"bench": "transmittance_c3", "rays": n, "points": len(pp), "reps": args.reps,
           "kernel_ms": {k: {"min": round(min(v), 4), "median": round(med[k], 4), "max": round(max(v), 4)}
                         for k, v in ms.items()},
           "k0_over_occluded": round(med["transmit_k0"] / med["occluded"], 4),
           "k8_over_occluded": round(med["transmit_k8"] / med["occluded"], 4),
           "k0_over_occluded_permuted": round(med["transmit_k0_permuted"] / med["occluded_permuted"], 4),
           "k8_over_occluded_permuted": round(med["transmit_k8_permuted"] / med["occluded_permuted"], 4),
           "points_glass_over_points": round(med["points_glass"] / med["points"], 4),
           "occluded_fraction": round(float(occ.float().mean()), 4),
           "glass_shapes": sum(1 for i in range(built.desc.n_shapes) if built.desc.shapes[i].material == dt.DT_MAT_GLASS),
           "panes_nonzero_equals_occluded": same, "max_panes_0_equals_points_occlusion": same_pts}
    scene.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
