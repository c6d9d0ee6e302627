"""Ray ordering (include/dt.h dt_ray_order, dt_permute_rows): what sorting caller-supplied rays into coherent
waves costs and what it buys. Single process, the C3 scene (final(240), 1920x1080), the 2^24 primary rays of
tools/rayquery_bench.py in its fixed random permutation (every wave's 64 rays scattered over the frame).
Method as there: HIP-event times, one warm-up of each, the repetitions alternating between the measurements,
min .. median .. max. One JSON line, ms:

    camera, permuted       dt_trace_rays (shape, t) on the rays in camera order and permuted (the parent's figures)
    per preset (default: origin_bits 5, dir_bits 6; camera: origin_bits 0, dir_bits 8 -- all origins lie on the lens):
      order                box + key + radix sort (dt_ray_order's kernel_ms)
      torch_sort           torch.sort(keys, stable=True) on the same keys: a yardstick the C library cannot call
      gather               dt_permute_rows of start and dir
      trace                dt_trace_rays (shape, t) on the gathered rays
      restore              dt_permute_rows of shape and t back to the caller's order
    occluded_*             dt_rays_occluded from the first hits towards each of the five lights: hits in camera
                           order, permuted, and permuted with one order (default preset, keyed on the hits and the
                           segments to the first light) reused for the five lights: order + gather of the hits once,
                           then per light the query and the restore of its answer

and the ratios: ordered trace over camera-order and over permuted trace, the break-even reuse count
(order + gather + restore) / (permuted - ordered), and the sort against its pure traffic bound (per pass
8 bytes read and 8 written per pair at the measured copy bandwidth).

    python tools/rayorder_bench.py [--rays 16777216] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBS = 6.29   # measured HBM copy bandwidth of the MI355X, TB/s


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
        sys.exit("rayorder_bench.py needs a GPU")
    torch.cuda.set_device(0)
    g, built = bench.build_globals(dt, "c3")
    scene = dt.Scene(built, g)
    start_h, dir_h = G.or_primary_ray(g, 240, 0, n)
    start, dir = torch.from_numpy(start_h).cuda(), torch.from_numpy(dir_h).cuda()
    perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()
    start_p, dir_p = start[perm].contiguous(), dir[perm].contiguous()
    del start_h, dir_h

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def planes():
        return {"shape": torch.empty(n, dtype=torch.int32, device="cuda"),
                "t": torch.empty(n, dtype=torch.float32, device="cuda")}

    two, two_p = planes(), planes()
    runs = {"camera": lambda: dt.trace_rays(scene, g, start, dir, out=two)[1].kernel_ms,
            "permuted": lambda: dt.trace_rays(scene, g, start_p, dir_p, out=two_p)[1].kernel_ms}

    presets = {"default": dt.ray_order_params_default(), "camera": dt.ray_order_params_default()}
    presets["camera"].origin_bits, presets["camera"].dir_bits = 0, 8
    state, passes, equal = {}, {}, {}
    for name, p in presets.items():
        B = 3 * p.origin_bits + 2 * p.dir_bits
        passes[name] = (B + 1 + 7) // 8
        o = dt.ray_order(start_p, dir_p, params=p, keys=True)
        st = {"order": o, "s": o.apply(start_p), "d": o.apply(dir_p), "sorted": planes(), "back": planes()}
        state[name] = st

        def f_order(p=p):
            return dt.ray_order(start_p, dir_p, params=p).kernel_ms

        def f_sort(st=st):
            return timed(lambda: torch.sort(st["order"].keys, stable=True))

        def f_gather(st=st):
            return timed(lambda: (st["order"].apply(start_p, out=st["s"]), st["order"].apply(dir_p, out=st["d"])))

        def f_trace(st=st):
            return dt.trace_rays(scene, g, st["s"], st["d"], out=st["sorted"])[1].kernel_ms

        def f_restore(st=st):
            return timed(lambda: [st["order"].restore(st["sorted"][k], out=st["back"][k]) for k in ("shape", "t")])

        runs.update({name + ".order": f_order, name + ".torch_sort": f_sort, name + ".gather": f_gather,
                     name + ".trace": f_trace, name + ".restore": f_restore})

    # visibility from the first hits towards the five lights
    full = {**planes(), "point": torch.empty(n, 3, dtype=torch.float64, device="cuda")}
    dt.trace_rays(scene, g, start, dir, out=full)
    pts = full["point"]
    pts_p = pts[perm].contiguous()
    desc = built.desc
    n_lights = min(5, desc.n_lights)
    centres = [torch.tensor(list(desc.lights[j].center), dtype=torch.float64, device="cuda") for j in range(n_lights)]
    skips = [torch.full((n,), int(desc.lights[j].shape_index), dtype=torch.int32, device="cuda") for j in range(n_lights)]
    seg = [(c[None, :] - pts).contiguous() for c in centres]
    seg_p = [(c[None, :] - pts_p).contiguous() for c in centres]
    vis = dt.ray_order(pts_p, seg_p[0])
    pts_s = vis.apply(pts_p)
    seg_s = [(c[None, :] - pts_s).contiguous() for c in centres]
    occ = [torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3)]
    occ_back = torch.empty(n, dtype=torch.uint8, device="cuda")

    def lights(p, s, out):
        return sum(dt.rays_occluded(scene, g, p, s[j], skip_shape=skips[j], out=out)[1].kernel_ms for j in range(n_lights))

    runs.update({"occluded_camera": lambda: lights(pts, seg, occ[0]),
                 "occluded_permuted": lambda: lights(pts_p, seg_p, occ[1]),
                 "occluded_ordered": lambda: lights(pts_s, seg_s, occ[2]),
                 "occluded_order": lambda: dt.ray_order(pts_p, seg_p[0]).kernel_ms,
                 "occluded_gather": lambda: timed(lambda: vis.apply(pts_p, out=pts_s)),
                 "occluded_restore": lambda: timed(lambda: [vis.restore(occ[2], out=occ_back) for _ in range(n_lights)])})

    for f in runs.values():   # warm-up
        f()
    ms = {k: [] for k in runs}
    for _ in range(args.reps):   # alternating
        for k, f in runs.items():
            ms[k].append(f())
    med = {k: statistics.median(v) for k, v in ms.items()}

    for name, st in state.items():
        equal[name] = bool(torch.equal(st["back"]["shape"], two_p["shape"]) and
                           torch.equal(st["back"]["t"].view(torch.int32), two_p["t"].view(torch.int32)))
        srt, idx = torch.sort(st["order"].keys, stable=True)
        equal[name + ".perm_is_torch_sort"] = bool(torch.equal(idx.to(torch.int32), st["order"].perm))
    equal["occluded"] = bool(torch.equal(occ_back, occ[1]))   # (the last light's answers)

    out = {"bench": "rayorder_c3", "rays": n, "reps": args.reps, "lights": n_lights, "passes": passes,
           "ms": {k: {"min": round(min(v), 4), "median": round(med[k], 4), "max": round(max(v), 4)} for k, v in ms.items()},
           "equal_to_unordered": equal}
    for name in presets:
        fixed = med[name + ".order"] + med[name + ".gather"] + med[name + ".restore"]
        gain = med["permuted"] - med[name + ".trace"]
        bound = passes[name] * 16.0 * n / (COPY_TBS * 1e12) * 1e3
        out[name] = {"ordered_over_camera": round(med[name + ".trace"] / med["camera"], 3),
                     "ordered_over_permuted": round(med[name + ".trace"] / med["permuted"], 3),
                     "order_gather_restore_ms": round(fixed, 4),
                     "chain_ms": round(fixed + med[name + ".trace"], 4),
                     "break_even_reuse": round(fixed / gain, 2) if gain > 0 else None,
                     "sort_traffic_bound_ms": round(bound, 4),
                     "order_over_traffic_bound": round(med[name + ".order"] / bound, 2),
                     "order_over_torch_sort": round(med[name + ".order"] / med[name + ".torch_sort"], 3)}
    chain = med["occluded_order"] + med["occluded_gather"] + med["occluded_ordered"] + med["occluded_restore"]
    out["occluded"] = {"chain_ms": round(chain, 4), "permuted_ms": round(med["occluded_permuted"], 4),
                       "camera_ms": round(med["occluded_camera"], 4),
                       "chain_over_permuted": round(chain / med["occluded_permuted"], 3),
                       "ordered_over_camera": round(med["occluded_ordered"] / med["occluded_camera"], 3)}
    scene.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
