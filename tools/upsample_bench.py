"""Guided upsampling of previews (include/dt.h dt_upsample; dt_upsample.hip): what a mixed-resolution
preview costs beside the full-resolution frame it stands in for, and what it loses. One JSON line.

    python tools/upsample_bench.py [--reps 7] [--dump FILE.npz]
        final(240) (the C3 camera) at 1920x1080, 64 spp, everything on the device, one process. First the
        full-resolution frame through the existing render call (dt_render, the parent commit's kernels:
        the yardstick; median kernel ms of `reps` after a warm-up). Then for s = 2 and s = 4: the trace ms
        of the render at low_res_globals(g, s), the ms of the two feature passes (dt_render_features at
        both resolutions), the HIP-event ms of dt_upsample (default parameters) and of a device-to-device
        copy moving the kernel's compulsory byte count (40 B per full-resolution pixel: A, N, Z read and out
        written, plus 40 B per low-resolution pixel read; hipMemcpyAsync of half that many bytes, which
        reads and writes each once), their sum and its ratio to the full frame. Quality against the
        full-resolution frame: mean squared error and PSNR (peak 255) of guided upsampling, of pixel
        replication, and of guided upsampling with sigma_albedo = +inf. Then the sweep the defaults of
        dt_upsample_params_default were chosen on: the MSE over a grid of sigmas at both
        factors, through the kernel.
"""
import argparse
import ctypes
import itertools
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("albedo", "normal", "depth")
INF = float("inf")


def timed_upsample(dt, g, lo, f_lo, f_hi, p, out):
    from distraytracer_amd._lib import Features
    fl, fh = Features(), Features()
    for k in NAMES:
        setattr(fl, k, f_lo[k].data_ptr())
        setattr(fh, k, f_hi[k].data_ptr())
    ms = ctypes.c_float(0)
    dt.check(dt.lib.dt_upsample(g.xRes, g.yRes, lo.data_ptr(), ctypes.byref(fl), ctypes.byref(fh), ctypes.byref(p),
                                out.data_ptr(), 1, None, ctypes.byref(ms)), "dt_upsample")
    return ms.value


def timed_copy(torch, dst, src):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    dst.copy_(src)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def mse_psnr(torch, a, full):
    d = a.double() - full.double()
    ok = ~torch.isnan(d)
    mse = float((d[ok] ** 2).mean())
    return round(mse, 4), round(10.0 * math.log10(255.0 ** 2 / mse), 3) if mse > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dump")
    a = ap.parse_args()
    import torch

    import bench
    import distraytracer_amd as dt
    med = statistics.median
    g, built = bench.build_globals(dt, "c3")
    g.antialias_samples = 64
    W, H = g.xRes, g.yRes
    scene = dt.Scene(built, g)
    full = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    dt.render(scene, g, 240, full)   # warm-up
    full_ms = med(dt.render(scene, g, 240, full).kernel_ms for _ in range(a.reps))
    st = dt.Stats()
    f_hi = dt.render_features(scene, g, 240, planes=NAMES, stats=st)
    hi_feat = []
    for _ in range(a.reps):
        dt.render_features(scene, g, 240, planes=NAMES, out=f_hi, stats=st)
        hi_feat.append(st.kernel_ms)
    scene.close()
    res = {"bench": "upsample_c3_1080p_64spp", "reps": a.reps, "full_frame_ms": round(full_ms, 4),
           "features_hi_ms": round(med(hi_feat), 4)}
    out = torch.empty_like(full)
    dump = {"full": full.cpu().numpy()}
    sweeps = {}
    for s in (2, 4):
        g_lo = dt.low_res_globals(g, s)
        scene = dt.Scene(built, g_lo)
        lo = torch.zeros(3 * g_lo.xRes * g_lo.yRes, dtype=torch.float32, device="cuda")
        dt.render(scene, g_lo, 240, lo)
        trace = med(dt.render(scene, g_lo, 240, lo).kernel_ms for _ in range(a.reps))
        f_lo = dt.render_features(scene, g_lo, 240, planes=NAMES, stats=st)
        lo_feat = []
        for _ in range(a.reps):
            dt.render_features(scene, g_lo, 240, planes=NAMES, out=f_lo, stats=st)
            lo_feat.append(st.kernel_ms)
        scene.close()
        p = dt.upsample_params_default()
        p.factor = s
        n_bytes = 40 * W * H + 40 * g_lo.xRes * g_lo.yRes
        src = torch.empty(n_bytes // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        timed_upsample(dt, g, lo, f_lo, f_hi, p, out)
        timed_copy(torch, dst, src)
        up, cp = [], []
        for _ in range(a.reps):   # alternating
            up.append(timed_upsample(dt, g, lo, f_lo, f_hi, p, out))
            cp.append(timed_copy(torch, dst, src))
        up_ms, cp_ms, feat_ms = med(up), med(cp), med(lo_feat) + med(hi_feat)
        total = trace + feat_ms + up_ms
        q = {"guided": mse_psnr(torch, out, full)}
        rep = lo.view(g_lo.yRes, 1, g_lo.xRes, 1, 3).expand(-1, s, -1, s, -1).reshape(-1)
        q["replicated"] = mse_psnr(torch, rep, full)
        p.sigma_albedo = INF
        q["guided_sigma_albedo_inf"] = mse_psnr(torch, dt.upsample(g, lo, f_lo, f_hi, p), full)
        rows = []
        for sn, sz, sa in itertools.product((0.125, 0.25, 0.5, 1.0, INF), (0.025, 0.05, 0.1, 0.2, 0.4, INF),
                                            (0.0625, 0.125, 0.25, 0.5, 1.0, INF)):
            p.sigma_normal, p.sigma_depth, p.sigma_albedo = sn, sz, sa
            rows.append((mse_psnr(torch, dt.upsample(g, lo, f_lo, f_hi, p, out=out), full)[0], sn, sz, sa))
        sweeps[s] = {(sn, sz, sa): m for m, sn, sz, sa in rows}
        rows.sort()
        res["x%d" % s] = {"low_res": "%dx%d" % (g_lo.xRes, g_lo.yRes), "trace_ms": round(trace, 4),
                          "features_lo_ms": round(med(lo_feat), 4), "features_both_ms": round(feat_ms, 4),
                          "upsample_kernel_ms": round(up_ms, 4), "copy_same_bytes_ms": round(cp_ms, 4),
                          "compulsory_bytes": n_bytes, "upsample_GBps": round(n_bytes / (up_ms / 1e3) / 1e9, 1),
                          "copy_GBps": round(n_bytes / (cp_ms / 1e3) / 1e9, 1), "sum_ms": round(total, 4),
                          "sum_over_full_frame": round(total / full_ms, 4),
                          "mse_psnr": q,
                          "sweep": {"grid": len(rows), "worst_mse": rows[-1][0],
                                    "best": [{"mse": m, "sigma_normal": sn, "sigma_depth": sz, "sigma_albedo": sa}
                                             for m, sn, sz, sa in rows[:6]]}}
        dump.update({"lo%d" % s: lo.cpu().numpy(), **{"lo%d_%s" % (s, k): v.cpu().numpy() for k, v in f_lo.items()}})
    # one set of defaults for every factor: the grid point with the smallest sum of the two MSEs, each over its own best
    both = sorted((sum(sweeps[s][k] / min(sweeps[s].values()) for s in sweeps), k) for k in sweeps[2])
    res["sweep_both_factors_best"] = [{"sum_of_mse_over_best": round(v, 4), "sigma_normal": k[0], "sigma_depth": k[1],
                                       "sigma_albedo": k[2]} for v, k in both[:6]]
    p = dt.upsample_params_default()
    res["params"] = {k: getattr(p, k) for k, _ in p._fields_ if k != "_pad"}
    if a.dump:
        import numpy as np
        np.savez(a.dump, **dump, **{"hi_" + k: v.cpu().numpy() for k, v in f_hi.items()})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
