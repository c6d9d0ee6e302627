"""Preview denoising (include/dt.h dt_denoise; dt_denoise.hip): its cost beside the sample window it
accompanies, and its quality. One JSON line per mode.

    python tools/denoise_bench.py [--procs 3] [--reps 7]
        Cost. final(240) (the C3 camera) at 1920x1080: the preview and the planes of one 64-sample window,
        default parameters, everything on the device. HIP-event ms of `reps` dt_denoise launches after a
        warm-up, in each of `procs` fresh processes, and in the same processes the dt_render_window time of
        that 64-sample window (the parent commit's kernels: the yardstick). The condition: the denoise time
        is below the window time. The level kernel: dt_denoise with 1..6 levels, each level's time the
        difference of two medians, against its compulsory traffic (three 16-byte records read and one
        written per pixel and level; the last level writes 12 bytes).
    python tools/denoise_bench.py --quality [--dump FILE.npz]
        Quality. final(240) at 160x90, 1024 spp: RMSE over the 0..255 floats, against the full frame, of
        the raw 64-sample preview and of the denoised one, and their ratio (the gate of
        tests/test_gpu_denoise.py is ratio < 1). --dump keeps preview, planes and full frame.
    python tools/denoise_bench.py --sweep FILE.npz
        No GPU: the ratio over a grid of sigmas on a dump, through the host loop (the same bits); how the
        defaults of dt_denoise_params_default were chosen.
    --variance with any of the three: the variance-guided filter (dt_variance + dt_denoise_var) as well.
        Cost: in the same processes, the HIP-event ms of dt_variance + dt_denoise_var (5 levels, defaults) on
        the sums of one adaptive 64-sample window, beside dt_denoise and the window. Quality: the preview of
        an AdaptiveProgressive that never stops a pixel (the same 64-sample preview) through dt_denoise and
        dt_denoise_var, and one adaptive case (tol 1.0, stopped after 4 windows) with the raw, plain and
        variance-guided ratios against the full frame; --dump keeps the variance planes too. Sweep: the
        host loop over sigma_variance x variance_floor x the guide sigmas, on both dumped cases.
"""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080


def timed_denoise(dt, g, colour, feats, p, work, out):
    import ctypes
    from distraytracer_amd._lib import Features
    f = Features()
    for k in ("albedo", "normal", "depth"):
        setattr(f, k, feats[k].data_ptr())
    ms = ctypes.c_float(0)
    dt.check(dt.lib.dt_denoise(g.xRes, g.yRes, colour.data_ptr(), ctypes.byref(f), ctypes.byref(p), out.data_ptr(),
                               work.data_ptr(), 1, None, ctypes.byref(ms)), "dt_denoise")
    return ms.value


def timed_variance_denoise(dt, g, sums, colour, feats, p, var, work, out):
    """(HIP-event ms of dt_variance + dt_denoise_var on the null stream, dt_denoise_var's own kernel_ms)"""
    import ctypes

    import torch
    from distraytracer_amd._lib import Features
    f = Features()
    for k in ("albedo", "normal", "depth"):
        setattr(f, k, feats[k].data_ptr())
    ms = ctypes.c_float(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    dt.variance(g, sums.accum, sums.accum2, sums.count, out=var)
    dt.check(dt.lib.dt_denoise_var(g.xRes, g.yRes, colour.data_ptr(), var.data_ptr(), ctypes.byref(f), ctypes.byref(p),
                                   out.data_ptr(), work.data_ptr(), 1, None, ctypes.byref(ms)), "dt_denoise_var")
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), ms.value


def child(reps, variance=False):
    import ctypes

    import torch

    import bench
    import distraytracer_amd as dt
    g, built = bench.build_globals(dt, "c3")
    g.xRes, g.yRes, g.antialias_samples = W, H, 64
    scene = dt.Scene(built, g)
    prog = dt.Progressive(scene, g, 240)
    prog.step()   # warm-up of the window render; its samples are the preview
    colour = prog.image()
    feats = prog.features(planes=("albedo", "normal", "depth"))
    win = []
    for _ in range(reps):
        prog.accum.zero_()
        win.append(dt.render_window(scene, g, 240, prog.accum, 0, 64).kernel_ms)
    p = dt.denoise_params_default()
    work = torch.empty(int(dt.lib.dt_denoise_workspace_floats(W, H, ctypes.byref(p))), dtype=torch.float32, device="cuda")
    out = torch.empty_like(colour)
    timed_denoise(dt, g, colour, feats, p, work, out)   # warm-up
    by_levels = {}
    for levels in (5, 1, 2, 3, 4, 6):
        p.levels = levels
        timed_denoise(dt, g, colour, feats, p, work, out)
        by_levels[levels] = sorted(timed_denoise(dt, g, colour, feats, p, work, out) for _ in range(reps))
    res = {"window_ms": sorted(win), "denoise_ms": {str(k): v for k, v in by_levels.items()}}
    if variance:
        # the sums of one adaptive 64-sample window (no pixel can stop before it): the same samples
        sums = dt.AdaptiveProgressive(scene, g, 240, tol=0.0, min_samples=64)
        sums.step()
        vp = dt.denoise_var_params_default()
        vp.levels = 5
        var = torch.empty_like(colour)
        vwork = torch.empty(int(dt.lib.dt_denoise_var_workspace_floats(W, H, ctypes.byref(vp))), dtype=torch.float32,
                            device="cuda")
        p.levels = 5
        timed_variance_denoise(dt, g, sums, colour, feats, vp, var, vwork, out)   # warm-up
        both, own, plain = [], [], []
        for _ in range(reps):   # alternating with dt_denoise, 5 levels
            a, b = timed_variance_denoise(dt, g, sums, colour, feats, vp, var, vwork, out)
            both.append(a)
            own.append(b)
            plain.append(timed_denoise(dt, g, colour, feats, p, work, out))
        res.update({"variance_plus_denoise_var_ms": sorted(both), "denoise_var_ms": sorted(own),
                    "denoise_ms_alternating": sorted(plain)})
    scene.close()
    print(json.dumps(res), flush=True)


def cost(procs, reps, variance=False):
    runs = []
    for _ in range(procs):
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)]
                           + (["--variance"] if variance else []), check=True,
                           stdout=subprocess.PIPE, timeout=600).stdout.decode()
        runs.append(json.loads(o.strip().splitlines()[-1]))
    med = statistics.median
    window = med([med(r["window_ms"]) for r in runs])
    den = {k: med([med(r["denoise_ms"][str(k)]) for r in runs]) for k in range(1, 7)}
    n_px = W * H
    levels = []
    for l in range(1, 6):   # level l alone: 1..l+1 levels minus 1..l levels (level 0 shares its launch with prepare)
        ms = den[l + 1] - den[l]
        levels.append({"level": l, "step": 1 << l, "ms": round(ms, 4),
                       "compulsory_GBps": round(64 * n_px / (ms / 1e3) / 1e9, 1) if ms > 0 else None})
    res = {"bench": "denoise_c3_1080p_64spp_window", "procs": procs, "reps": reps,
           "denoise_ms_default": round(den[5], 4),
           "denoise_ms_per_process": [round(med(r["denoise_ms"]["5"]), 4) for r in runs],
           "window_ms": round(window, 4), "window_ms_per_process": [round(med(r["window_ms"]), 4) for r in runs],
           "denoise_over_window": round(den[5] / window, 4),
           "denoise_ms_by_levels": {str(k): round(v, 4) for k, v in den.items()},
           "prepare_plus_level0_ms": round(den[1], 4), "level_kernel": levels,
           "compulsory_bytes_per_level": 64 * n_px}
    if variance:
        both = med([med(r["variance_plus_denoise_var_ms"]) for r in runs])
        own = med([med(r["denoise_var_ms"]) for r in runs])
        plain = med([med(r["denoise_ms_alternating"]) for r in runs])
        res.update({"variance_plus_denoise_var_ms": round(both, 4),
                    "variance_plus_denoise_var_ms_per_process": [round(med(r["variance_plus_denoise_var_ms"]), 4) for r in runs],
                    "denoise_var_ms": round(own, 4), "denoise_ms_alternating": round(plain, 4),
                    "variance_plus_denoise_var_over_denoise": round(both / plain, 4),
                    "variance_plus_denoise_var_over_window": round(both / window, 4)})
    print(json.dumps(res), flush=True)


def rmse_ratio(raw, clean, full):
    import numpy as np
    raw, clean, full = (np.asarray(v, np.float64) for v in (raw, clean, full))
    ok = ~(np.isnan(raw) | np.isnan(clean) | np.isnan(full))
    a = float(np.sqrt(np.mean((raw[ok] - full[ok]) ** 2)))
    b = float(np.sqrt(np.mean((clean[ok] - full[ok]) ** 2)))
    return a, b, b / a


def quality(dump):
    import numpy as np

    import distraytracer_amd as dt
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples = 160, 90, 1024
    scene = dt.Scene(built, g)
    prog = dt.Progressive(scene, g, 240)
    prog.step()
    raw = prog.image().cpu().numpy()
    feats = {k: v.cpu().numpy() for k, v in prog.features(planes=("albedo", "normal", "depth")).items()}
    clean = prog.denoised().cpu().numpy()
    prog.run()
    full = prog.image().cpu().numpy()
    scene.close()
    if dump:
        np.savez(dump, raw=raw, full=full, **feats)
    a, b, r = rmse_ratio(raw, clean, full)
    p = dt.denoise_params_default()
    print(json.dumps({"bench": "denoise_quality_final240_160x90_64_of_1024spp", "rmse_raw": round(a, 4),
                      "rmse_denoised": round(b, 4), "ratio": round(r, 4),
                      "params": {k: getattr(p, k) for k, _ in p._fields_}}), flush=True)


def quality_variance(dump):
    import numpy as np

    import distraytracer_amd as dt
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples = 160, 90, 1024
    scene = dt.Scene(built, g)
    planes = ("albedo", "normal", "depth")
    # never stops a pixel: the 64-sample preview of quality(), and the full frame
    prog = dt.AdaptiveProgressive(scene, g, 240, tol=0.0, min_samples=1024)
    prog.step()
    raw, var = prog.image().cpu().numpy(), prog.variance().cpu().numpy()
    feats = {k: v.cpu().numpy() for k, v in prog.features(planes=planes).items()}
    plain, guided = prog.denoised().cpu().numpy(), prog.denoised(variance=True).cpu().numpy()
    prog.run()
    full = prog.image().cpu().numpy()
    # the adaptive case: tol 1.0, stopped after 4 windows
    ad = dt.AdaptiveProgressive(scene, g, 240, tol=1.0)
    for _ in range(4):
        ad.step()
    a_raw, a_var, a_count = ad.image().cpu().numpy(), ad.variance().cpu().numpy(), ad.count.cpu().numpy()
    a_feats = {k: v.cpu().numpy() for k, v in ad.features(planes=planes).items()}
    a_plain, a_guided = ad.denoised().cpu().numpy(), ad.denoised(variance=True).cpu().numpy()
    scene.close()
    if dump:
        np.savez(dump, raw=raw, full=full, variance=var, a_raw=a_raw, a_variance=a_var, a_count=a_count,
                 **feats, **{"a_" + k: v for k, v in a_feats.items()})
    p = dt.denoise_var_params_default()
    r0, r1 = rmse_ratio(raw, plain, full), rmse_ratio(raw, guided, full)
    b0, b1 = rmse_ratio(a_raw, a_plain, full), rmse_ratio(a_raw, a_guided, full)
    print(json.dumps({"bench": "denoise_var_quality_final240_160x90_64_of_1024spp", "rmse_raw": round(r0[0], 4),
                      "rmse_denoise": round(r0[1], 4), "rmse_denoise_var": round(r1[1], 4),
                      "ratio_denoise": round(r0[2], 4), "ratio_denoise_var": round(r1[2], 4),
                      "adaptive_tol1_4_windows": {"share_of_pixels_at_64": round(float((a_count == 64).mean()), 4),
                                                  "rmse_raw": round(b0[0], 4), "rmse_denoise": round(b0[1], 4),
                                                  "rmse_denoise_var": round(b1[1], 4), "ratio_denoise": round(b0[2], 4),
                                                  "ratio_denoise_var": round(b1[2], 4)},
                      "params": {k: getattr(p, k) for k, _ in p._fields_ if k != "_pad"}}), flush=True)


def sweep_variance(path):
    import numpy as np

    import distraytracer_amd as dt
    d = np.load(path)
    g = dt.globals_default()
    g.xRes, g.yRes = 160, 90
    out = {"bench": "denoise_var_sigma_sweep"}
    for case, pre in (("preview_64_of_1024", ""), ("adaptive_tol1_4_windows", "a_")):
        feats = {k: d[pre + k] for k in ("albedo", "normal", "depth")}
        raw, var = d[pre + "raw"], d[pre + "variance"]
        rows = []
        for sv, vf, sn, sz, sa in itertools.product((1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0),
                                                    (0.015625, 0.0625, 0.25, 1.0, 4.0, 16.0, 64.0, 256.0),
                                                    (0.03125, 0.0625, 0.125), (0.003125, 0.00625, 0.0125),
                                                    (0.015625, 0.03125, 0.0625)):
            p = dt.DenoiseVarParams(5, 1, sn, sz, sa, sv, vf, 0.0)
            a, b, r = rmse_ratio(raw, dt.denoise(g, raw, feats, p, variance=var), d["full"])
            rows.append((r, sv, vf, sn, sz, sa))
        rows.sort()
        at = {(sv, vf): r for r, sv, vf, sn, sz, sa in rows if (sn, sz, sa) == rows[0][3:]}
        out[case] = {"grid": len(rows),
                     "best": [{"ratio": round(r, 4), "sigma_variance": sv, "variance_floor": vf, "sigma_normal": sn,
                               "sigma_depth": sz, "sigma_albedo": sa} for r, sv, vf, sn, sz, sa in rows[:8]],
                     "at_best_guides": {"%g/%g" % k: round(v, 4) for k, v in sorted(at.items())},
                     "worst_ratio": round(rows[-1][0], 4)}
    print(json.dumps(out), flush=True)


def sweep(path):
    import numpy as np

    import distraytracer_amd as dt
    d = np.load(path)
    g = dt.globals_default()
    g.xRes, g.yRes = 160, 90
    feats = {k: d[k] for k in ("albedo", "normal", "depth")}
    rows = []
    for sn, sz, sc, sa in itertools.product((0.03125, 0.0625, 0.125, 0.25, 0.5), (0.003125, 0.00625, 0.0125, 0.05, 0.1),
                                            (16.0, 32.0, 48.0, 64.0, 96.0, 128.0),
                                            (0.015625, 0.03125, 0.0625, 0.125, 0.25)):
        p = dt.DenoiseParams(5, 1, sn, sz, sc, sa)
        a, b, r = rmse_ratio(d["raw"], dt.denoise(g, d["raw"], feats, p), d["full"])
        rows.append((r, sn, sz, sc, sa))
    rows.sort()
    print(json.dumps({"bench": "denoise_sigma_sweep", "grid": len(rows),
                      "best": [{"ratio": round(r, 4), "sigma_normal": sn, "sigma_depth": sz, "sigma_colour": sc,
                                "sigma_albedo": sa} for r, sn, sz, sc, sa in rows[:8]],
                      "worst_ratio": round(rows[-1][0], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--dump")
    ap.add_argument("--sweep")
    ap.add_argument("--variance", action="store_true")
    a = ap.parse_args()
    if a.sweep:
        (sweep_variance if a.variance else sweep)(a.sweep)
    elif a.quality:
        (quality_variance if a.variance else quality)(a.dump)
    elif a.child:
        child(a.reps, a.variance)
    else:
        cost(a.procs, a.reps, a.variance)


if __name__ == "__main__":
    main()
