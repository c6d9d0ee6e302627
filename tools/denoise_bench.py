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


def child(reps):
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
    scene.close()
    print(json.dumps({"window_ms": sorted(win), "denoise_ms": {str(k): v for k, v in by_levels.items()}}), flush=True)


def cost(procs, reps):
    runs = []
    for _ in range(procs):
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], check=True,
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
    a = ap.parse_args()
    if a.sweep:
        sweep(a.sweep)
    elif a.quality:
        quality(a.dump)
    elif a.child:
        child(a.reps)
    else:
        cost(a.procs, a.reps)


if __name__ == "__main__":
    main()
