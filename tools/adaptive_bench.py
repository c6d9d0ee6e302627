#!/usr/bin/env python3
"""What adaptive sampling saves (BASELINE.md "Adaptive sampling"): buildFinal(240) with the OBJ models,
1920x1080, 256 spp (C4's settings) on one GPU. Run by hand; not part of bench.py.

A full Progressive run (four one-chunk windows and the resolve) is the yardstick. For every --tol, an
AdaptiveProgressive run of the same frame (min_samples 64) reports

  * samples taken as a share of pixels * spp, and the pixels traced per window,
  * wall time (host clock around the synchronous steps and the resolve) against the full run's,
  * the device time of the selection kernels alone, per window (dt_adapt_select_ms),
  * max and RMS difference, in grey levels, from the full-spp image.

Warm (--warmup runs of each first), the median of --reps. Prints one JSON line.

    python tools/adaptive_bench.py [--tol 0.25 0.5 1 2] [--reps 5] [--warmup 1] [--config c4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, nargs="+", default=[0.25, 0.5, 1.0, 2.0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="c4", choices=("c3", "c4"))
    args = ap.parse_args()
    import torch

    import bench
    import distraytracer_amd as dt

    torch.cuda.set_device(0)
    g, built = bench.build_globals(dt, args.config)
    scene = dt.Scene(built, g)
    n_px = g.xRes * g.yRes
    med = statistics.median

    def full_run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = dt.Progressive(scene, g, 240).run()
        img = p.image()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, img

    def adaptive_run(tol):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = dt.AdaptiveProgressive(scene, g, 240, tol=tol)
        px, sel = [], []
        while not p.done:
            st = p.step()
            px.append(int(st.pixels))
            sel.append(dt.adapt_select_ms(scene))
        img = p.image()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, img, p, px, sel

    for _ in range(args.warmup):
        full_run()
        adaptive_run(args.tol[0])
    t_full = []
    for _ in range(args.reps):
        ms, ref = full_run()
        t_full.append(ms)
    rows = []
    for tol in args.tol:
        ts, sels = [], []
        for _ in range(args.reps):
            ms, img, p, px, sel = adaptive_run(tol)
            ts.append(ms)
            sels.append(sel)
        diff = (img.double() - ref.double()).abs()
        rows.append({
            "tol": tol, "samples_share": round(p.samples_taken / (n_px * p.spp), 4), "pixels_per_window": px,
            "wall_ms": round(med(ts), 2), "wall_vs_full": round(med(ts) / med(t_full), 4),
            "select_ms_per_window": [round(med([s[k] for s in sels]), 4) for k in range(len(px))],
            "max_diff": round(float(diff.max()), 3), "rms_diff": round(float((diff * diff).mean().sqrt()), 4),
        })
    scene.close()
    print(json.dumps({"config": args.config, "xRes": g.xRes, "yRes": g.yRes, "spp": dt._spp(g), "max_depth": g.max_depth,
                      "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
                      "full_wall_ms": round(med(t_full), 2), "rows": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
