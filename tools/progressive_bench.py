#!/usr/bin/env python3
"""Cost of windowing (BASELINE.md "Progressive"): C4's settings (buildFinal(240) with the OBJ models,
1920x1080, 256 spp, depth 8) on one GPU, the device time of

  * one dt_render (the one-shot frame: the yardstick),
  * four one-chunk windows (dt_render_window_async) plus one dt_resolve on the same stream,
  * one window alone, per window, and one dt_resolve alone.

HIP events (torch.cuda.Event on the launches' stream), warm (--warmup renders of each first), the
median of --reps (>= 5). Checks once that the resolved image is the one-shot image bit for bit.
Prints one JSON line.

    python tools/progressive_bench.py [--reps 7] [--warmup 2] [--config c4]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="c4", choices=("c3", "c4"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5")
    import torch

    import bench
    import distraytracer_amd as dt

    torch.cuda.set_device(0)
    g, built = bench.build_globals(dt, args.config)
    scene = dt.Scene(built, g)
    n = 3 * g.xRes * g.yRes
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    img = torch.zeros(n, dtype=torch.float32, device="cuda")
    p = dt.Progressive(scene, g, 240)
    spp, chunks = p.spp, (p.spp + 63) // 64
    wins = [(64 * c, min(64 * c + 64, spp)) for c in range(chunks)]
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def one_shot():
        dt.render_async(scene, g, 240, out, stream=stream)

    def windows():
        p.accum.zero_()
        for b, e in wins:
            dt.render_window_async(scene, g, 240, p.accum, b, e, stream=stream)
        dt.check(dt.lib.dt_resolve(ctypes.byref(g), None, p.accum.data_ptr(), spp, img.data_ptr(), 1, stream, None), "dt_resolve")

    def resolve_only():
        dt.check(dt.lib.dt_resolve(ctypes.byref(g), None, p.accum.data_ptr(), spp, img.data_ptr(), 1, stream, None), "dt_resolve")

    def one_window(b, e):
        return lambda: dt.render_window_async(scene, g, 240, p.accum, b, e, stream=stream)

    for _ in range(args.warmup):
        one_shot()
        windows()
    torch.cuda.synchronize()
    bit_identical = bool(torch.equal(out.view(torch.int32), img.view(torch.int32)))
    t_one, t_win, t_res = [], [], []
    t_per = [[] for _ in wins]
    for _ in range(args.reps):   # interleaved, so drift lands on every series alike
        t_one.append(timed(one_shot))
        t_win.append(timed(windows))
        t_res.append(timed(resolve_only))
        p.accum.zero_()
        for k, (b, e) in enumerate(wins):
            t_per[k].append(timed(one_window(b, e)))
    scene.close()
    med = statistics.median
    res = {
        "config": args.config, "xRes": g.xRes, "yRes": g.yRes, "spp": spp, "max_depth": g.max_depth,
        "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
        "one_shot_ms": round(med(t_one), 3), "one_shot_ms_min_max": [round(min(t_one), 3), round(max(t_one), 3)],
        "windows_plus_resolve_ms": round(med(t_win), 3),
        "windows_plus_resolve_ms_min_max": [round(min(t_win), 3), round(max(t_win), 3)],
        "window_ms": [round(med(t), 3) for t in t_per],
        "resolve_ms": round(med(t_res), 4),
        "windowing_overhead": round(med(t_win) / med(t_one) - 1.0, 4),
        "accum_bytes": int(p.accum.numel()) * 8,
        "bit_identical": bit_identical,
    }
    print(json.dumps(res))
    return 0 if bit_identical else 1


if __name__ == "__main__":
    sys.exit(main())
