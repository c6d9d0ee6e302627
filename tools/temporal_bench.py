"""Temporal reuse for animation previews (include/dt.h dt_reproject; dt_temporal.hip): what accumulating the
previews of consecutive frames buys, and what it costs. Single process, the frames in order (tools/animate.py
renders frames out of order and is not involved). One JSON line per frame or per measurement.

    python tools/temporal_bench.py [--frames 240:288:8] [--res 160x90] [--spp 64] [--depth 10] [--denoise]
                                   [--reference-spp 1024] [--alpha-min A --max-history M --depth-tol D --normal-tol N --albedo-tol A]
        Sequence. --frames are BUILDER frames of "final", start:stop:step (the animation's frame n is builder
        frame 8 n, and the skeleton has a posture only for (int)frame a multiple of 8: 240:241:0.125 is the eighth
        steps between two of them). Each frame is built, its preview rendered with a seed of its own and
        its feature planes taken, and the preview is pushed into a TemporalAccumulator. Per frame: the share of
        pixels by history length; with --reference-spp the RMSE over the 0..255 floats against that frame at N
        samples (another seed) of the raw preview and the accumulated one, and with --denoise of dt_denoise of
        each (spatial alone, spatial after temporal), all over the pixels that are no NaN in any of them.
    python tools/temporal_bench.py --sweep [--frames ...] --reference-spp N
        The sequence is rendered once and kept; the accumulation is repeated over a grid of the five parameters.
        Per combination: the mean over the frames after the first of RMSE(accumulated) / RMSE(raw) and the mean
        history length at the last frame; the combinations in ascending order of the ratio.
    python tools/temporal_bench.py --cost [--res 1920x1080] [--reps 9]
        Cost. final(240) at 64 spp: HIP-event ms of dt_reproject (the planes of frame 240 as the previous frame
        under the camera of builder frame 241 - 1/64, a turn of 0.41 degrees: a sub-pixel gather at 160x90, five
        pixels at 1920x1080), with and without variance planes, of
        dt_denoise (defaults) on the same frame, alternating, and dt_render_window's kernel time of the
        64-sample window they accompany; every repetition's time, sorted, and the medians.
"""
import argparse
import itertools
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LENGTH_BINS = ((0, 0), (1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 1 << 30))


def frange(s):
    a, b, c = (float(v) for v in s.split(":"))
    out = []
    while a < b:
        out.append(a)
        a += c
    return out


def build(dt, frame, W, H, depth):
    g = dt.globals_default()   # fresh globals per frame, as tools/animate.py
    g.use_model = 0
    built = dt.build_scene("final", frame, g)
    g.xRes, g.yRes, g.max_depth = W, H, depth
    return g, dt.Scene(built, g)


def render(dt, scene, g, frame, spp, seed, features):
    import torch
    gs = dt.Globals.from_buffer_copy(g)
    gs.antialias_samples, gs.seed = spp, seed
    out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
    dt.render(scene, gs, int(frame), out)
    return out, (dt.render_features(scene, gs, int(frame)) if features else None)


def rmse(a, ref, ok):
    import torch
    d = (a.double() - ref.double())[ok]
    return float(torch.sqrt(torch.mean(d * d)))


def shares(length):
    n = length.numel()
    return {("%d" % lo if lo == hi else "%d+" % lo if hi > 1000 else "%d-%d" % (lo, hi)):
            round(float(((length >= lo) & (length <= hi)).sum()) / n, 4) for lo, hi in LENGTH_BINS}


def sequence(dt, args, params):
    """render the frames in order; yields (frame, g, raw, feats, ref or None)"""
    W, H = (int(v) for v in args.res.split("x"))
    for k, frame in enumerate(frange(args.frames)):
        g, scene = build(dt, frame, W, H, args.depth)
        raw, feats = render(dt, scene, g, frame, args.spp, 1000 + k, True)
        ref = render(dt, scene, g, frame, args.reference_spp, 7, False)[0] if args.reference_spp else None
        scene.close()
        yield frame, g, raw, feats, ref


def run_sequence(dt, args, params):
    import torch
    acc = dt.TemporalAccumulator(params)
    for frame, g, raw, feats, ref in sequence(dt, args, params):
        out = acc.push(g, raw, feats)
        length = acc.history_length()
        line = {"frame": frame, "res": args.res, "spp": args.spp, "share_by_history_length": shares(length),
                "mean_history_length": round(float(length.mean()), 3)}
        imgs = {"raw": raw, "accumulated": out}
        if args.denoise:
            imgs["denoised"] = dt.denoise(g, raw, feats)
            imgs["accumulated_denoised"] = dt.denoise(g, out, feats)
        if ref is not None:
            ok = ~torch.isnan(ref)
            for v in imgs.values():
                ok &= ~torch.isnan(v)
            r = {k: rmse(v, ref, ok) for k, v in imgs.items()}
            line["rmse"] = {k: round(v, 4) for k, v in r.items()}
            line["accumulated_over_raw"] = round(r["accumulated"] / r["raw"], 4)
            if args.denoise:
                line["accumulated_denoised_over_denoised"] = round(r["accumulated_denoised"] / r["denoised"], 4)
        print(json.dumps(line), flush=True)


def run_sweep(dt, args, params):
    import torch
    from distraytracer_amd._lib import TemporalParams
    if not args.reference_spp:
        sys.exit("--sweep needs --reference-spp")
    frames = list(sequence(dt, args, params))
    grid = itertools.product((0.05, 0.2), (8.0, 32.0), (0.005, 0.02, 0.08), (0.1, 0.25, 0.5),
                             (0.03125, 0.0625, 0.125, 0.25, float("inf")))
    rows = []
    for a, m, d, n, t in grid:
        acc = dt.TemporalAccumulator(TemporalParams(1, a, m, d, n, t))
        ratios = []
        for k, (frame, g, raw, feats, ref) in enumerate(frames):
            out = acc.push(g, raw, feats)
            if k:
                ok = ~(torch.isnan(ref) | torch.isnan(raw) | torch.isnan(out))
                ratios.append(rmse(out, ref, ok) / rmse(raw, ref, ok))
        rows.append({"alpha_min": a, "max_history": m, "depth_tol": d, "normal_tol": n, "albedo_tol": t,
                     "mean_accumulated_over_raw": round(statistics.mean(ratios), 4), "last": round(ratios[-1], 4),
                     "mean_history_length_last": round(float(acc.history_length().mean()), 3)})
    for r in sorted(rows, key=lambda r: r["mean_accumulated_over_raw"]):
        print(json.dumps(r), flush=True)


def run_cost(dt, args, params):
    import ctypes

    import torch
    from distraytracer_amd._lib import Features
    W, H = (int(v) for v in args.res.split("x"))
    g, scene = build(dt, 240, W, H, args.depth)
    g.antialias_samples = 64
    prog = dt.Progressive(scene, g, 240)
    prog.step()   # warm-up of the window render; its samples are the preview
    colour, feats = prog.image(), prog.features()
    window = []
    for _ in range(args.reps):
        prog.accum.zero_()
        window.append(dt.render_window(scene, g, 240, prog.accum, 0, 64).kernel_ms)
    scene.close()
    g1 = dt.globals_default()
    dt.build_scene("final", 241 - 1.0 / 64, g1)   # (241 has no posture in the bone table; the camera is continuous)
    g1.xRes, g1.yRes = W, H
    cur, prev = dt.camera(g1), dt.camera(g)
    var = torch.full_like(colour, 4.0)
    first = dt.reproject(prev, colour, feats, None, None, None, params, variance=var)   # frame 240's history
    hist = first[1]
    plain_hist = {k: hist[k] for k in ("colour", "len")}
    p = dt.denoise_params_default()
    f = Features()
    for k in ("albedo", "normal", "depth"):
        setattr(f, k, feats[k].data_ptr())
    work = torch.empty(int(dt.lib.dt_denoise_workspace_floats(W, H, ctypes.byref(p))), dtype=torch.float32, device="cuda")
    out = torch.empty_like(colour)
    out_var = torch.empty_like(colour)
    ho = {"colour": torch.empty_like(colour), "var": torch.empty_like(colour), "len": torch.empty_like(hist["len"])}

    def t_denoise():
        ms = ctypes.c_float(0)
        dt.check(dt.lib.dt_denoise(W, H, colour.data_ptr(), ctypes.byref(f), ctypes.byref(p), out.data_ptr(),
                                   work.data_ptr(), 1, None, ctypes.byref(ms)), "dt_denoise")
        return ms.value

    def t_reproject(with_var):
        return dt.reproject(cur, colour, feats, prev, feats, hist if with_var else plain_hist, params,
                            variance=var if with_var else None, out=out, out_var=out_var if with_var else None,
                            out_history=ho if with_var else {k: ho[k] for k in ("colour", "len")}, timed=True)[3]

    t_denoise(), t_reproject(False), t_reproject(True)   # warm-up
    den, rep, repv = [], [], []
    for _ in range(args.reps):   # alternating
        rep.append(t_reproject(False))
        den.append(t_denoise())
        repv.append(t_reproject(True))
    found = float((ho["len"] > 1).float().mean())
    med = statistics.median
    n_px = W * H
    # compulsory traffic without variance: reads C, A, N (36 B), Z (4), shape (4) and, once per previous pixel, A', N', Z',
    # shape', history colour and length (48); writes out, history colour and length (28)
    print(json.dumps({"bench": "temporal_cost_final240", "res": args.res, "reps": args.reps,
                      "reproject_ms": sorted(round(v, 4) for v in rep), "reproject_ms_median": round(med(rep), 4),
                      "reproject_var_ms": sorted(round(v, 4) for v in repv), "reproject_var_ms_median": round(med(repv), 4),
                      "denoise_ms": sorted(round(v, 4) for v in den), "denoise_ms_median": round(med(den), 4),
                      "window_ms": sorted(round(v, 4) for v in window), "window_ms_median": round(med(window), 4),
                      "reproject_over_denoise": round(med(rep) / med(den), 4),
                      "reproject_over_window": round(med(rep) / med(window), 6),
                      "share_with_history": round(found, 4),
                      "reproject_compulsory_GBps": round(120 * n_px / (med(rep) / 1e3) / 1e9, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="240:288:8")
    ap.add_argument("--res", default=None)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--denoise", action="store_true")
    ap.add_argument("--reference-spp", type=int, default=0)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--alpha-min", type=float)
    ap.add_argument("--max-history", type=float)
    ap.add_argument("--depth-tol", type=float)
    ap.add_argument("--normal-tol", type=float)
    ap.add_argument("--albedo-tol", type=float)
    args = ap.parse_args()
    args.res = args.res or ("1920x1080" if args.cost else "160x90")

    import torch

    import distraytracer_amd as dt
    if not torch.cuda.is_available():
        sys.exit("temporal_bench.py needs a GPU")
    torch.cuda.set_device(0)
    params = dt.temporal_params_default()
    for name in ("alpha_min", "max_history", "depth_tol", "normal_tol", "albedo_tol"):
        if getattr(args, name) is not None:
            setattr(params, name, getattr(args, name))
    (run_cost if args.cost else run_sweep if args.sweep else run_sequence)(dt, args, params)


if __name__ == "__main__":
    main()
