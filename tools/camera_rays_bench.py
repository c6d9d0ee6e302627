"""Camera rays as arrays and their way back to pixels (include/dt.h dt_camera_rays, dt_rays_resolve): what the two
kernels cost on C3 (final(240), 1920x1080, samples 0..7: 16 588 800 rows, 2 x 398 MB of f64 rays). Single process,
no scene. One JSON line of HIP-event ms (min, median, max over the repetitions, after one warm-up of each, the
repetitions alternating):

    camera_rays      dt_camera_rays into device arrays (the call's own kernel_ms)
    memset           hipMemsetAsync of the same two arrays: the time it takes to write those bytes
    h2d_pageable     torch.from_numpy(...).cuda() of the same two arrays made on the host, which is what
                     tools/rayquery_bench.py, multihit_bench.py, rayorder_bench.py and points_occlusion_bench.py
                     pay after generating their rays on the CPU (the generation itself is not timed here)
    h2d_pinned       the same copy from pinned host memory
    resolve          dt_rays_resolve of a 3-wide f64 plane (the dir array) at n_samples = 8, with a shape plane
    resolve_noshape  the same without shape

and camera_rays / memset, the figure DESIGN.md discusses.

    python tools/camera_rays_bench.py [--samples 8] [--reps 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.reps < 3:
        sys.exit("camera_rays_bench.py: at least 3 timed runs")

    import torch

    import bench
    import distraytracer_amd as dt
    if not torch.cuda.is_available():
        sys.exit("camera_rays_bench.py needs a GPU")
    torch.cuda.set_device(0)
    g, _ = bench.build_globals(dt, "c3")
    ns = args.samples
    rows = dt.camera_rays_rows(g, (0, ns))
    start, dir = dt.camera_rays(g, 240, samples=(0, ns))
    nbytes = start.numel() * 8
    hip = ctypes.CDLL("libamdhip64.so")   # the runtime torch loaded
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    a, b = torch.empty_like(start), torch.empty_like(dir)
    host = (start.cpu().numpy(), dir.cpu().numpy())
    pinned = (start.cpu().pin_memory(), dir.cpu().pin_memory())
    shape = (torch.arange(rows, device="cuda", dtype=torch.int32) % 5) - 1   # a fifth of the rows miss
    plane = torch.zeros((rows // ns, 3), dtype=torch.float32, device="cuda")

    def events(f):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run

    def camera():
        ms = ctypes.c_float(0)
        dt.check(dt.lib.dt_camera_rays(ctypes.byref(g), 240, None, 0, ns, ctypes.c_void_p(a.data_ptr()),
                                       ctypes.c_void_p(b.data_ptr()), 1, ctypes.c_void_p(stream), ctypes.byref(ms)),
                 "dt_camera_rays")
        return ms.value

    def memset():
        for t in (a, b):
            if hip.hipMemsetAsync(ctypes.c_void_p(t.data_ptr()), 0, nbytes, ctypes.c_void_p(stream)):
                sys.exit("hipMemsetAsync failed")

    def h2d(src):
        def f():
            if hasattr(src[0], "is_pinned"):
                a.copy_(src[0], non_blocking=True)
                b.copy_(src[1], non_blocking=True)
            else:
                torch.from_numpy(src[0]).cuda()
                torch.from_numpy(src[1]).cuda()
        return f

    runs = {"camera_rays": camera, "memset": events(memset), "h2d_pageable": events(h2d(host)),
            "h2d_pinned": events(h2d(pinned)),
            "resolve": events(lambda: dt.rays_resolve(g, dir, ns, shape=shape, out=plane, stream=stream)),
            "resolve_noshape": events(lambda: dt.rays_resolve(g, dir, ns, out=plane, stream=stream))}
    for f in runs.values():   # warm-up
        f()
    ms = {name: [] for name in runs}
    for _ in range(args.reps):   # alternating
        for name, f in runs.items():
            ms[name].append(f())
    same = bool(torch.equal(a, start) and torch.equal(b, dir))
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {"bench": "camera_rays_c3", "rows": rows, "samples": ns, "reps": args.reps, "bytes_per_array": nbytes,
           "ms": {name: {"min": round(min(v), 4), "median": round(med[name], 4), "max": round(max(v), 4)}
                  for name, v in ms.items()},
           "gb_per_s": {"camera_rays": round(2 * nbytes / med["camera_rays"] / 1e6, 1),
                        "memset": round(2 * nbytes / med["memset"] / 1e6, 1),
                        "resolve": round((nbytes + rows * 4 + plane.numel() * 4) / med["resolve"] / 1e6, 1)},
           "camera_rays_over_memset": round(med["camera_rays"] / med["memset"], 3), "rays_reproduced": same}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
