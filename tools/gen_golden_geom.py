"""Generate tests/golden/geom_ref.npz from the REFERENCE's own geometry.cpp (compiled unmodified against
oracle/ref/eigen_shim by oracle/Makefile into oracle/_ref/libref_geom.so). The vectors are drawn seeded,
with the edge cases placed per class (oracle/geom.py draw): start inside / on the surface / behind,
unnormalized rays, exactly-zero components, rays parallel to a cylinder axis or in a polygon's plane,
grazing discriminants, edge and vertex hits, cap against body, t_max one float ulp either side of the
hit, checker square and border boundaries, the RectPrismV2 getNorm fallback, prism holes through the cap
plane -- and every threshold found by bisection between two rays the reference answers differently.
A second group: one-shape camera scenes whose primary rays come from the project (or_primary_ray) and
whose answers (leaf box test, then the shape's intersect) come from the reference alone.

The file holds data only: shape records (constructor-derived members as the reference computed them),
rays, points, answers. Run where the reference is (make -C oracle ref); the fixture travels, the
reference does not. Vectors on which oracle.c and the reference differ are named; the script refuses to
write if they exceed 2 % of any one function's vectors (DESIGN.md "Oracle": such a vector is either an
oracle bug to fix or an Eigen-convention case to record, never silently dropped)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20240611
W, H = 32, 16           # x 8 samples per pixel: the 4096 primary rays of one dt_intersect_primary launch
N_RAYS = W * H * 8

# shape, eye, lookingAt, fov, default aperture?, on the device? (dt_intersect_primary refuses a
# RectPrismWithCylinder scene: that one is answered by the oracle only)
SCENES = [
    ("sphere", (0, 0, 0), (0.5, -0.25, -3), 50, 0, 1),
    ("sphere", (0.7, -0.15, -2.7), (0.5, 0.5, -6), 70, 1, 1),                 # the eye inside the sphere
    ("sphere_small", (0.2, 0.1, 0), (-0.731, 0.412, -2.377), 25, 0, 1),
    ("cylinder_y", (0, 0, 0), (0, 0, -4), 40, 0, 1),                          # centre column / row: zero components
    ("cylinder_oblique", (0.3, 0.4, 0.5), (0.15, 0.55, -4.25), 40, 0, 1),
    ("triangle", (0, 0, 0), (0, 0, -3), 50, 0, 1),
    ("triangle_mesh_uv", (0.5, 0.2, 0.4), (0, 0, -3.2), 45, 0, 1),
    ("rectangle", (0, 0, 0), (0, 0, -4), 40, 0, 1),
    ("rectangle_oblique", (-0.4, 0.3, 0), (0.3, 0.1, -4.2), 40, 1, 1),
    ("prism", (0, 0, 0), (0, 0, -4), 50, 0, 1),
    ("prism", (0.1, 0.2, -4.1), (0.5, 0.3, -8), 80, 0, 1),                    # the eye inside the prism
    ("prism_oblique", (1.5, 1.0, 0), (0, 0.05, -3.9), 35, 0, 1),
    ("checkerboard", (0, 0.5, -1), (0, -1, -4), 60, 0, 1),
    ("checkerboard_hole", (0.3, 1.0, -1.5), (0.1, -1, -4), 60, 0, 1),
    ("checker_cylinder_y", (1, 0.3, -1), (0, 0, -4), 35, 0, 1),
    ("checker_cylinder_oblique", (0, 0, 0), (0.15, 0.55, -4.25), 40, 0, 1),
    ("checker_cylinder_x", (0, 0, 0), (0, 0.5, -4), 40, 0, 1),
    # from the side: seen from the front, the cap plane of a hole (no radius test, geometry.cpp:297-324)
    # lies before the whole box and every ray misses (geometry.cpp:1640-1643)
    ("prism_cyl", (5, 0.8, -4.4), (0, 0, -4.5), 40, 0, 0),
]


def camera_scenes(G, dt, ref, names):
    recs, shape_idx, on_dev, starts, dirs, hit, ts, box = [], [], [], [], [], [], [], []
    for name, eye, look, fov, ap, dev in SCENES:
        si = names.index(name)
        g = dt.globals_default()
        g.xRes, g.yRes, g.fov = W, H, fov
        if not ap:
            g.aperture = 0.0
        for a in range(3):
            g.eye[a], g.lookingAt[a] = eye[a], look[a]
        start, d = G.or_primary_ray(g, 0, 0, N_RAYS)
        with np.errstate(divide="ignore"):
            inv = 1.0 / d
        bh = np.array([ref.box(si, 1, r, iv, s)[0] for r, iv, s in zip(d, inv, start)], dtype=np.int32)
        ans = [ref.intersect(si, r, s) for r, s in zip(d, start)]
        sh = np.array([a[0] for a in ans], dtype=np.int32)
        t = np.array([a[1] for a in ans], dtype=np.float32)
        # rayColor's closest hit over the gathered leaf (cpp:491-538): t_dist < t_min = FLT_MAX
        ok = (bh != 0) & (sh != 0) & (t < G.FLT_MAX)
        recs.append(G.record_from_globals(g))
        shape_idx.append(si)
        on_dev.append(dev)
        starts.append(start)
        dirs.append(d)
        box.append(bh)
        hit.append(np.where(ok, 0, -1).astype(np.int32))
        ts.append(np.where(ok, t, G.FLT_MAX).astype(np.float32))
        print("scene %-26s box hits %4d  shape hits %4d  misses %4d%s" % (
            name, int(bh.sum()), int(ok.sum()), int((~ok).sum()), "" if dev else "  (oracle only)"))
    globals_rec = np.zeros(len(recs), dtype=G.GLOBALS_DT)   # zeroed first: the struct's padding is not data
    for i, r in enumerate(recs):
        globals_rec[i] = r
    return {"cam.globals": globals_rec, "cam.shape": np.array(shape_idx, dtype=np.int32),
            "cam.on_device": np.array(on_dev, dtype=np.int32), "cam.start": np.array(starts),
            "cam.dir": np.array(dirs), "cam.box_hit": np.array(box), "cam.hit": np.array(hit),
            "cam.t": np.array(ts)}


def builder_members(G, dt):
    """center / length / width the reference's constructors derive for shapes the project's scene builders
    made (host_scenes.cpp derives them itself): tests compare the builders' values with these"""
    out = {"builder.scene": [], "builder.frame": [], "builder.use_model": [], "builder.index": [],
           "builder.type": [], "builder.center": [], "builder.lwhr": []}
    for scene, frame, use_model in G.BUILDER_SCENES:
        built, rec, hrec, idx = G.builder_sample(dt, scene, frame, use_model)
        ref = G.Ref(rec, hrec)
        for i in idx:
            c, _, f, _ = ref.derived(int(i))
            for k, v in zip(out, (scene, frame, use_model, i, rec["type"][i], c, f)):
                out[k].append(v)
        print("builder %-9s frame %4d models %d: %4d shapes, %3d sampled" % (scene, frame, use_model, len(rec), len(idx)))
    return {k: np.array(v) for k, v in out.items()}


def main():
    import distraytracer_amd as dt
    from oracle import geom as G
    if not G.Ref.available():
        sys.exit("oracle/_ref/libref_geom.so missing: make -C oracle ref")
    report_only = "--report" in sys.argv
    names, shapes, holes = G.make_shapes()
    hole_rec = G.records_from_shapes(holes)
    G.derive_fields(G.Ref(G.records_from_shapes(shapes), hole_rec), shapes)
    shape_rec = G.records_from_shapes(shapes)
    ref, orc = G.Ref(shape_rec, hole_rec), G.Oracle(shape_rec, hole_rec)
    types = shape_rec["type"]

    cases = G.draw(ref, shapes, holes, SEED, n_random=16, n_bisect=6)
    want = G.evaluate(ref, cases)
    got = G.evaluate(orc, cases)
    out = {"shape_names": np.array(names), "shapes": shape_rec, "holes": hole_rec}
    for si, name in enumerate(names):
        m = cases["intersect"]["shape"] == si
        print("%-26s intersect vectors %4d  hit %4d  inside %3d  t unwritten on a hit %d" % (
            name, int(m.sum()), int(want["intersect"]["hit"][m].sum()), int(want["intersect"]["inside"][m].sum()),
            int(((want["intersect"]["t"][m] == G.T_INIT) & (want["intersect"]["hit"][m] != 0)).sum())))
    too_many = False
    for fn in want:
        n = len(next(iter(want[fn].values())))
        tv = types[cases[fn]["shape"]] if "shape" in cases[fn] else None
        mm = G.mismatches(fn, want[fn], got[fn], tv)
        bad = np.unique(np.concatenate([v for v in mm.values()])) if mm else np.array([], dtype=int)
        for field, idx in mm.items():
            for i in idx:
                who = names[cases[fn]["shape"][i]] if tv is not None else ""
                print("MISMATCH %s.%s vector %d %s: reference %r oracle %r  inputs %s" % (
                    fn, field, i, who, want[fn][field][i], got[fn][field][i],
                    {k: v[i].tolist() for k, v in cases[fn].items() if k != "shape"}))
        print("%-12s %4d vectors, %d differ from oracle.c" % (fn, n, len(bad)))
        if len(bad) > 0.02 * n:
            too_many = True
        keep = np.ones(n, dtype=bool)
        keep[bad] = False
        for k, v in cases[fn].items():
            out["%s.in.%s" % (fn, k)] = v[keep]
        for k, v in want[fn].items():
            out["%s.out.%s" % (fn, k)] = v[keep]
        out["%s.removed" % fn] = bad.astype(np.int32)

    # per shape: getBounds, BoundingVolume bounds, CheckerCylinder objM; the constructor-derived members
    ws, gs = G.evaluate_shapes(ref, len(shapes), types), G.evaluate_shapes(orc, len(shapes), types)
    for k in ws:
        d = G.differs(ws[k], gs[k])
        if d.any():
            print("MISMATCH per-shape %s: %s" % (k, [names[i] for i in np.nonzero(d)[0]]))
            too_many = True
        out["per_shape.%s" % k] = ws[k]
    der = [ref.derived(si) for si in range(len(shapes))]
    out["derived.center"] = np.array([d[0] for d in der])
    out["derived.axis"] = np.array([d[1] for d in der])
    out["derived.lwhr"] = np.array([d[2] for d in der])
    # answers only the reference has (the oracle restates no intersectMax / buildCOB / lineIntersect and
    # drops shortestLine's coefficients): recorded for the day something restates them
    c = cases["intersect"]
    sel = np.nonzero(np.isin(types[c["shape"]], (1, 2)) & (c["tag"] != 6) & (c["tag"] != 7))[0]
    imax = [ref.intersect_max(int(c["shape"][i]), c["ray"][i], c["start"][i]) for i in sel]
    out["intersect_max.in.index"] = sel.astype(np.int32)    # into the drawn (unfiltered) intersect vectors
    out["intersect_max.in.shape"], out["intersect_max.in.ray"] = c["shape"][sel], c["ray"][sel]
    out["intersect_max.in.start"] = c["start"][sel]
    out["intersect_max.out.hit"] = np.array([x[0] for x in imax], dtype=np.int32)
    out["intersect_max.out.t"] = np.array([x[1] for x in imax], dtype=np.float32)
    out["build_cob.in.z"] = cases["build_cob"]["z"]
    out["build_cob.out.m"] = np.array([ref.build_cob(z) for z in cases["build_cob"]["z"]])
    s = cases["segment"]
    sl = [ref.shortest_line(A, B, r + o, o) for A, B, r, o in zip(s["A"], s["B"], s["ray"], s["origin"])]
    out["shortest_line.out.u"] = np.array(sl, dtype=np.float32)
    out["line_intersect.out.hit"] = np.array([ref.line(A, B, r, o) for A, B, r, o in
                                              zip(s["A"], s["B"], s["ray"], s["origin"])], dtype=np.int32)

    out.update(camera_scenes(G, dt, ref, names))
    out.update(builder_members(G, dt))
    if too_many and not report_only:
        sys.exit("more than 2 % of one function's vectors differ between oracle.c and the reference: not written")
    path = os.path.join(ROOT, "tests", "golden", "geom_ref.npz")
    if not report_only:
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
