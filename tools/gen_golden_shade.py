"""Generate tests/golden/shade_ref.npz from the REFERENCE's own rayColor and generateBVH
(render_final_project.cpp and helpers.h, included unmodified by oracle/ref/shade_harness.cpp and compiled
against oracle/ref/eigen_shim into oracle/_ref/libref_shade_cr.so and libref_shade.so, oracle/Makefile).

The scenes are tests/scene_gen.py's SHADE_SCENES and shade_textured; their primary rays are the project's
(or_primary_ray); every answer is the reference's alone. Per class the file holds the shape, light and
globals records, the rays, the colour / hit / in_motion of the build under the float-libm rule of
DESIGN.md §5 (`cr`), the colour of the plain-libm build (the vectors on which it differs), and the BVH as dt_bvh_build exports it.

geom_ref's rule: every vector on which or_sample_color differs from the cr build (beyond 1e-12 relative:
pow(x, 5) by multiplication, §5) is named. In the glass class such a vector rests on the reference's undefined
read of `inside` (Q5): it is stored with skip = 1, and the script refuses to write if they exceed 2 % of the
class. In every other class one differing vector, or one the reference threw on, refuses the write: there is
no documented reason to skip it. Classes with the same camera share one stored ray set (`<class>.rays`). It also refuses if 5 % or more of a class's reference channels clamp. Run where the reference is
(make -C oracle ref); the fixture travels, the reference does not. Data only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ["phong", "oren-nayar", "cook-torrance", "raw", "mirror", "mirror-mesh", "grazing", "glass", "emitters",
           "textured", "area", "own-shape", "wave5-phong", "wave5-cook-torrance", "wave5-oren-nayar",
           "wave5-phong-mesh", "wave5-cook-torrance-mesh", "averaged"]
SKIP_CLASSES = {"glass": "the reference's undefined read of `inside` (Q5)"}   # the only documented reason
REL = 1e-12


def compare(G, out, ocol, ohit):
    """per vector: 0 identical, 1 within REL, 2 differs (colour beyond REL, a NaN on one side, or hit)"""
    col = out["color"]
    bits = G.differs(col.reshape(-1, 3), ocol.reshape(-1, 3)).reshape(col.shape[:-1])
    with np.errstate(all="ignore"):
        nan_same = np.isnan(col) == np.isnan(ocol)
        rel = np.abs(col - ocol) <= REL * np.maximum(np.abs(col), np.abs(ocol))
        close = (nan_same & (rel | np.isnan(col))).all(axis=-1)
    bad = ~close | (out["hit"] != ohit)
    return np.where(bad, 2, np.where(bits, 1, 0)).astype(np.int32)


def write_npz(path, store):
    """a fixed member order and no timestamps: the same answers give the same bytes"""
    import zipfile
    import io
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(store):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(store[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scene_gen as sg
    from oracle import geom as G
    from oracle import shade as S
    if not (S.RefShade.available(True) and S.RefShade.available(False)):
        sys.exit("oracle/_ref/libref_shade_cr.so or libref_shade.so missing: make -C oracle ref")
    report_only = "--report" in sys.argv
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    store, refuse, ray_sets = {"classes": np.array(CLASSES)}, [], {}
    print("%-20s %7s %9s %7s %12s %12s %12s %8s" % ("class", "vectors", "non-ident", "differ", "max rel", "image diff",
                                                 "plain image", "clamped"))
    for name in (only or CLASSES):
        out, (desc, g, keep), (ocol, ohit) = S.answer(name, sg)
        cmp_ = compare(G, out, ocol, ohit)
        n = cmp_.size
        differ = np.argwhere(cmp_ == 2)
        skip = (cmp_ == 2).astype(np.int32)
        ok = cmp_ != 2
        ref_img, or_img = S.image_from_colors(g, out["color"]), S.image_from_colors(g, ocol)
        plain_img = S.image_from_colors(g, S.plain_unpack(out["color"], out["plain_index"], out["plain_color"]))
        keep_px = S.pixel_mask_to_channels(g, ok.all(axis=1))
        with np.errstate(all="ignore"):
            img_diff = np.nanmax(np.abs(ref_img - or_img)[keep_px], initial=0.0)
            plain_diff = np.nanmax(np.abs(ref_img - plain_img), initial=0.0)
            clamped = float(((out["color"] > 1) | (out["color"] < 0)).mean())
        print("%-20s %7d %9d %7d %12.3g %12.3g %12.3g %7.2f%%" % (
            name, n, int((cmp_ == 1).sum()), len(differ), S.rel_diff(out["color"][ok], ocol[ok]), img_diff, plain_diff,
            100 * clamped))
        for p, i in differ[:12]:
            print("  DIFFERS %s pixel %d sample %d: reference %r hit %d, oracle %r hit %d" % (
                name, p, i, out["color"][p, i].tolist(), out["hit"][p, i], ocol[p, i].tolist(), ohit[p, i]))
        if out["threw"].any():
            print("  the reference threw on %d vectors" % int(out["threw"].sum()))
            skip |= out["threw"]
        if len(differ) > (0.02 * n if name in SKIP_CLASSES else 0):
            refuse.append("%s: %d of %d vectors differ from or_sample_color" % (name, len(differ), n))
        if out["threw"].any():
            refuse.append("%s: the reference threw" % name)
        if clamped >= 0.05:
            refuse.append("%s: %.1f %% of the reference's channels clamp" % (name, 100 * clamped))
        out["skip"] = skip
        out["skip_reason"] = np.array(SKIP_CLASSES.get(name, ""))
        # classes with one camera share their rays: a ray set is stored once, each class names its own
        rays = (out.pop("start"), out.pop("dir"))
        for key in ray_sets:
            if all(a.shape == b.shape and not G.differs(a.reshape(-1, 3), b.reshape(-1, 3)).any()
                   for a, b in zip(ray_sets[key], rays)):
                break
        else:
            key = "rays%d" % len(ray_sets)
            ray_sets[key] = rays
            store[key + ".start"], store[key + ".dir"] = rays
        out["rays"] = np.array(key)
        for k, v in out.items():
            store["%s.%s" % (name, k)] = v
    if refuse:
        print("\n".join("REFUSED " + r for r in refuse))
    if report_only or only:
        return
    if refuse:
        sys.exit("not written")
    write_npz(os.path.join(ROOT, "tests", "golden", "shade_ref.npz"), store)


if __name__ == "__main__":
    main()
