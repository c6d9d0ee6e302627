"""Generate tests/golden/shade_sampling_ref.npz: the stochastic paths of the REFERENCE's own rayColor (glossy,
rectangle-light and sphere-light sampling, in_motion) on tests/scene_gen.py's SAMPLING_SCENES.

The draw-tape builds (oracle/_ref/libref_shade_tape_cr.so and libref_shade_tape.so, oracle/Makefile: the same
unmodified sources as for shade_ref.npz, with oracle/ref/tape_random.h force-included, so that every
uniform_real_distribution they name hands out a tape) answer each of the project's primary rays with the draws
or_sample_color_log logged for that pixel and sample as the tape. Per class the file holds the shape, light and
globals records, the rays, the colour / hit / in_motion / threw of the cr build, the number of draws it consumed
per vector, and the plain-libm build's colours where they differ. The tape is not stored: the tests regenerate
it from the oracle.

One vector on which or_sample_color_log differs from the cr build (colour beyond 1e-12 relative, hit, in_motion
or the number of draws), one over-asked tape or one throw refuses the write: no class here has a documented
reason to skip. Run where the reference is (make -C oracle ref); the fixture travels, the reference does not.
tests/golden/shade_ref.npz is not touched. Data only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CLASSES = ["rect-light", "sphere-light", "glossy", "glossy-area", "in-motion", "wave5-glossy-area",
           "wave5-glossy-area-mesh"]
LIMIT = 447845   # bytes of tests/golden/shade_ref.npz: this fixture must not be larger


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scene_gen as sg
    from gen_golden_shade import compare, write_npz
    from oracle import geom as G
    from oracle import shade as S
    if not (S.RefShade.available(True, tape=True) and S.RefShade.available(False, tape=True)):
        sys.exit("oracle/_ref/libref_shade_tape_cr.so or libref_shade_tape.so missing: make -C oracle ref")
    report_only = "--report" in sys.argv
    only = [a for a in sys.argv[1:] if not a.startswith("--")]
    store, refuse, ray_sets = {"classes": np.array(CLASSES)}, [], {}
    print("%-24s %7s %9s %7s %10s %5s %5s %11s %9s %7s %12s %8s" % (
        "class", "vectors", "non-ident", "differ", "max rel", "skip", "threw", "draws", "consumed=", "moving",
        "plain image", "clamped"))
    for name in (only or CLASSES):
        out, (desc, g, keep), (ocol, ohit, omot, on, over) = S.answer_sampling(name, sg)
        cmp_ = compare(G, out, ocol, ohit)
        cmp_[(out["in_motion"] != omot) | (out["draws"] != on) | (over != 0)] = 2
        n = cmp_.size
        differ = np.argwhere(cmp_ == 2)
        ok = cmp_ != 2
        ref_img = S.image_from_colors(g, out["color"])
        plain_img = S.image_from_colors(g, S.plain_unpack(out["color"], out["plain_index"], out["plain_color"]))
        with np.errstate(all="ignore"):
            plain_diff = np.nanmax(np.abs(ref_img - plain_img), initial=0.0)
            clamped = float(((out["color"] > 1) | (out["color"] < 0)).mean())
        same = bool((out["draws"] == on).all() and not over.any())
        print("%-24s %7d %9d %7d %10.3g %5d %5d %5d/%-5d %9s %7d %12.3g %7.2f%%" % (
            name, n, int((cmp_ == 1).sum()), len(differ), S.rel_diff(out["color"][ok], ocol[ok]), 0,
            int(out["threw"].sum()), int(out["draws"].min()), int(out["draws"].max()), "yes" if same else "NO",
            int(out["in_motion"].sum()), plain_diff, 100 * clamped))
        for p, i in differ[:12]:
            print("  DIFFERS %s pixel %d sample %d: reference %r hit %d moving %d draws %d over %d, oracle %r hit %d "
                  "moving %d draws %d" % (name, p, i, out["color"][p, i].tolist(), out["hit"][p, i], out["in_motion"][p, i],
                                          out["draws"][p, i], over[p, i], ocol[p, i].tolist(), ohit[p, i], omot[p, i],
                                          on[p, i]))
        if len(differ):
            refuse.append("%s: %d of %d vectors differ from or_sample_color_log" % (name, len(differ), n))
        if out["threw"].any():
            refuse.append("%s: the reference threw on %d vectors" % (name, int(out["threw"].sum())))
        if clamped >= 0.05:
            refuse.append("%s: %.1f %% of the reference's channels clamp" % (name, 100 * clamped))
        out["skip"] = np.zeros_like(out["hit"])
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
        # flags and counts are small numbers: stored narrow, compared as integers
        for k in ("hit", "in_motion", "threw", "skip"):
            out[k] = out[k].astype(np.int8)
        out["draws"] = out["draws"].astype(np.int16)
        for k, v in out.items():
            store["%s.%s" % (name, k)] = v
    if refuse:
        print("\n".join("REFUSED " + r for r in refuse))
    if report_only or only:
        return
    if refuse:
        sys.exit("not written")
    path = os.path.join(ROOT, "tests", "golden", "shade_sampling_ref.npz")
    write_npz(path, store)
    if os.path.getsize(path) > LIMIT:
        sys.exit("%s is larger than shade_ref.npz's %d bytes: shrink a class" % (path, LIMIT))


if __name__ == "__main__":
    main()
