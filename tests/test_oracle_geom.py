"""oracle.c's restatement of geometry.cpp pinned against the reference's own geometry.cpp: the committed
golden vectors (tests/golden/geom_ref.npz, written by tools/gen_golden_geom.py from geometry.cpp compiled
unmodified against oracle/ref/eigen_shim) are put to the oracle's test-only entry points (or_shape_*,
or_box_intersect, or_fix_norm, ...), which wrap the statics the render loop calls.

Every stored vector is compared: integers (hit, inside, valid, lastHit) as integers, every float and
double by bit pattern; any NaN equals any NaN. geometry.cpp has no transcendental calls on these paths
but pow(x, 2) and one double atan2, so there is no tolerance to choose. What this pins is the reference's
program logic (branches, thresholds, declared types, statement-level operation order); the summation
order inside Eigen's dot() and its handling of a zero vector are assumptions the shim and the oracle
share (DESIGN.md "Oracle")."""
import os

import numpy as np
import pytest

import oracle
from oracle import geom as G

GOLD = os.path.join(os.path.dirname(__file__), "golden", "geom_ref.npz")
FUNCTIONS = ["intersect", "shadow", "cap", "norm", "uv", "box", "fix_norm", "barycentric", "segment"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def orc(gold):
    return G.Oracle(gold["shapes"], gold["holes"])


def _split(gold, fn):
    cases = {k.split(".in.")[1]: gold[k] for k in gold.files if k.startswith(fn + ".in.")}
    want = {k.split(".out.")[1]: gold[k] for k in gold.files if k.startswith(fn + ".out.")}
    return cases, want


def _assert_same(fn, cases, want, got, types, names, who="golden"):
    tv = types[cases["shape"]] if "shape" in cases else None
    for field, idx in G.mismatches(fn, want, got, tv).items():
        n = len(want[field])
        i = idx[0] if len(idx) else None
        assert len(idx) == 0, "%s.%s: %d of %d %s vectors differ; first: vector %d %s reference %r oracle %r inputs %s" % (
            fn, field, len(idx), n, who, i, names[cases["shape"][i]] if tv is not None else "",
            want[field][i], got[field][i], {k: v[i].tolist() for k, v in cases.items()})


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_golden_vectors_bit_exact(gold, orc, fn):
    cases, want = _split(gold, fn)
    n = len(next(iter(want.values())))
    assert n >= 40, "fixture lost its %s vectors" % fn
    # removed vectors are Eigen-convention cases recorded in DESIGN.md: never more than 2 % of a function
    assert len(gold[fn + ".removed"]) <= 0.02 * (n + len(gold[fn + ".removed"]))
    got = G.evaluate(orc, {fn: cases})[fn]
    _assert_same(fn, cases, want, got, gold["shapes"]["type"], gold["shape_names"])


def test_fixture_covers_the_edges(gold):
    """the answers themselves show that the deliberate cases are in the file: every shape type is hit,
    missed and (3-D shapes) entered from inside; an unwritten t occurs; every uv class occurs"""
    cases, want = _split(gold, "intersect")
    types = gold["shapes"]["type"][cases["shape"]]
    for t in range(1, 10):
        m = types == t
        assert want["hit"][m].any() and not want["hit"][m].all(), t
        if t in (1, 2, 8, 9):
            assert want["inside"][m].any(), t
    assert ((cases["ray"] == 0).sum(axis=1) == 1).any() and ((cases["ray"] == 0).sum(axis=1) == 2).any()
    assert ((want["hit"] != 0) & (want["t"] == G.T_INIT)).any()      # Checkerboard edge-on: true, t unwritten
    _, uv = _split(gold, "uv")
    assert set(np.unique(uv["valid"])) == {0, 1, 2}
    _, sh = _split(gold, "shadow")
    assert sh["hit"].any() and not sh["hit"].all()
    _, bx = _split(gold, "box")
    assert bx["hit"].any() and not bx["hit"].all()
    _, nm = _split(gold, "norm")
    assert nm["threw"].any()


def test_per_shape_members(gold, orc):
    """getBounds, the BoundingVolume bounds over one shape (leaf and inner node: same padding) and
    CheckerCylinder::objM (buildCOB times the translation; one cylinder lies along x, where buildCOB takes its
    second basis choice) of every shape record"""
    types = gold["shapes"]["type"]
    got = G.evaluate_shapes(orc, len(types), types)
    for k, v in got.items():
        d = G.differs(gold["per_shape." + k], v)
        assert not d.any(), "%s differs for %s" % (k, list(gold["shape_names"][d]))


def test_fixture_shape_records_carry_the_reference_members(gold):
    """center / length / width of the fixture's shape records are the reference constructors' values
    (derived.*), which is what the oracle reads from a record (length and width in
    CheckerboardWithHole::getUV)"""
    rec = gold["shapes"]
    assert not G.differs(rec["center"], gold["derived.center"]).any()
    quad = np.isin(rec["type"], (4, 5, 6, 7, 9))
    assert not G.differs(rec["length"][quad], gold["derived.lwhr"][quad, 0]).any()
    assert not G.differs(rec["width"][quad], gold["derived.lwhr"][quad, 1]).any()
    # members no constructor sets are stored as 0, never as whatever memory held
    assert not gold["derived.lwhr"][~quad, :2].any() and not gold["derived.axis"][~np.isin(rec["type"], (2, 8))].any()


def test_scene_builder_members_match_reference_constructors(gold):
    """host_scenes.cpp derives center, length and width itself when it fills a dt_shape_desc. For a sample
    of the shapes of the shipped builders (every type they place, rectangle and sphere lights included:
    a rectangleLight keeps Rectangle()'s length = width = 1), the stored values are what the reference's
    constructors compute from the same vertices: same doubles, same floats."""
    import distraytracer_amd as dt
    scenes = list(zip(gold["builder.scene"], gold["builder.frame"], gold["builder.use_model"]))
    seen = 0
    for key in dict.fromkeys(scenes):
        rows = [i for i, k in enumerate(scenes) if k == key]
        built, rec, _, idx = G.builder_sample(dt, str(key[0]), int(key[1]), int(key[2]))
        assert list(idx) == list(gold["builder.index"][rows]), key
        mine = rec[idx]
        assert np.array_equal(mine["type"], gold["builder.type"][rows]), key
        bad = G.differs(mine["center"], gold["builder.center"][rows])
        assert not bad.any(), "%s: center of shapes %s" % (key, list(idx[bad]))
        quad = np.isin(mine["type"], (4, 5, 6, 7, 9))
        want = gold["builder.lwhr"][rows]
        bad = quad & (G.differs(mine["length"], want[:, 0]) | G.differs(mine["width"], want[:, 1]))
        assert not bad.any(), "%s: length / width of shapes %s" % (key, list(idx[bad]))
        seen += len(rows)
    assert seen >= 60 and set(gold["builder.type"]) >= {1, 2, 3, 4, 5, 7, 8, 9}


def test_camera_scenes_oracle(gold):
    """the one-shape camera scenes tests/test_gpu_geom.py runs on the device: the stored rays are still
    the ones or_primary_ray draws, and or_primary_hit (BVH gather over the one leaf + closest hit) gives
    the reference's stored answer for every ray"""
    for k in range(len(gold["cam.shape"])):
        g = G.globals_from_record(gold["cam.globals"][k])
        n = gold["cam.hit"].shape[1]
        start, d = G.or_primary_ray(g, 0, 0, n)
        assert not G.differs(start, gold["cam.start"][k]).any() and not G.differs(d, gold["cam.dir"][k]).any()
        desc, keep = G.one_shape_scene(gold["shapes"][gold["cam.shape"][k]], gold["holes"])
        shape, t = oracle.primary_hit(desc, g, 0, 0, n)
        bad = np.nonzero((shape != gold["cam.hit"][k]) | G.differs(t, gold["cam.t"][k]))[0]
        name = gold["shape_names"][gold["cam.shape"][k]]
        assert len(bad) == 0, "scene %d (%s) ray %d: reference (%d, %r) oracle (%d, %r)" % (
            k, name, bad[0], gold["cam.hit"][k][bad[0]], gold["cam.t"][k][bad[0]], shape[bad[0]], t[bad[0]])
        assert 0 < (gold["cam.hit"][k] >= 0).sum(), name
    kinds = gold["shapes"]["type"][gold["cam.shape"]]
    assert set(kinds) == set(range(1, 10))
    aperture = np.array([r["aperture"] for r in gold["cam.globals"]])
    assert (aperture == 0).any() and (aperture > 0).any()


def test_against_reference_build_if_present(gold):
    """The same comparison on freshly drawn vectors (another seed), answered by the reference build
    itself; also: the committed fixture's answers are still what that build gives."""
    if not G.Ref.available():
        pytest.skip("oracle/_ref/libref_geom.so not built (needs the reference)")
    names, shapes, holes = G.make_shapes()
    hole_rec = G.records_from_shapes(holes)
    G.derive_fields(G.Ref(G.records_from_shapes(shapes), hole_rec), shapes)
    shape_rec = G.records_from_shapes(shapes)
    ref, orc = G.Ref(shape_rec, hole_rec), G.Oracle(shape_rec, hole_rec)
    cases = G.draw(ref, shapes, holes, seed=987654321, n_random=24, n_bisect=6)
    want, got = G.evaluate(ref, cases), G.evaluate(orc, cases)
    for fn in FUNCTIONS:
        _assert_same(fn, cases[fn], want[fn], got[fn], shape_rec["type"], np.array(names), "fresh")
    ref_gold = G.Ref(gold["shapes"], gold["holes"])
    for fn in FUNCTIONS:
        c, w = _split(gold, fn)
        again = G.evaluate(ref_gold, {fn: c})[fn]
        for field in w:
            assert not G.differs(w[field], again[field]).any(), (fn, field)
