"""oracle.c's rayColor and generateBVH against the REFERENCE's own, ray by ray.

tests/golden/shade_ref.npz (tools/gen_golden_shade.py) holds, per scene class of tests/scene_gen.py
SHADE_SCENES, the project's primary rays and what the reference's rayColor (render_final_project.cpp and
helpers.h, compiled unmodified against oracle/ref/eigen_shim under the float-libm rule of DESIGN.md §5)
answered for each: colour as unclamped doubles, hit, in_motion; and the tree its generateBVH built.

  or_sample_color   double bit patterns, hit equal (in_motion is NOT pinned: or_sample_color does not report
                    it and no scene here moves; the reference's flag is only checked to be clear). Doubles that differ must agree to a relative 1e-12
                    (pow(x, 5) by multiplication, §5: <= 8 roundings, a thousand times that bound and 2^-16
                    of a float ulp); the count of non-identical vectors is printed.
  or_render         the f32 image against clamp((float)ref) * 255, assert_parity's 1e-4; for the averaged
                    class the per-sample colours are summed in renderImage's order first.
  or_bvh, dt_bvh_build   node for node, index for index, bounds by bit pattern.

`skip` vectors (the reference's undefined read of `inside`, Q5) are stored and left out; only the glass
class may have any. Classes with the same camera share one stored ray set (`<class>.rays`). Reads the fixture
only; the live variant regenerates one class where oracle/_ref/libref_shade_cr.so exists."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
import oracle
import scene_gen as sg
from distraytracer_amd import work as W
from oracle import geom as G
from oracle import shade as S
from parity_check import assert_parity

_gold = np.load(S.GOLD)
CLASSES = [str(c) for c in _gold["classes"]]
REL = 1e-12


def _rays(name):
    key = str(_gold[name + ".rays"])
    return _gold[key + ".start"], _gold[key + ".dir"]


def _scene(name):
    tex = str(_gold[name + ".texture"])
    desc, keep = S.desc_from_records(_gold[name + ".shapes"], _gold[name + ".lights"], tex or None)
    return desc, G.globals_from_record(_gold[name + ".globals"]), keep


@pytest.fixture(scope="module")
def answers():
    """or_sample_color over every stored vector, once per class"""
    cache = {}

    def get(name):
        if name not in cache:
            desc, g, keep = _scene(name)
            col, hit = S.oracle_colors(desc, g)
            col.setflags(write=False)
            cache[name] = (desc, g, keep, col, hit)
        return cache[name]
    return get


@pytest.mark.parametrize("name", CLASSES)
def test_stored_rays_are_the_projects(name):
    """the rays the reference answered are or_primary_ray's for the stored globals, bit for bit"""
    g = G.globals_from_record(_gold[name + ".globals"])
    start, d = S.primary_rays(g)
    want_start, want_d = _rays(name)
    assert start.shape == want_start.shape == want_d.shape == _gold[name + ".color"].shape
    assert not G.differs(start.reshape(-1, 3), want_start.reshape(-1, 3)).any()
    assert not G.differs(d.reshape(-1, 3), want_d.reshape(-1, 3)).any()


@pytest.mark.parametrize("name", CLASSES)
def test_sample_color_against_reference(name, answers):
    _, g, _, col, hit = answers(name)
    want, want_hit, skip = _gold[name + ".color"], _gold[name + ".hit"], _gold[name + ".skip"] != 0
    assert not _gold[name + ".threw"].any()
    # no shape of these scenes is in motion: the oracle re-traces such a sample (out of scope), the
    # reference's flag must be clear
    assert not _gold[name + ".in_motion"].any() and not (_gold[name + ".shapes"]["flags"] & 2).any()
    keep = ~skip
    bits = G.differs(col.reshape(-1, 3), want.reshape(-1, 3)).reshape(keep.shape) & keep
    with np.errstate(all="ignore"):
        close = ((np.isnan(col) == np.isnan(want)) &
                 (np.isnan(want) | (np.abs(col - want) <= REL * np.maximum(np.abs(col), np.abs(want))))).all(axis=-1)
    bad = keep & (~close | (hit != want_hit))
    print("%s: %d vectors, %d skipped, %d not bit-identical, largest relative difference %.3g, NaN vectors %d" % (
        name, keep.size, int(skip.sum()), int(bits.sum()), S.rel_diff(col[keep], want[keep]),
        int(np.isnan(want).any(axis=-1).sum())))
    assert skip.sum() <= 0.02 * skip.size and (name == "glass" or not skip.any())
    p, i = (np.argwhere(bad)[0] if bad.any() else (0, 0))
    assert not bad.any(), "%d vectors differ; pixel %d sample %d start %s dir %s: reference %s hit %d, oracle %s hit %d" % (
        int(bad.sum()), p, i, _rays(name)[0][p, i].tolist(), _rays(name)[1][p, i].tolist(),
        want[p, i].tolist(), want_hit[p, i], col[p, i].tolist(), hit[p, i])


def test_classes_cover_their_paths():
    """what each class is there for shows in the reference's own answers"""
    nan = lambda n: np.isnan(_gold[n + ".color"]).any(axis=-1)
    assert nan("glass").sum() >= 4 and not any(nan(c).any() for c in CLASSES if c != "glass")    # Q25
    for c in CLASSES:
        h = _gold[c + ".hit"]
        assert h.any() and not h.all(), c                     # hits and misses
        col = _gold[c + ".color"]
        with np.errstate(invalid="ignore"):
            assert ((col > 1) | (col < 0)).mean() < 0.05, c   # few channels clamp
            black = (col == 0).all(axis=-1) & (h != 0)
        if c in ("phong", "oren-nayar", "cook-torrance", "raw"):
            assert black.any(), c                             # lit by no light: hits == 0
    assert len(_gold["wave5-phong.hit"].reshape(-1)) == 2048 and _gold["averaged.color"].shape == (128, 4, 3)
    # own-shape: every hit pixel is lit by the one light once its own rectangle is skipped (never black)
    col, h = _gold["own-shape.color"], _gold["own-shape.hit"]
    assert h.sum() > 200 and not ((col == 0).all(axis=-1) & (h != 0)).any()


def _work(name):
    desc, g, keep = _scene(name)
    return oracle.render_work(desc, g, 0, dt.tiles())[2]


def test_classes_reach_their_paths():
    """the events of the reference's loop that each class exists for, counted by the oracle's restatement"""
    ev = lambda w, n: int(w[W.NAMES.index(n)])
    m = _work("mirror")
    assert ev(m, "mirror") > 100 and ev(m, "glossy") == 0            # nogloss = 1: the glossy floor mirrors
    assert ev(_work("glass"), "refract") > 50
    assert ev(_work("emitters"), "emit") >= 16
    assert ev(_work("textured"), "tex") > 200
    w = _work("area")
    assert ev(w, "light") > 400 and ev(w, "light") == 2 * ev(w, "hit")
    w = _work("own-shape")
    assert ev(w, "light") > 200 and ev(w, "light") == ev(w, "hit")
    # textured: texel colours (type 1), the border colour (type 2) and the hole (type 0: the sample returns)
    desc, g, keep = _scene("textured")
    col, h = _gold["textured.color"], _gold["textured.hit"] != 0
    border = np.array(list(desc.shapes[0].bordercolor)) * 0.6        # the one light's colour, Lambert <= 1
    with np.errstate(all="ignore"):
        ratio = col[h] / border
    on_border = (np.abs(ratio - ratio[:, :1]) < 1e-9).all(axis=-1) & (ratio[:, 0] > 0)
    assert on_border.sum() >= 8 and (h & (col == 0).all(axis=-1)).any() and (~on_border).sum() > 100
    # grazing: rays of one pixel row on both sides of the mirror cut
    desc, g, keep = _scene("grazing")
    start, d = _rays("grazing")
    strip = desc.shapes[2]
    A, B, D = (np.array(list(strip.v[k])) for k in (0, 1, 3))
    n = np.cross(B - A, D - A)
    n /= np.linalg.norm(n)
    row = slice(8 * g.xRes, 9 * g.xRes)
    cos = np.abs(d[row, 0] @ n) / np.linalg.norm(d[row, 0], axis=1)
    t = ((A - start[row, 0]) @ n) / (d[row, 0] @ n)
    z = start[row, 0, 2] + t * d[row, 0, 2]
    assert ((z > 0.5) & (z < 4.5)).all()                              # the whole row meets the strip
    assert (cos > 1.02e-3).sum() >= 8 and (cos < 0.98e-3).sum() >= 8, cos


@pytest.mark.parametrize("name", CLASSES)
def test_render_against_reference_image(name):
    desc, g, keep = _scene(name)
    img, _ = oracle.render(desc, g, 0, dt.tiles())
    ref = S.image_from_colors(g, _gold[name + ".color"])
    ok = S.pixel_mask_to_channels(g, (_gold[name + ".skip"] == 0).all(axis=1))
    assert_parity("shade %s or_render vs reference" % name, img[ok], ref[ok], nan_ok=(name == "glass"))


def _built(fn, desc, g):
    nn, ni = ctypes.c_int32(), ctypes.c_int32()
    dp = ctypes.pointer(desc)
    fn(dp, ctypes.byref(g), None, 0, None, 0, ctypes.byref(nn), ctypes.byref(ni))
    nodes, idx = (dt.BVHNode * max(nn.value, 1))(), (ctypes.c_int32 * max(ni.value, 1))()
    rc = fn(dp, ctypes.byref(g), nodes, nn.value, idx, ni.value, ctypes.byref(nn), ctypes.byref(ni))
    assert rc == 0
    return S.bvh_arrays(list(nodes)[:nn.value], list(idx)[:ni.value])


@pytest.mark.parametrize("name", CLASSES)
@pytest.mark.parametrize("who", ["or_bvh", "dt_bvh_build"])
def test_bvh_against_reference(name, who):
    desc, g, keep = _scene(name)
    if who == "or_bvh":
        nodes, idx = S.bvh_arrays(*oracle.bvh(desc, g))
    else:
        nodes, idx = _built(dt.lib.dt_bvh_build, desc, g)
    want_nodes, want_idx = _gold[name + ".bvh_nodes"], _gold[name + ".bvh_idx"]
    assert len(want_nodes) > 1 and sorted(want_idx.tolist()) == list(range(desc.n_shapes))
    assert S.bvh_differs(nodes, want_nodes) is None, S.bvh_differs(nodes, want_nodes)
    assert idx.tolist() == want_idx.tolist()


@pytest.mark.skipif(not S.RefShade.available(True) or not S.RefShade.available(False),
                    reason="oracle/_ref/libref_shade_cr.so absent (built only where the reference is)")
@pytest.mark.parametrize("name", ["cook-torrance"])
def test_live_reference_reproduces_the_fixture(name):
    out, _, _ = S.answer(name, sg)
    for k, v in out.items():
        if k in ("start", "dir"):
            want = _rays(name)[k == "dir"]
            assert not G.differs(v.reshape(-1, 3), want.reshape(-1, 3)).any(), k
            continue
        want = _gold["%s.%s" % (name, k)]
        if np.asarray(v).dtype.kind == "f":
            assert not G.differs(np.asarray(v).reshape(-1, 1), want.reshape(-1, 1)).any(), k
        else:
            assert np.array_equal(np.asarray(v), want), k
