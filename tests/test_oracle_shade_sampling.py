"""oracle.c's glossy, rectangle-light and sphere-light sampling and its in_motion against the REFERENCE's own
rayColor, ray by ray and draw by draw.

tests/golden/shade_sampling_ref.npz (tools/gen_golden_shade_sampling.py) holds, per class of tests/scene_gen.py
SAMPLING_SCENES, the project's primary rays and what the draw-tape build of the reference answered for each
when its uniform_real_distribution handed out the draws or_sample_color_log logged for that pixel and sample
(oracle/ref/tape_random.h; the float-libm rule of DESIGN.md §5): colour as unclamped doubles, hit, in_motion,
threw, and the number of draws it consumed. The tape is not stored: it is the oracle's log, regenerated here.

  or_sample_color_log   colour by double bit pattern or to a relative 1e-12 (the bound of test_oracle_shade.py;
                        the count of non-identical vectors is printed), hit and in_motion equal, the log's
                        length equal to the number of draws the reference consumed. A restatement that draws
                        in another order or another number of times than the reference fails the count even
                        where the fixture's colours were made from its own tape.
  or_sample_color       the same colour and hit without a log (the log changes nothing).
  or_render             the f32 image against clamp((float)ref) * 255, assert_parity's 1e-4.

No class has skipped vectors or throws. Reads the fixture only; the live variant feeds the tape build the
oracle's logs again where oracle/_ref/libref_shade_tape_cr.so exists."""
import numpy as np
import pytest

import distraytracer_amd as dt
import oracle
import scene_gen as sg
from distraytracer_amd import work as W
from oracle import geom as G
from oracle import shade as S
from parity_check import assert_parity

_gold = np.load(S.GOLD_SAMPLING)
CLASSES = [str(c) for c in _gold["classes"]]
REL = 1e-12


def _rays(name):
    key = str(_gold[name + ".rays"])
    return _gold[key + ".start"], _gold[key + ".dir"]


def _scene(name):
    desc, keep = S.desc_from_records(_gold[name + ".shapes"], _gold[name + ".lights"], None)
    return desc, G.globals_from_record(_gold[name + ".globals"]), keep


@pytest.fixture(scope="module")
def answers():
    """or_sample_color_log over every stored vector, once per class"""
    cache = {}

    def get(name):
        if name not in cache:
            desc, g, keep = _scene(name)
            col, hit, mot, draws = S.oracle_logs(desc, g)
            col.setflags(write=False)
            cache[name] = (desc, g, keep, col, hit, mot, draws)
        return cache[name]
    return get


def test_fixture_is_no_larger_than_the_deterministic_one():
    import os
    assert os.path.getsize(S.GOLD_SAMPLING) <= 447845
    assert set(CLASSES) == set(sg.SAMPLING_SCENES)


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
    desc, g, _, col, hit, mot, draws = answers(name)
    want, want_hit, want_mot = _gold[name + ".color"], _gold[name + ".hit"], _gold[name + ".in_motion"]
    want_n, n = _gold[name + ".draws"], S.draw_counts(draws)
    assert not _gold[name + ".threw"].any() and not _gold[name + ".skip"].any()
    assert g.blur_samples == 0          # the colour is the primary rayColor call's alone
    bits = G.differs(col.reshape(-1, 3), want.reshape(-1, 3)).reshape(hit.shape)
    with np.errstate(all="ignore"):
        close = ((np.isnan(col) == np.isnan(want)) &
                 (np.isnan(want) | (np.abs(col - want) <= REL * np.maximum(np.abs(col), np.abs(want))))).all(axis=-1)
    bad = ~close | (hit != want_hit) | (mot != want_mot) | (n != want_n)
    print("%s: %d vectors, %d not bit-identical, largest relative difference %.3g, in_motion differs on %d, draw "
          "count differs on %d, draws per vector %d..%d, %d vectors in motion" % (
              name, bits.size, int(bits.sum()), S.rel_diff(col, want), int((mot != want_mot).sum()),
              int((n != want_n).sum()), int(want_n.min()), int(want_n.max()), int(want_mot.sum())))
    p, i = (np.argwhere(bad)[0] if bad.any() else (0, 0))
    assert not bad.any(), ("%d vectors differ; pixel %d sample %d start %s dir %s: reference %s hit %d in_motion %d draws %d, "
                           "oracle %s hit %d in_motion %d draws %d" % (
                               int(bad.sum()), p, i, _rays(name)[0][p, i].tolist(), _rays(name)[1][p, i].tolist(),
                               want[p, i].tolist(), want_hit[p, i], want_mot[p, i], want_n[p, i], col[p, i].tolist(),
                               hit[p, i], mot[p, i], n[p, i]))


@pytest.mark.parametrize("name", ["rect-light", "in-motion"])
def test_the_log_changes_nothing(name, answers):
    """or_sample_color (no log) and or_sample_color_log give the same bits"""
    desc, g, _, col, hit, _, _ = answers(name)
    plain_col, plain_hit = S.oracle_colors(desc, g)
    assert not G.differs(col.reshape(-1, 3), plain_col.reshape(-1, 3)).any() and np.array_equal(hit, plain_hit)


def test_classes_cover_their_paths():
    """what each class is there for shows in the reference's own answers"""
    for c in CLASSES:
        h, col = _gold[c + ".hit"], _gold[c + ".color"]
        assert h.any() and not h.all(), c                     # hits and misses
        assert not np.isnan(col).any(), c
        assert ((col > 1) | (col < 0)).mean() < 0.05, c       # few channels clamp
        assert _gold[c + ".draws"].max() >= 4, c
        assert (_gold[c + ".in_motion"] != 0).any() == (c == "in-motion"), c
    assert _gold["wave5-glossy-area.hit"].size == _gold["wave5-glossy-area-mesh.hit"].size == 2048
    # rect-light: red comes from light 0 alone. A floor pixel under the plate's edge has samples with and
    # without it (penumbra), others have it in every sample (lit) or in none (umbra)
    col, h = _gold["rect-light.color"], _gold["rect-light.hit"] != 0
    red = col[..., 0] > 0
    floor = h.all(axis=1) & (col[..., 2] > 0).all(axis=1)    # the point lights (blue) reach every open floor sample
    lit, umbra = floor & red.all(axis=1), floor & ~red.any(axis=1)
    penumbra = floor & red.any(axis=1) & ~red.all(axis=1)
    assert lit.sum() >= 8 and umbra.sum() >= 4 and penumbra.sum() >= 4, (lit.sum(), umbra.sum(), penumbra.sum())
    # two samples of a lit pixel differ: the sampled point of the light moves with the draw
    assert (np.ptp(col[lit][..., 0], axis=1) > 0).all()
    # sphere-light: the own-shape light (green alone) lights floor points near the origin
    col = _gold["sphere-light.color"]
    assert (col[..., 1] > 0).sum() >= 20 and (col[..., 0] > 0).sum() >= 100 and (col[..., 2] > 0).sum() >= 100


def _work(name):
    desc, g, keep = _scene(name)
    return oracle.render_work(desc, g, 0, dt.tiles())[2]


def _primary_shape(desc, g):
    """the shape the primary ray of [pixel, sample] hits (or_primary_hit), -1 for none"""
    n = g.xRes * g.yRes * max(8, -(-S.spp(g) // 8) * 8)
    return oracle.primary_hit(desc, g, 0, 0, n)[0][S.ray_index(g)]


def test_classes_reach_their_paths(answers):
    """the events of the reference's loop that each class exists for: the oracle's counters, its draw logs and
    the stored fields"""
    ev = lambda w, n: int(w[W.NAMES.index(n)])
    # rect-light: 5 lights per hit, no reflection; 3 of them draw (2 values each)
    w = _work("rect-light")
    assert ev(w, "light") == 5 * ev(w, "hit") > 1000 and ev(w, "glossy") == ev(w, "mirror") == 0
    n = _gold["rect-light.draws"]
    assert set(np.unique(n)) == {0, 6} and (n == 6).sum() == ev(w, "hit")
    # sphere-light: 3 lights, at least 2 values each; more where the baxis light drew again (attempt >= 1)
    w = _work("sphere-light")
    n, h = _gold["sphere-light.draws"], _gold["sphere-light.hit"] != 0
    assert ev(w, "light") > 900 and ev(w, "glossy") == 0
    assert (n[n > 0] >= 6).all() and (n % 2 == 0).all()
    redrawn = (n > 6).sum() / max((n > 0).sum(), 1)
    print("sphere-light: %.1f %% of the lit vectors drew again for the baxis light" % (100 * redrawn))
    assert 0.1 < redrawn < 0.9
    # ... and the light without baxis took the mirror image: its draw (the first two values of the log)
    # faces away from the floor point for about half of the floor's vectors
    desc, g, keep, _, _, _, draws = answers("sphere-light")
    start, d = _rays("sphere-light")
    shape = _primary_shape(desc, g)
    C, away, seen = np.array(list(desc.lights[0].center)), 0, 0
    for p, i in np.argwhere(shape == 0):
        P = start[p, i] - start[p, i, 1] / d[p, i, 1] * d[p, i]          # the floor is y = 0
        u0, u1 = draws[p][i][:2]
        phi, th = np.arccos(1 - 2 * u1), 2 * np.pi * u0
        t = np.array([np.sin(phi) * np.cos(th), np.sin(phi) * np.sin(th), np.cos(phi)])
        seen += 1
        away += (t @ (P - C)) < -1e-6
    assert seen > 100 and 0.3 < away / seen < 0.7, (away, seen)
    # glossy: brdf_samples samples per glossy hit, and resamples (each rebuilds the rectangle)
    desc, g, keep = _scene("glossy")
    w = _work("glossy")
    b = g.brdf_samples
    first = (ev(w, "glossy") - ev(w, "glossy_rect")) // (b - 1)          # glossy = b first + r, rects = first + r
    resampled = ev(w, "glossy_rect") - first
    print("glossy: %d sample rectangles, %d resamples" % (first, resampled))
    assert first > 300 and resampled >= 8 and ev(w, "mirror") == 0
    # ... the ray of pixel (W/2, H/2) is exactly along -x and meets the x-normal wall: the isApprox fallback
    start, d = _rays("glossy")
    centre = (g.yRes // 2) * g.xRes + g.xRes // 2
    assert (d[centre, :, 1] == 0).all() and (d[centre, :, 2] == 0).all() and (d[centre, :, 0] < 0).all()
    assert (_primary_shape(desc, g)[centre] == 1).all() and desc.shapes[1].v[0][0] == desc.shapes[1].v[2][0] == -4.0
    assert (_gold["glossy.draws"][centre] >= 2 * b).all()
    # ... grazing views: floor hits whose reflected ray rises by less than the sample rectangle's half width
    # (0.25 at twice the unit reflection), so a vertex starts below the floor and the squeeze loops move it
    fl = _primary_shape(desc, g) == 0
    rise = 2 * np.abs(d[..., 1]) / np.linalg.norm(d, axis=-1)
    assert (fl & (rise < 0.125)).sum() >= 16 and (fl & (rise > 0.6)).sum() >= 40
    # glossy-area: glossy children under rectangle lights, two levels of glossy recursion
    for c in ("glossy-area", "wave5-glossy-area", "wave5-glossy-area-mesh"):
        desc, g, keep = _scene(c)
        w = _work(c)
        assert ev(w, "glossy") >= 2 * ev(w, "glossy_rect") > 0 and ev(w, "light") == 2 * (ev(w, "hit") - ev(w, "emit"))
        # a first-level glossy hit alone draws 2 b + 4 values (its samples and two lights), each child 4: more
        # than 2 b + 4 + 4 b values means a child was glossy too
        assert (_gold[c + ".draws"] > 6 * g.brdf_samples + 4).sum() >= 10, c
    # in-motion: the four ways the flag comes about
    desc, g, keep = _scene("in-motion")
    shape, mot = _primary_shape(desc, g), _gold["in-motion.in_motion"] != 0
    moving = [(desc.shapes[i].flags & sg.F_MOTION) != 0 for i in range(desc.n_shapes)]
    assert moving == [False, False, False, True, True, False]
    assert mot[shape == 3].all() and (shape == 3).sum() >= 8                  # seen directly
    assert mot[shape == 2].any() and not mot[shape == 2].all()                # the static mirror shows it, or not
    assert (shape == 4).sum() >= 8 and (~mot[shape == 4]).sum() >= 6          # the moving mirror shows static shapes
    assert mot[shape == 0].any() and not mot[shape == 0].all()                # the glossy floor's last sample decides
    assert not mot[shape == 1].any() and not mot[shape == 5].any() and not mot[shape < 0].any()
    assert ev(_work("in-motion"), "mirror") > 50


@pytest.mark.parametrize("name", CLASSES)
def test_render_against_reference_image(name):
    desc, g, keep = _scene(name)
    img, _ = oracle.render(desc, g, 0, dt.tiles())
    ref = S.image_from_colors(g, _gold[name + ".color"])
    assert_parity("shade sampling %s or_render vs reference" % name, img, ref)


@pytest.mark.skipif(not S.RefShade.available(True, tape=True) or not S.RefShade.available(False, tape=True),
                    reason="oracle/_ref/libref_shade_tape_cr.so absent (built only where the reference is)")
@pytest.mark.parametrize("name", ["sphere-light", "glossy", "glossy-area"])
def test_live_reference_reproduces_the_fixture(name):
    """the tape build, fed the oracle's logs now, gives the stored answers; it never asks past a tape's end"""
    out, _, (_, _, _, n, over) = S.answer_sampling(name, sg)
    assert not over.any() and np.array_equal(n, out["draws"])
    for k, v in out.items():
        if k in ("start", "dir"):
            want = _rays(name)[k == "dir"]
            assert not G.differs(v.reshape(-1, 3), want.reshape(-1, 3)).any(), k
            continue
        want = _gold["%s.%s" % (name, k)]
        assert np.asarray(v).shape == want.shape, k
        if np.asarray(v).dtype.kind == "f" and np.asarray(v).size:
            assert not G.differs(np.asarray(v).reshape(-1, 1), want.reshape(-1, 1)).any(), k
        else:
            assert np.array_equal(np.asarray(v), want), k
