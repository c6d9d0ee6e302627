"""Object mattes, the host half (include/dt.h dt_render_mattes, dt_matte_mask): the exports, the argument
checks that come before the scene is looked at, dt_matte_mask's host
loop against tests/mattes_ref.py bit for bit, shape_groups, and the restatement itself on oracle ids. No GPU."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
import mattes_ref as R
import oracle
import scene_gen as sg
from distraytracer_amd._lib import EXPORTS, Mattes

INVALID, UNSUPPORTED = -1, -4


def _err():
    return dt.lib.dt_last_error().decode()


N_SHAPES = 7   # a stand-in count: the scene is never looked at in this file


def _globals(aa=64, w=16, h=12):
    g = dt.globals_default()
    g.xRes, g.yRes, g.antialias_samples = w, h, aa
    return g


def _planes(n_px, layers):
    keep = [np.zeros(n_px * layers, np.int32), np.zeros(n_px * layers, np.float32), np.zeros(n_px, np.int32)]
    return Mattes(*[a.ctypes.data for a in keep]), keep


def _call(scene, g, n, gmap, n_shapes, layers, m):
    gp = ctypes.c_void_p(gmap.ctypes.data) if gmap is not None else None
    return dt.lib.dt_render_mattes(scene, ctypes.byref(g) if g is not None else None, 0, None, n, gp, n_shapes, layers,
                                   ctypes.byref(m) if m is not None else None, 0, None, None, None)


def test_exports():
    assert "dt_render_mattes" in EXPORTS and "dt_matte_mask" in EXPORTS
    assert hasattr(dt.lib, "dt_render_mattes") and hasattr(dt.lib, "dt_matte_mask")
    assert dt.lib.dt_abi_version() == 8
    assert ctypes.sizeof(Mattes) == 3 * ctypes.sizeof(ctypes.c_void_p)


def test_render_mattes_refuses_bad_arguments():
    """dt_render_mattes checks scene, globals, out, the planes, n_samples, layers, the sign of n_shapes and the
    map's entries in this order and looks at the scene only after all of them (dt_api.cpp): the scene is a
    stand-in address that is never dereferenced, as in tests/test_features_host.py. The two checks that read
    the scene (its shape count, a RectPrismWithCylinder) need a created scene, which needs a device:
    tests/test_gpu_mattes.py."""
    g = _globals()
    h, n_shapes = ctypes.c_void_p(64), N_SHAPES
    m, keep = _planes(16 * 12, 4)
    cases = [
        ((None, g, 64, None, n_shapes, 4, m), "null scene"),
        ((h, None, 64, None, n_shapes, 4, m), "null globals"),
        ((h, g, 64, None, n_shapes, 4, None), "null out"),
        ((h, g, 64, None, n_shapes, 4, Mattes()), "out wants no plane"),
        ((h, g, 32, None, n_shapes, 4, m), "n_samples"),
        ((h, g, 0, None, n_shapes, 4, m), "n_samples"),
        ((h, g, 128, None, n_shapes, 4, m), "n_samples"),
        ((h, g, 64, None, n_shapes, 0, m), "layers 0"),
        ((h, g, 64, None, n_shapes, 9, m), "layers 9"),
        ((h, g, 64, None, -1, 4, m), "n_shapes -1"),
    ]
    for args, word in cases:
        assert _call(*args) == INVALID, word
        assert _err().startswith("dt_render_mattes: ") and word in _err(), (word, _err())
    bad = np.arange(n_shapes, dtype=np.int32)
    bad[3] = -1
    assert _call(h, g, 64, bad, n_shapes, 4, m) == INVALID
    assert _err().startswith("dt_render_mattes: ") and "group_of_shape[3]" in _err()
    # the window rule's own words survive behind the argument's name
    assert _call(h, g, 32, None, n_shapes, 4, m) == INVALID and "multiple of 64 or spp" in _err()
    assert _call(h, _globals(16), 8, None, n_shapes, 4, m) == INVALID and "the only window is [0,16)" in _err()


class _NoScene:
    handle = None
    _keep = sg.features()[0]


def test_wrapper_checks_planes_and_map():
    g = _globals()
    n1 = 16 * 12
    with pytest.raises(dt.DTError, match="id holds"):
        dt.render_mattes(_NoScene, g, 0, out={"id": np.zeros(n1 * 3, np.int32)})
    with pytest.raises(dt.DTError, match="distinct holds"):
        dt.render_mattes(_NoScene, g, 0, out={"distinct": np.zeros(n1 * 4, np.int32)})
    with pytest.raises(dt.DTError, match="int32"):
        dt.render_mattes(_NoScene, g, 0, out={"id": np.zeros(n1 * 4, np.float32)})
    with pytest.raises(dt.DTError, match="float32"):
        dt.render_mattes(_NoScene, g, 0, out={"weight": np.zeros(n1 * 4, np.int32)})
    with pytest.raises(dt.DTError, match="unknown plane"):
        dt.render_mattes(_NoScene, g, 0, out={"colour": np.zeros(n1, np.float32)})
    with pytest.raises(dt.DTError, match="groups holds 3 entries"):
        dt.render_mattes(_NoScene, g, 0, groups=[0, 1, 2], out={"id": np.zeros(n1 * 4, np.int32)})
    # rightly sized planes reach the library, which refuses the null scene
    with pytest.raises(dt.DTError, match="dt_render_mattes: null scene"):
        dt.render_mattes(_NoScene, g, 0, layers=2, out={"id": np.zeros(n1 * 2, np.int32),
                                                        "distinct": np.zeros(n1, np.int32)})


def _mask(n, layers, ids, w, groups, n_groups, mask):
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    return dt.lib.dt_matte_mask(n, layers, p(ids), p(w), p(groups), n_groups, p(mask), 0, None)


def test_matte_mask_refuses_bad_arguments():
    ids, w, mask = np.zeros(8, np.int32), np.zeros(8, np.float32), np.zeros(2, np.float32)
    gr = np.array([1, 2], np.int32)
    cases = [
        ((2, 4, None, w, gr, 2, mask), "null id"),
        ((2, 4, ids, None, gr, 2, mask), "null weight"),
        ((2, 4, ids, w, None, 2, mask), "null groups"),
        ((2, 4, ids, w, gr, 2, None), "null mask"),
        ((-1, 4, ids, w, gr, 2, mask), "n_pixels"),
        ((2, 0, ids, w, gr, 2, mask), "layers 0"),
        ((2, 9, ids, w, gr, 2, mask), "layers 9"),
        ((2, 4, ids, w, gr, 0, mask), "n_groups 0"),
        ((2, 4, ids, w, np.zeros(65, np.int32), 65, mask), "n_groups 65"),
        ((2, 4, ids, w, np.array([1, -1], np.int32), 2, mask), "groups[1]"),
    ]
    for args, word in cases:
        assert _mask(*args) == INVALID, word
        assert _err().startswith("dt_matte_mask: ") and word in _err(), (word, _err())
    mask[:] = 7
    assert _mask(0, 4, ids, w, gr, 2, mask) == 0 and (mask == 7).all()


@pytest.mark.parametrize("layers", [1, 4, 8])
def test_matte_mask_host_loop_is_the_restatement(layers):
    rng = np.random.default_rng(layers)
    n = 1000
    ids = rng.integers(-1, 6, size=(n, layers)).astype(np.int32)
    w = rng.random((n, layers)).astype(np.float32) * np.float32(1 / 3)
    for groups in ([2], [0, 3, 3, 5, 0], [9], list(range(64))):
        got = dt.matte_mask({"id": ids, "weight": w}, groups)
        want = R.matte_mask(ids, w, groups)
        assert got.shape == (n,) and got.dtype == np.float32
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), groups
    assert (dt.matte_mask({"id": ids, "weight": w}, [9]) == 0).all()
    # -1 never matches, whatever the weights beside it hold
    only = np.full((4, layers), -1, np.int32)
    assert (dt.matte_mask({"id": only, "weight": np.ones((4, layers), np.float32)}, [0, 1]) == 0).all()
    with pytest.raises(dt.DTError, match="groups\\[0\\]"):
        dt.matte_mask({"id": ids, "weight": w}, [-1])


def test_shape_groups():
    desc, g, keep = sg.features()
    ident = dt.shape_groups(desc, "shape")
    assert ident.dtype == np.int32 and ident.tolist() == list(range(desc.n_shapes))
    assert dt.shape_groups(desc, "type").tolist() == [desc.shapes[i].type for i in range(desc.n_shapes)]
    # seven shapes, each a material of its own
    assert dt.shape_groups(desc, "material").tolist() == list(range(desc.n_shapes))
    with pytest.raises(dt.DTError, match="by is"):
        dt.shape_groups(desc, "colour")
    g2 = dt.globals_default()
    built = dt.build_scene("spheres", 0, g2)
    gm = dt.shape_groups(built)
    d = built.desc
    assert gm.dtype == np.int32 and gm.size == d.n_shapes and gm[0] == 0
    # numbered in order of first appearance, and equal signature <=> equal group
    assert sorted(set(gm.tolist())) == list(range(gm.max() + 1))
    firsts = [gm.tolist().index(k) for k in range(gm.max() + 1)]
    assert firsts == sorted(firsts)
    sig = lambda s: (s.type == 3 and bool(s.flags & 32), s.model, s.material, s.emit, s.flags & (1 | 4 | 8 | 32),
                     s.tex_frame, tuple(s.color))
    for i in range(d.n_shapes):
        for j in range(i):
            assert (gm[i] == gm[j]) == (sig(d.shapes[i]) == sig(d.shapes[j])), (i, j)


def test_the_restatement_on_oracle_ids():
    """or_primary_hit ids of the 16x12, 64-spp scene through mattes_ref: the histogram against plain counting,
    and pixels with three groups and more, so that the GPU cases are not vacuous"""
    desc, g, keep = sg.features()
    W, H, n = 16, 12, 64
    g.xRes, g.yRes, g.antialias_samples = W, H, n
    R.defocus(g)
    shape, t = oracle.primary_hit(desc, g, 0, 0, W * H * n)
    ids = R.pixel_ids(shape, W, H, n)
    m = R.mattes(ids, n, 4)
    print("distinct groups per pixel: max %d, pixels with >= 3: %d" % (m["distinct"].max(), (m["distinct"] >= 3).sum()))
    assert (m["distinct"] >= 3).any() and not m["overflow"].any()
    for p in range(W * H):
        vals, counts = np.unique(ids[p][ids[p] >= 0], return_counts=True)
        assert m["distinct"][p] == vals.size
        order = sorted(zip(-counts, vals))[:4]
        assert m["id"][p].tolist() == [int(v) for _, v in order] + [-1] * (4 - len(order))
        assert m["weight"][p].tolist() == [float(-c) / n for c, _ in order] + [0.0] * (4 - len(order))
    # merging every sphere into one group changes some pixel's ranking
    gmap = np.array([0 if desc.shapes[i].type == sg.SPHERE else i + 1 for i in range(desc.n_shapes)], np.int32)
    mm = R.mattes(ids, n, 4, gmap)
    assert (mm["distinct"] <= m["distinct"]).all() and (mm["distinct"] < m["distinct"]).any()
    # the table rule: a tiny table overflows exactly where the pixel holds more groups than entries
    small = R.mattes(ids, n, 2, table=2)
    assert (small["overflow"] == (m["distinct"] > 2)).all() and (small["distinct"] == np.minimum(m["distinct"], 2)).all()
    e, over = R.pixel_table([5, 5, 7, -1, 9, 7, 5, 9, 9, 9], table=2)
    assert e == [[5, 3], [7, 2]] and over
    assert R.rank([[5, 2], [3, 2], [8, 4]]) == [[8, 4], [3, 2], [5, 2]]
