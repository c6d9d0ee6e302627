"""Ray queries (include/dt.h dt_trace_rays, dt_rays_occluded; dt_rayq_kernel, dt_rayq_occl_kernel) against
the prediction of tests/rayquery_ref.py, which tests/test_rayquery_host.py pins to the oracle's own loop.
All comparisons are by bit pattern (oracle.geom.differs); every case first asserts, of its own prediction,
that it holds what it claims to exercise."""
import functools
import os

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
from oracle import geom as G

from rayquery_ref import ATTRS, FLT_MAX, RayQueryRef, void_rays
from test_gpu_features import MIXED_AT, MIXED_EYE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_BENCH = 1 << 24

# (eye, lookingAt) in and around the room of final(240) (x -10..10, y 0.3..10.3, z -5..8): the mixed camera
# of tests/test_gpu_features.py (its lens straddles the wall x = 10: hits and misses), the scene's own
# camera, the skeleton from close by, the checker cylinder, the floor from above, the ceiling lights from
# below, and the room from outside (outer faces and misses)
CAMERAS = [(MIXED_EYE, MIXED_AT), (None, None), ((0.0, 4.0, 6.0), (0.75, 1.0, 0.65)), ((-8.0, 2.0, 6.0), (5.0, 3.0, -4.0)),
           ((5.0, 9.0, 0.0), (0.0, 0.3, 2.0)), ((0.0, 1.0, -3.0), (2.3, 10.25, 3.8)), ((15.0, 5.0, 20.0), (0.0, 5.0, 0.0))]
N_SCATTER = 4096 + 37


def _final(W=1920, H=1080):
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes = W, H
    return g, built


@functools.lru_cache(maxsize=None)
def final_case():
    """final(240) at 1920x1080, its prediction object, and the scattered rays of case 2 with their prediction
    (computed once, shared by the cases that need them, never written to)"""
    g, built = _final()
    ref = RayQueryRef(built, g)
    starts, dirs = [], []
    per = -(-N_SCATTER // len(CAMERAS))
    for eye, at in CAMERAS:
        gc = g.copy()
        gc.xRes, gc.yRes = 40, 24
        if eye is not None:
            for a in range(3):
                gc.eye[a], gc.lookingAt[a] = eye[a], at[a]
        s, d = G.or_primary_ray(gc, 240, 0, 40 * 24 * 8)
        pick = np.linspace(0, len(s) - 1, per).astype(int)   # spread over the frame
        starts.append(s[pick])
        dirs.append(d[pick])
    perm = np.random.default_rng(20240).permutation(per * len(CAMERAS))[:N_SCATTER]
    start = np.ascontiguousarray(np.concatenate(starts)[perm])
    dir = np.ascontiguousarray(np.concatenate(dirs)[perm])
    want, seen = ref.trace(start, dir)
    for a in (start, dir, *want.values()):
        a.setflags(write=False)
    return g, built, ref, start, dir, want, seen


def _cuda(a):
    """a device copy (the shared arrays are read-only)"""
    return torch.from_numpy(np.array(a)).cuda()


def compare(got, want, what, keys=None):
    for k in keys or want:
        a = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        assert a.size == want[k].size and a.dtype == want[k].dtype, (what, k, a.shape, a.dtype)
        if a.size == 0:
            continue
        bad = np.nonzero(G.differs(a.reshape(want[k].shape), want[k]))[0]
        print("%s %s: %d of %d rays differ" % (what, k, bad.size, len(want[k])))
        assert bad.size == 0, "%s %s ray %d: device %r, prediction %r" % (what, k, bad[0], a.reshape(want[k].shape)[bad[0]],
                                                                          want[k][bad[0]])


def test_camera_rays_as_explicit_rays():
    """case 1: windows of the 2^24 benchmark rays, handed over explicitly, from device and from host arrays"""
    g, built, ref = final_case()[:3]
    scene = dt.Scene(built, g)
    try:
        for first in (0, N_BENCH // 2, N_BENCH - 4096):
            start, dir = G.or_primary_ray(g, 240, first, 4096)
            ws, wt = oracle.primary_hit(built, g, 240, first, 4096)
            assert (ws >= 0).any()
            want = {"shape": ws, "t": wt}
            ishape = torch.empty(4096, dtype=torch.int32, device="cuda")
            it = torch.empty(4096, dtype=torch.float32, device="cuda")
            dt.intersect_primary(scene, g, 240, first, ishape, it)
            compare({"shape": ishape, "t": it}, want, "dt_intersect_primary %d" % first)
            dev, st = dt.trace_rays(scene, g, _cuda(start), _cuda(dir), planes=("shape", "t"))
            assert dev["shape"].is_cuda and st.rays == 4096 and st.kernel_ms > 0
            compare(dev, want, "device arrays %d" % first)
            host, st = dt.trace_rays(scene, g, start, dir, planes=("shape", "t"))
            assert isinstance(host["t"], np.ndarray) and st.rays == 4096
            compare(host, want, "host arrays %d" % first)
    finally:
        scene.close()


def test_scattered_waves_all_planes_and_counts():
    """case 2: rays of seven cameras in one fixed permutation, n = 4096 + 37"""
    g, built, ref, start, dir, want, seen = final_case()
    desc = built.desc
    hit = want["shape"] >= 0
    assert len(start) == N_SCATTER and (~hit).any()
    waves = [hit[w:w + 64] for w in range(0, N_SCATTER, 64)]
    assert any(w.any() and not w.all() for w in waves)
    types_hit = {desc.shapes[int(s)].type for s in want["shape"][hit]}
    assert types_hit == {desc.shapes[i].type for i in range(desc.n_shapes)}, types_hit
    assert seen["textured"] > 0 and seen["checker"] > 0 and seen["border"] > 0, seen
    print("prediction:", seen, "misses", int((~hit).sum()), "types", sorted(types_hit))
    scene = dt.Scene(built, g)
    try:
        got, st = dt.trace_rays(scene, g, _cuda(start), _cuda(dir))
        compare(got, want, "scattered")
        assert st.rays == seen["rays"] == N_SCATTER
        assert st.tex_fetches == seen["tex_fetches"] and st.uv_out_of_range == seen["uv_out_of_range"]
        assert st.prism_norm_fallback == seen["prism_norm_fallback"]
        assert st.pixels == st.samples == st.shadow_rays == st.sky_pixels == st.nan_pixels == st.stack_overflows == 0
        got, _ = dt.trace_rays(scene, g, start, dir)
        compare(got, want, "scattered, host arrays")
    finally:
        scene.close()


_gold = np.load(os.path.join(HERE, "golden", "geom_ref.npz"))
_SCENES = [k for k in range(len(_gold["cam.shape"])) if _gold["cam.on_device"][k]]
_ONE_PER_TYPE = sorted({int(_gold["shapes"][_gold["cam.shape"][k]]["type"]): k for k in reversed(_SCENES)}.values())


def _rays_around(lb, ub, rng):
    """rays around a shape's bounds: from outside towards points in the box, from inside the box outwards
    (some start inside the shape), pointing away from it, and with one and two zero components of dir"""
    c, h = (lb + ub) / 2, np.maximum((ub - lb) / 2, 0.05)
    inside = lambda n: c + rng.uniform(-1, 1, (n, 3)) * h
    outside = lambda n: c + (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(n, 3))) * \
        (np.linalg.norm(h) * rng.uniform(1.5, 4, (n, 1)))
    S, D, tag = [], [], []

    def add(s, d, name):
        S.append(s)
        D.append(d)
        tag.extend([name] * len(s))

    s = outside(120)
    add(s, (inside(120) - s) * rng.uniform(0.3, 3, (120, 1)), "towards")
    s = inside(60)
    add(s, rng.normal(size=(60, 3)), "from inside")
    s = outside(40)
    add(s, (s - c) * rng.uniform(0.5, 2, (40, 1)), "away")
    for zero in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
        # axis-parallel rays through the box: the start differs from a point in it only along the free axes
        n = 16
        p = inside(n)
        d = rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(0.5, 2, (n, 3))
        d[:, list(zero)] = 0.0
        add(p - d * rng.uniform(1.5, 3, (n, 1)) * np.linalg.norm(h), d, "zero %s" % (zero,))
    return np.ascontiguousarray(np.concatenate(S)), np.ascontiguousarray(np.concatenate(D)), np.array(tag)


@pytest.mark.parametrize("k", _ONE_PER_TYPE, ids=["%d-%s" % (k, _gold["shape_names"][_gold["cam.shape"][k]])
                                                  for k in _ONE_PER_TYPE])
def test_one_shape_scenes(k):
    """case 3: the one-shape scenes of tests/golden/geom_ref.npz, one per supported type"""
    g = G.globals_from_record(_gold["cam.globals"][k])
    desc, keep = G.one_shape_scene(_gold["shapes"][_gold["cam.shape"][k]], _gold["holes"])
    ref = RayQueryRef(desc, g)
    lb, ub = ref.orc.bounds(0)
    start, dir, tag = _rays_around(lb, ub, np.random.default_rng(100 + k))
    want, seen = ref.trace(start, dir)
    hit = want["shape"] >= 0
    print("scene %d: %d rays, hits by kind %s" % (k, len(start), {t: int(hit[tag == t].sum()) for t in np.unique(tag)}))
    one = np.array([(d == 0).sum() == 1 for d in dir]), np.array([(d == 0).sum() == 2 for d in dir])
    assert one[0].sum() >= 48 and one[1].sum() >= 48
    assert hit[tag == "towards"].any() and (~hit).any()
    assert hit[one[0]].any() and hit[one[1]].any(), "no axis-parallel ray hits"
    if desc.shapes[0].type not in (3, 4, 6, 7):   # (flat shapes have no inside)
        assert hit[tag == "from inside"].any()
    assert not hit[tag == "away"].any()
    wocc = ref.occluded(start, dir)
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.trace_rays(scene, g, start, dir)
        compare(got, want, "scene %d" % k)
        assert st.prism_norm_fallback == seen["prism_norm_fallback"] and st.tex_fetches == seen["tex_fetches"]
        occ, _ = dt.rays_occluded(scene, g, start, dir)
        compare({"occluded": occ}, {"occluded": wocc}, "scene %d" % k)
    finally:
        scene.close()


@functools.lru_cache(maxsize=None)
def visibility_case():
    """case 4's segments and predictions: (a) from the hit points of case 2 to every light's centre, skipping
    the shape the light is; (b) between pairs of random points in the room. Seeds chosen on the CPU so that
    each outcome makes up at least a tenth of either set."""
    g, built, ref, start, dir, want, seen = final_case()
    desc = built.desc
    hit = np.nonzero(want["shape"] >= 0)[0][:600]
    pts = want["point"][hit]
    li = np.arange(len(pts)) % desc.n_lights
    centre = np.array([list(desc.lights[i].center) for i in range(desc.n_lights)])
    skip = np.array([desc.lights[i].shape_index for i in range(desc.n_lights)], np.int32)
    a = (np.ascontiguousarray(pts), np.ascontiguousarray(centre[li] - pts), np.ascontiguousarray(skip[li]))
    rng = np.random.default_rng(7)
    lo, hi = np.array([-9.5, 0.5, -4.5]), np.array([9.5, 10.0, 7.5])
    p, q = rng.uniform(lo, hi, (600, 3)), rng.uniform(lo, hi, (600, 3))
    b = (np.ascontiguousarray(p), np.ascontiguousarray(q - p))
    return a, ref.occluded(*a), b, ref.occluded(*b)


def test_visibility():
    """case 4"""
    g, built, ref = final_case()[:3]
    a, want_a, b, want_b = visibility_case()
    for name, w in (("a", want_a), ("b", want_b)):
        print("visibility (%s): %d of %d occluded" % (name, int(w.sum()), len(w)))
        assert 0.1 * len(w) <= w.sum() <= 0.9 * len(w), name
    assert len(set(a[2].tolist())) > 2   # the waves hold several skip_shape values
    scene = dt.Scene(built, g)
    try:
        got, st = dt.rays_occluded(scene, g, _cuda(a[0]), _cuda(a[1]), skip_shape=_cuda(a[2]))
        assert got.is_cuda and got.dtype == torch.uint8
        compare({"occluded": got}, {"occluded": want_a}, "to the lights")
        assert st.shadow_rays == len(want_a) and st.rays == 0 and st.kernel_ms > 0
        got, _ = dt.rays_occluded(scene, g, a[0], a[1], skip_shape=a[2])
        compare({"occluded": got}, {"occluded": want_a}, "to the lights, host arrays")
        got, _ = dt.rays_occluded(scene, g, b[0], b[1])
        compare({"occluded": got}, {"occluded": want_b}, "between points")
        minus, _ = dt.rays_occluded(scene, g, b[0], b[1], skip_shape=np.full(len(want_b), -1, np.int32))
        assert np.array_equal(minus, got)
    finally:
        scene.close()


def test_skip_shape_matters():
    """(the light's own shape hides its centre from below unless it is skipped: the skip is exercised)"""
    a, want_a, b, want_b = visibility_case()
    ref = final_case()[2]
    assert (ref.occluded(a[0][:100], a[1][:100]) != want_a[:100]).any()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_sizes(n):
    """case 5: no ray, one ray, a wave less one, a whole wave, a wave and one"""
    g, built, ref, start, dir, want, seen = final_case()
    va, wa, vb, wb = visibility_case()
    scene = dt.Scene(built, g)
    try:
        got, st = dt.trace_rays(scene, g, start[:n].copy(), dir[:n].copy())
        assert st.rays == n and all(len(v) == n for v in got.values())
        compare(got, {k: v[:n] for k, v in want.items()}, "n = %d" % n)
        occ, st = dt.rays_occluded(scene, g, _cuda(vb[0][:n]), _cuda(vb[1][:n]))
        assert st.shadow_rays == n and occ.numel() == n
        compare({"occluded": occ}, {"occluded": wb[:n]}, "n = %d" % n)
    finally:
        scene.close()


def test_void_rays_are_misses_and_leave_their_neighbours_alone():
    """case 5: NaN, inf and zero-dir rays interleaved with live ones"""
    g, built, ref, start, dir, want, seen = final_case()
    n = 200
    s, d = start[:n].copy(), dir[:n].copy()
    s[1::8, 0] = np.nan
    d[3::8, 2] = np.inf
    d[4::8] = 0.0
    s[6::8, 1] = -np.inf
    d[7::8, 1] = np.nan
    void = void_rays(s, d)
    assert void.sum() == 5 * n // 8 and (want["shape"][:n][~void] >= 0).any()
    va, wa, vb, wb = visibility_case()
    sb, db = vb[0][:n].copy(), vb[1][:n].copy()
    sb[void], db[void] = s[void], d[void]
    assert wb[:n][~void].any() and not wb[:n][~void].all()
    scene = dt.Scene(built, g)
    try:
        got, st = dt.trace_rays(scene, g, _cuda(s), _cuda(d))
        got = {k: v.cpu().numpy() for k, v in got.items()}
        assert st.rays == n - void.sum()
        compare({k: v[~void] for k, v in got.items()}, {k: v[:n][~void] for k, v in want.items()}, "live rays")
        assert (got["shape"][void] == -1).all() and (got["t"][void] == FLT_MAX).all()
        for k in ATTRS:
            assert not G.differs(got[k][void], np.zeros((int(void.sum()), 3))).any(), k
        occ, st = dt.rays_occluded(scene, g, sb, db)
        assert st.shadow_rays == n - void.sum()
        assert np.array_equal(occ[~void], wb[:n][~void]) and not occ[void].any()
    finally:
        scene.close()


def test_partial_planes_write_the_full_calls_bits():
    """case 6"""
    g, built, ref, start, dir, want, seen = final_case()
    scene = dt.Scene(built, g)
    try:
        for planes in (("shape",), ("normal",), ("t", "albedo")):
            got, st = dt.trace_rays(scene, g, start, dir, planes=planes)
            assert tuple(got) == planes
            compare(got, want, "planes %s" % (planes,), keys=planes)
            assert st.tex_fetches == (seen["tex_fetches"] if "albedo" in planes else 0)
    finally:
        scene.close()


def test_a_render_afterwards_is_unaffected():
    """case 7"""
    g, built, ref, start, dir, want, seen = final_case()
    va, wa, vb, wb = visibility_case()
    g2, built2 = _final(40, 24)
    g2.antialias_samples = 4
    scene = dt.Scene(built2, g2)
    try:
        a = torch.zeros(3 * 40 * 24, device="cuda")
        b = torch.zeros_like(a)
        dt.render(scene, g2, 240, a)
        dt.trace_rays(scene, g2, start[:512].copy(), dir[:512].copy())
        dt.rays_occluded(scene, g2, vb[0][:512].copy(), vb[1][:512].copy())
        st = dt.render(scene, g2, 240, b)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and st.pixels == 40 * 24
    finally:
        scene.close()


def test_prismcyl_scene_is_unsupported():
    """case 8"""
    g = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, g)
    scene = dt.Scene(built, g)
    rays = np.ones((4, 3))
    try:
        with pytest.raises(dt.DTError, match=r"dt_trace_rays failed \(-4\).*RectPrismWithCylinder"):
            dt.trace_rays(scene, g, rays, rays)
        with pytest.raises(dt.DTError, match=r"dt_rays_occluded failed \(-4\).*RectPrismWithCylinder"):
            dt.rays_occluded(scene, g, rays, rays)
    finally:
        scene.close()
