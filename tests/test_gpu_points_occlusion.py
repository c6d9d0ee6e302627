"""Occlusion queries at surface points (include/dt.h dt_points_occlusion; dt_points_occl_kernel) against the
prediction of tests/points_occlusion_ref.py, made on the CPU from the oracle's exports alone, bit for bit.

Every comparison is by bit pattern (uint32 views of the float32 planes); counters as integers. The scene is
scene_gen.features (the unit case) with its sphere, rectangle and point light. The points are the closest hits of
samples 0 and 1 of a 16x8 camera, traced on the CPU by RayQueryRef.trace, the first 130 of them. Probe r of sample
s of point i depends on (i, s, r) alone, so one prediction of 130 points x 4 samples x (2 AO probes + 3 lights),
2600 probes, serves every case here as a prefix cut."""
import functools
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import scene_gen
from oracle import geom as G
from points_occlusion_ref import PointsOcclusionRef
from rayquery_ref import RayQueryRef
from test_gpu_features import DTRENDER

pytestmark = pytest.mark.gpu

W, H = 16, 8
N_POINTS, N_SAMPLES, AO_RAYS, AO_RADIUS, LIGHTS = 130, 4, 2, 0.75, (0, 1, 2)   # sphere, rectangle, point light
FRAME = 3   # enters the RNG key only


def _unit():
    desc, g, keep = scene_gen.features(*scene_gen.CASES["unit"])
    g.xRes, g.yRes, g.antialias_samples = W, H, 1
    return desc, g, keep


@functools.lru_cache(maxsize=None)
def _case():
    """(prediction, points, normals, desc, g, keep): computed once, never written to"""
    desc, g, keep = _unit()
    rq = RayQueryRef(desc, g)
    start, ray = G.or_primary_ray(g, 0, 0, W * H * 8)
    start, ray = start.reshape(-1, 8, 3)[:, :2].reshape(-1, 3), ray.reshape(-1, 8, 3)[:, :2].reshape(-1, 3)
    out, _ = rq.trace(start, ray)
    hit = np.nonzero(out["shape"] >= 0)[0][:N_POINTS]
    assert len(hit) == N_POINTS and len(np.unique(out["shape"][hit])) >= 3
    p, n = np.ascontiguousarray(out["point"][hit]), np.ascontiguousarray(out["normal"][hit])
    for a in (p, n):
        a.setflags(write=False)
    ref = PointsOcclusionRef(desc, g, FRAME, p, n, N_SAMPLES, AO_RAYS, AO_RADIUS, LIGHTS, rq=rq)
    return ref, p, n, desc, g, keep


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = _bits(got[k]), _bits(want[k])
        bad = np.nonzero(g != w)[0] if g.size == w.size else np.array([-1])
        print("%s %s: %d of %d entries differ" % (what, k, bad.size, w.size))
        assert bad.size == 0, "%s %s entry %d" % (what, k, bad[0])


def _kw(**over):
    kw = dict(frame=FRAME, n_samples=N_SAMPLES, ao_rays=AO_RAYS, ao_radius=AO_RADIUS, lights=LIGHTS)
    kw.update(over)
    return kw


def _conditions(want):
    """what makes the comparison mean something, asserted of the prediction alone"""
    assert ((want["ao"] > 0) & (want["ao"] < 1)).any(), "no point with 0 < ao < 1"
    for j in range(want["light"].shape[1]):
        v = want["light"][:, j]
        assert (v > 0).any() and (v < 1).any(), "light %d is all lit or all dark" % j


def test_all_light_types_and_ao_host_and_device_arrays():
    ref, p, n, desc, g, keep = _case()
    want, probes = ref.planes(n_samples=3)
    _conditions(want)
    scene = dt.Scene(desc, g)
    try:
        host, sh = dt.points_occlusion(scene, g, p, n, **_kw(n_samples=3))
        dev, sd = dt.points_occlusion(scene, g, torch.from_numpy(p.copy()).cuda(), torch.from_numpy(n.copy()).cuda(),
                                      **_kw(n_samples=3))
        flat, _ = dt.points_occlusion(scene, g, p.reshape(-1), n.reshape(-1), **_kw(n_samples=3))
    finally:
        scene.close()
    assert isinstance(host["ao"], np.ndarray) and dev["ao"].is_cuda
    assert host["ao"].shape == (N_POINTS,) and host["light"].shape == (N_POINTS, 3)
    _same(host, want, "host arrays")
    _same(dev, want, "device arrays")
    _same(flat, want, "flat arrays")
    print("shadow_rays", sh.shadow_rays, sd.shadow_rays, "prediction", probes)
    assert sh.shadow_rays == sd.shadow_rays == probes and 0 < probes <= N_POINTS * 3 * (AO_RAYS + len(LIGHTS))
    assert sh.kernel_ms > 0 and sd.kernel_ms > 0
    for st in (sh, sd):   # everything else is 0
        d = st.as_dict()
        assert all(v == 0 for k, v in d.items() if k not in ("shadow_rays", "kernel_ms")), d


@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 130])
def test_tail_lanes_and_a_second_wave(n_points):
    ref, p, n, desc, g, keep = _case()
    want, probes = ref.planes(n_points=n_points)
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_occlusion(scene, g, np.ascontiguousarray(p[:n_points]), np.ascontiguousarray(n[:n_points]),
                                      **_kw())
    finally:
        scene.close()
    _same(got, want, "%d points" % n_points)
    assert st.shadow_rays == probes


def test_void_points_write_zeros_and_leave_their_neighbours_alone():
    ref, p, n, desc, g, keep = _case()
    pv, nv = p.copy(), n.copy()
    void = np.zeros(N_POINTS, bool)
    # interleaved, in both arrays, both kinds, in every component; the lanes 62..66 straddle the waves' border
    for i, (arr, comp, val) in {1: (pv, 0, np.nan), 4: (nv, 1, np.inf), 5: (pv, 2, -np.inf), 17: (nv, 0, np.nan),
                                62: (pv, 1, np.inf), 64: (nv, 2, np.nan), 66: (pv, 0, np.nan),
                                129: (nv, 1, -np.inf)}.items():
        arr[i, comp] = val
        void[i] = True
    want = PointsOcclusionRef(desc, g, FRAME, pv, nv, N_SAMPLES, AO_RAYS, AO_RADIUS, LIGHTS, rq=ref.rq)
    wantv, probesv = want.planes()
    clean, probes = ref.planes()
    assert probesv < probes
    scene = dt.Scene(desc, g)
    try:
        a, sa = dt.points_occlusion(scene, g, p, n, **_kw())
        b, sb = dt.points_occlusion(scene, g, pv, nv, **_kw())
        # a wave of void points only
        allv, sv = dt.points_occlusion(scene, g, np.full((70, 3), np.nan), np.ascontiguousarray(n[:70]), **_kw())
    finally:
        scene.close()
    _same(b, wantv, "with void points")
    assert sa.shadow_rays == probes and sb.shadow_rays == probesv and sv.shadow_rays == 0
    assert (_bits(b["ao"])[void] == 0).all() and (_bits(b["light"]).reshape(-1, 3)[void] == 0).all()
    assert np.array_equal(_bits(a["ao"])[~void], _bits(b["ao"])[~void])
    assert np.array_equal(_bits(a["light"]).reshape(-1, 3)[~void], _bits(b["light"]).reshape(-1, 3)[~void])
    assert (_bits(allv["ao"]) == 0).all() and (_bits(allv["light"]) == 0).all()


@pytest.mark.parametrize("n_samples", [1, 2, 4])
def test_n_samples_is_a_prefix_cut(n_samples):
    ref, p, n, desc, g, keep = _case()
    want, probes = ref.planes(n_samples=n_samples)
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_occlusion(scene, g, p, n, **_kw(n_samples=n_samples))
    finally:
        scene.close()
    _same(got, want, "%d samples" % n_samples)
    assert st.shadow_rays == probes


def test_plane_choice_costs_no_probes():
    """AO only and lights only write the full call's bits, and their probes add up to the full call's"""
    ref, p, n, desc, g, keep = _case()
    want, probes = ref.planes()
    scene = dt.Scene(desc, g)
    try:
        only_a, s_a = dt.points_occlusion(scene, g, p, n, **_kw(lights=()))
        only_l, s_l = dt.points_occlusion(scene, g, p, n, **_kw(ao_rays=0))
        one, _ = dt.points_occlusion(scene, g, p, n, **_kw(ao_rays=1))
        with pytest.raises(dt.DTError, match=r"\(-1\): dt_points_occlusion: lights\[1\].*the scene has 3 lights"):
            dt.points_occlusion(scene, g, p, n, **_kw(lights=(1, 3)))
        with pytest.raises(dt.DTError, match="every pointer is null"):
            dt.points_occlusion(scene, g, p, n, **_kw(ao_rays=0, lights=()))
    finally:
        scene.close()
    _same(only_a, {"ao": want["ao"]}, "ao only")
    _same(only_l, {"light": want["light"]}, "lights only")
    _same(one, ref.planes(ao_rays=1)[0], "one ao probe")
    assert s_a.shadow_rays + s_l.shadow_rays == probes and s_a.shadow_rays > 0 and s_l.shadow_rays > 0


def _covered_camera():
    """the unit scene seen from above: every pixel of the 16x8 frame hits the floor or what stands on it"""
    desc, g, keep = _unit()
    for a, (e, l) in enumerate(zip((0.2, 3.0, 1.5), (0.3, 0.0, 0.0))):
        g.eye[a], g.lookingAt[a] = e, l
    g.aperture, g.antialias_samples = 0.0, 1
    return desc, g, keep


def test_the_cameras_first_hits_give_render_occlusions_planes():
    """the cross-check with dt_occlusion_kernel: sample 0 of pixel y*xRes + x is point y*xRes + x"""
    desc, g, keep = _covered_camera()
    start, ray = G.or_primary_ray(g, 0, 0, W * H * 8)
    start, ray = np.ascontiguousarray(start.reshape(-1, 8, 3)[:, 0]), np.ascontiguousarray(ray.reshape(-1, 8, 3)[:, 0])
    cpu, _ = RayQueryRef(desc, g).trace(start, ray, attrs=False)
    assert (cpu["shape"] >= 0).all(), "coverage is not 1 everywhere"
    assert len(np.unique(cpu["shape"])) >= 3
    scene = dt.Scene(desc, g)
    try:
        hits, _ = dt.trace_rays(scene, g, torch.from_numpy(start).cuda(), torch.from_numpy(ray).cuda(),
                                planes=("shape", "point", "normal"))
        assert np.array_equal(hits["shape"].cpu().numpy(), cpu["shape"])
        got, st = dt.points_occlusion(scene, g, hits["point"], hits["normal"], frame=0, n_samples=1, ao_rays=3,
                                      ao_radius=AO_RADIUS, lights=LIGHTS)
        planes, so = dt.render_occlusion(scene, g, 0, n_samples=1, ao_rays=3, ao_radius=AO_RADIUS, lights=LIGHTS)
    finally:
        scene.close()
    # slot q = (yRes-1-y)*xRes + x of the image layout -> pixel y*xRes + x
    want = {"ao": planes["ao"].cpu().numpy().reshape(H, W)[::-1].reshape(-1),
            "light": planes["light"].cpu().numpy().reshape(H, W, 3)[::-1].reshape(-1, 3)}
    assert ((want["ao"] > 0) & (want["ao"] < 1)).any() and (want["light"] == 0).any() and (want["light"] == 1).any()
    _same(got, want, "points from the camera")
    assert st.shadow_rays == so.shadow_rays > 0


def _own_shape_scene():
    """a floor, a sphere light whose emitter shape encloses every target of its probes, and a plate between the
    light and one part of the floor"""
    b = scene_gen._Builder(1.0, (0.0, 0.0, 0.0))
    scene_gen._rect(b, (-6, 0, 6), (6, 0, 6), (6, 0, -6), (-6, 0, -6), (0.5, 0.5, 0.5))
    sl = b.shape(scene_gen.SPHERE, v=[(0, 3, 0)], radius=0.5, color=(1, 1, 0.9), emit=1, flags=scene_gen.F_LIGHT,
                 center=(0, 3, 0))
    scene_gen._rect(b, (0.5, 1.5, 2), (2.5, 1.5, 2), (2.5, 1.5, -2), (0.5, 1.5, -2), (0.7, 0.7, 0.7), flags=0)
    b.light(scene_gen.SPHERE_LIGHT, sl, 0.5, center=(0, 3, 0), color=(1, 1, 0.9), baxis=(0, -1, 0))
    g = b.globals((0.0, 2.0, 8.0), (0.0, 1.0, 0.0), 0.0, 6.0)
    g.xRes, g.yRes, g.antialias_samples = W, H, 1
    desc, keep = b.desc()
    return desc, g, keep, sl


def test_a_sphere_lights_own_shape_is_skipped_and_a_wall_is_not():
    desc, g, keep, sl = _own_shape_scene()
    p = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [-0.5, 0.0, 0.5]])
    n = np.tile([0.0, 1.0, 0.0], (3, 1))
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_occlusion(scene, g, p, n, frame=0, n_samples=4, ao_rays=0, lights=(0,))
        # the same question without the skip: the light's own shape hides its centre
        centre = np.array([[0.0, 3.0, 0.0]]) - p
        own, _ = dt.rays_occluded(scene, g, p, np.ascontiguousarray(centre))
        skipped, _ = dt.rays_occluded(scene, g, p, np.ascontiguousarray(centre), skip_shape=np.full(3, sl, np.int32))
    finally:
        scene.close()
    assert list(np.asarray(own)) == [1, 1, 1] and list(np.asarray(skipped)) == [0, 1, 0]
    # every target lies within 0.5 of the centre: below the plate all four probes are stopped, elsewhere none
    assert got["light"].reshape(-1).tolist() == [1.0, 0.0, 1.0] and st.shadow_rays == 12
    want, probes = PointsOcclusionRef(desc, g, 0, p, n, 4, 0, 1.0, (0,)).planes()
    _same(got, want, "own shape")


def test_a_render_before_and_after_is_the_same_bytes():
    ref, p, n, desc, g, keep = _case()
    desc, g, keep = _unit()
    g.antialias_samples, g.max_depth = 4, 3
    scene = dt.Scene(desc, g)
    try:
        a = torch.zeros(3 * W * H, device="cuda")
        b = torch.zeros_like(a)
        dt.render(scene, g, 0, a)
        o, _ = dt.points_occlusion(scene, g, p, n, **_kw())
        st = dt.render(scene, g, 0, b)
    finally:
        scene.close()
    assert (o["ao"] > 0).any() and (o["light"] > 0).any()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and st.pixels == W * H and (a != 0).any()


def test_prismcyl_is_unsupported_and_no_points_is_ok():
    ref, p, n, desc, g, keep = _case()
    gp = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, gp)
    scene = dt.Scene(built, gp)
    try:
        with pytest.raises(dt.DTError,
                           match=r"dt_points_occlusion failed \(-4\): dt_points_occlusion: .*RectPrismWithCylinder"):
            dt.points_occlusion(scene, gp, p, n, ao_radius=1.0)
    finally:
        scene.close()
    scene = dt.Scene(desc, g)
    try:
        for empty in (np.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.float64, device="cuda")):
            got, st = dt.points_occlusion(scene, g, empty, empty, **_kw())
            assert got["ao"].shape == (0,) and got["light"].shape == (0, 3)
            assert st.shadow_rays == 0 and st.kernel_ms == 0
    finally:
        scene.close()


def test_bake_occlusion_is_points_occlusion_on_the_texels():
    desc, g, keep = _unit()
    floor, tri = 0, 4   # scene_gen.features: the checkerboard floor, the raw triangle
    assert desc.shapes[floor].type == scene_gen.CHECKER and desc.shapes[tri].type == scene_gen.TRIANGLE
    kw = dict(frame=FRAME, n_samples=2, ao_rays=2, ao_radius=AO_RADIUS, lights=LIGHTS)
    scene = dt.Scene(desc, g)
    try:
        pts, nrm = dt.shape_texels(desc, floor, 8, 4)   # cross(B-A, D-A) points up, into the room
        assert (nrm == [0.0, 1.0, 0.0]).all()
        want, sw = dt.points_occlusion(scene, g, pts, nrm, **kw)
        got, sg = dt.bake_occlusion(scene, desc, g, floor, 8, 4, **kw)
        tp, tn = dt.shape_texels(desc, tri, 4, 4)
        twant, _ = dt.points_occlusion(scene, g, tp, tn, **kw)
        tgot, _ = dt.bake_occlusion(scene, desc, g, tri, 4, 4, **kw)
    finally:
        scene.close()
    assert got["ao"].shape == (4, 8) and got["light"].shape == (4, 8, 3) and sg.shadow_rays == sw.shadow_rays > 0
    _same(got, want, "bake of the floor")
    assert (want["ao"] > 0).any() and (want["light"] > 0).any() and (want["light"] < 1).any()
    # the triangle's 10 texels inside it, in order; the 6 outside stay 0
    a, b = np.meshgrid((np.arange(4) + 0.5) / 4, (np.arange(4) + 0.5) / 4)
    inside = (a + b <= 1).reshape(-1)
    assert inside.sum() == len(tp) == 10
    assert np.array_equal(_bits(tgot["ao"])[inside], _bits(twant["ao"])) and (_bits(tgot["ao"])[~inside] == 0).all()
    assert np.array_equal(_bits(tgot["light"]).reshape(16, 3)[inside], _bits(twant["light"]).reshape(10, 3))


def test_cli_bake_occlusion_images(tmp_path):
    """dtrender final 30 --bake-occlusion S ...: the PNGs are the bytes dt_write_png makes of bake_occlusion's planes
    through occlusion_images, and the frame is the file written without the flag"""
    g = dt.globals_default()   # the CLI's globals: defaults, no models, buildFinal(240), then the options
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = 40, 24, 16, 2
    d = built.desc
    shape = next(i for i in range(d.n_shapes) if d.shapes[i].type in (scene_gen.RECTANGLE, scene_gen.CHECKER))
    BW, BH = 8, 4
    common = [DTRENDER, "final", "30", "--res", "40x24", "--spp", "16", "--depth", "2"]
    plain, with_b, prefix = str(tmp_path / "plain.png"), str(tmp_path / "bake.png"), str(tmp_path / "B")
    subprocess.run(common + ["--out", plain], check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run(common + ["--out", with_b, "--bake-occlusion", str(shape), "--bake-size", "%dx%d" % (BW, BH),
                             "--bake-out", prefix, "--bake-samples", "3", "--ao-rays", "2", "--occlusion-lights", "0,1"],
                   check=True, timeout=120, stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_b, "rb").read()
    scene = dt.Scene(built, g)
    try:
        planes, _ = dt.bake_occlusion(scene, built, g, shape, BW, BH, frame=240, n_samples=3, ao_rays=2, lights=(0, 1))
    finally:
        scene.close()
    gb = g.copy()
    gb.xRes, gb.yRes = BW, BH
    imgs = dt.occlusion_images(gb, planes)
    assert sorted(imgs) == ["ao", "light0", "light1"]
    for name, v in imgs.items():
        want = str(tmp_path / ("want.%s.png" % name))
        dt.write_png(want, gb, np.ascontiguousarray(v, np.float32))
        assert open("%s.%s.png" % (prefix, name), "rb").read() == open(want, "rb").read(), name
    assert imgs["ao"].max() > 0
    # a usage error: no size
    r = subprocess.run(common + ["--out", with_b, "--bake-occlusion", str(shape), "--bake-out", prefix],
                       timeout=120, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--bake-size" in r.stderr
