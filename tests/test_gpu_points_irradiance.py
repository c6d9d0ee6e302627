"""Irradiance queries at surface points (include/dt.h dt_points_irradiance; dt_points_irr_kernel) against the
prediction of tests/points_irradiance_ref.py, made on the CPU from the oracle's exports and the two host exports,
bit for bit.

Every comparison is by bit pattern (uint32 views of the float32 planes); counters as integers. The fixture is
tests/test_gpu_points_occlusion.py's: scene_gen.features (the unit case) with its sphere, rectangle and point light,
and as points the first 130 closest hits of samples 0 and 1 of a 16x8 camera, traced on the CPU. A probe of sample s
of point i depends on (i, s, r, slot) alone, so one prediction of 130 points x 4 samples x (3 light probes + 2
gather probes x (1 closest hit + 3 light probes)), 5720 walks, serves the cases here as prefix cuts; the void
points and the other light choices take smaller predictions of their own."""
import functools
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import scene_gen
from oracle import geom as G
from points_irradiance_ref import F_LIGHT, PointsIrradianceRef
from rayquery_ref import RayQueryRef
from test_gpu_features import DTRENDER

pytestmark = pytest.mark.gpu

W, H = 16, 8
N_POINTS, N_SAMPLES, GATHER, LIGHTS = 130, 4, 2, (0, 1, 2)   # sphere, rectangle, point light
FRAME = 3   # enters the RNG key only
ALL = ("direct", "direct_rgb", "indirect_rgb", "sky")


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
    ref = PointsIrradianceRef(desc, g, FRAME, p, n, N_SAMPLES, LIGHTS, GATHER, rq=rq)
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


def _counts(st, counts, what=""):
    print(what, "shadow_rays", st.shadow_rays, "rays", st.rays, "prediction", counts)
    assert st.shadow_rays == counts["shadow_rays"] and st.rays == counts["rays"], what
    d = st.as_dict()   # everything else is 0
    assert all(v == 0 for k, v in d.items() if k not in ("shadow_rays", "rays", "kernel_ms")), d


def _kw(**over):
    kw = dict(frame=FRAME, n_samples=N_SAMPLES, lights=LIGHTS, gather_rays=GATHER)
    kw.update(over)
    return kw


def test_the_prediction_exercises_every_path():
    """what makes the comparisons mean something, asserted of the prediction alone"""
    ref, p, n, desc, g, keep = _case()
    want, counts = ref.planes()
    for j in range(len(LIGHTS)):
        v = want["direct"][:, j]
        assert ((v > 0) & (v < v.max())).any(), "light slot %d: no point strictly between 0 and its maximum" % j
    assert (want["indirect_rgb"] != 0).any(), "no point with indirect light"
    assert ((want["sky"] > 0) & (want["sky"] < 1)).any(), "sky is 0 or 1 everywhere"
    assert ref.g_emit.any(), "no gather probe ends on a DT_F_LIGHT shape"
    assert (ref.g_traced & ~ref.g_miss & ~ref.g_emit).any(), "no gather probe ends on a surface that is shaded"
    assert any(desc.shapes[i].flags & F_LIGHT for i in range(desc.n_shapes))
    assert 0 < counts["rays"] <= N_POINTS * N_SAMPLES * GATHER
    assert N_POINTS * N_SAMPLES * len(LIGHTS) <= counts["shadow_rays"]


def test_all_planes_host_device_and_flat_arrays():
    ref, p, n, desc, g, keep = _case()
    want, counts = ref.planes(n_samples=3)
    scene = dt.Scene(desc, g)
    try:
        host, sh = dt.points_irradiance(scene, g, p, n, **_kw(n_samples=3))
        dev, sd = dt.points_irradiance(scene, g, torch.from_numpy(p.copy()).cuda(), torch.from_numpy(n.copy()).cuda(),
                                       **_kw(n_samples=3))
        flat, sf = dt.points_irradiance(scene, g, p.reshape(-1), n.reshape(-1), **_kw(n_samples=3))
    finally:
        scene.close()
    assert isinstance(host["direct"], np.ndarray) and dev["direct"].is_cuda
    assert host["direct"].shape == (N_POINTS, 3) and host["direct_rgb"].shape == (N_POINTS, 3)
    assert host["indirect_rgb"].shape == (N_POINTS, 3) and host["sky"].shape == (N_POINTS,)
    _same(host, want, "host arrays")
    _same(dev, want, "device arrays")
    _same(flat, want, "flat arrays")
    for st in (sh, sd, sf):
        _counts(st, counts)
        assert st.kernel_ms > 0


@pytest.mark.parametrize("n_points", [1, 63, 64, 65, 130])
def test_tail_lanes_and_a_second_wave(n_points):
    ref, p, n, desc, g, keep = _case()
    want, counts = ref.planes(n_points=n_points)
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_irradiance(scene, g, np.ascontiguousarray(p[:n_points]), np.ascontiguousarray(n[:n_points]),
                                       **_kw())
    finally:
        scene.close()
    _same(got, want, "%d points" % n_points)
    _counts(st, counts)


@pytest.mark.parametrize("n_samples", [1, 3])
def test_n_samples_is_a_prefix_cut(n_samples):
    ref, p, n, desc, g, keep = _case()
    want, counts = ref.planes(n_samples=n_samples)
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_irradiance(scene, g, p, n, **_kw(n_samples=n_samples))
    finally:
        scene.close()
    _same(got, want, "%d samples" % n_samples)
    _counts(st, counts)


@pytest.mark.parametrize("gather_rays", [0, 1, 2])
def test_gather_rays_is_a_prefix_cut(gather_rays):
    ref, p, n, desc, g, keep = _case()
    want, counts = ref.planes(gather_rays=gather_rays)
    assert sorted(want) == sorted(ALL if gather_rays else ALL[:2])
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_irradiance(scene, g, p, n, **_kw(gather_rays=gather_rays))
    finally:
        scene.close()
    _same(got, want, "%d gather rays" % gather_rays)
    _counts(st, counts)
    assert (counts["rays"] == 0) == (gather_rays == 0)


@pytest.mark.parametrize("plane", ALL)
def test_each_plane_alone_costs_only_its_own_probes(plane):
    ref, p, n, desc, g, keep = _case()
    want, counts = ref.planes(want=(plane,))
    full = ref.planes()[1]
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_irradiance(scene, g, p, n, **_kw(planes=(plane,)))
    finally:
        scene.close()
    _same(got, want, plane + " alone")
    _counts(st, counts, plane)
    # a NULL plane costs no probes: the direct rows, the gather walks and the gather's light loop are each skipped
    direct = ref.planes(want=("direct",))[1]["shadow_rays"]
    expect = {"direct": (direct, 0), "direct_rgb": (direct, 0),
              "indirect_rgb": (full["shadow_rays"] - direct, full["rays"]), "sky": (0, full["rays"])}[plane]
    assert (st.shadow_rays, st.rays) == expect and 0 < direct < full["shadow_rays"]


@functools.lru_cache(maxsize=None)
def _edge_case():
    """70 points, 2 samples, 1 gather probe: void points at 5 and 64 (a point, a normal), a zero normal at 9"""
    ref, p, n, desc, g, keep = _case()
    pv, nv = p[:70].copy(), n[:70].copy()
    pv[5, 1] = np.nan
    nv[64, 2] = np.inf
    nv[9] = 0.0
    return PointsIrradianceRef(desc, g, FRAME, pv, nv, 2, LIGHTS, 1, rq=ref.rq), pv, nv


def test_void_points_and_a_zero_normal():
    ref, p, n, desc, g, keep = _case()
    edge, pv, nv = _edge_case()
    want, counts = edge.planes()
    clean, clean_counts = ref.planes(n_points=70, n_samples=2, gather_rays=1)
    assert counts["shadow_rays"] < clean_counts["shadow_rays"] and counts["rays"] < clean_counts["rays"]
    # the zero normal: every cosine is 0, and the gather probe is the ball point's direction itself
    assert (want["direct"][9] == 0).all() and (want["direct_rgb"][9] == 0).all() and edge.g_traced[9].all()
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_irradiance(scene, g, pv, nv, **_kw(n_samples=2, gather_rays=1))
        allv, sv = dt.points_irradiance(scene, g, np.full((70, 3), np.nan), np.ascontiguousarray(n[:70]), **_kw())
    finally:
        scene.close()
    _same(got, want, "void points and a zero normal")
    _counts(st, counts)
    other = np.ones(70, bool)
    other[[5, 9, 64]] = False
    for k in ALL:
        a, c = _bits(got[k]).reshape(70, -1), _bits(clean[k]).reshape(70, -1)
        assert (a[[5, 64]] == 0).all(), k                      # a void point writes 0 to every plane
        assert np.array_equal(a[other], c[other]), k           # and leaves its neighbours alone
        assert (_bits(allv[k]) == 0).all(), k                  # a wave of void points only
    assert sv.shadow_rays == 0 and sv.rays == 0


@pytest.mark.parametrize("lights", [(2, 0), (1,)])
def test_light_subsets_and_slot_order(lights):
    ref, p, n, desc, g, keep = _case()
    pp, nn = np.ascontiguousarray(p[:70]), np.ascontiguousarray(n[:70])
    sub = PointsIrradianceRef(desc, g, FRAME, pp, nn, 2, lights, 1, rq=ref.rq)
    want, counts = sub.planes()
    assert (want["direct"] > 0).any() and want["direct"].shape == (70, len(lights))
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_irradiance(scene, g, pp, nn, **_kw(n_samples=2, gather_rays=1, lights=lights))
        with pytest.raises(dt.DTError, match=r"\(-1\): dt_points_irradiance: light\[1\] = 3, the scene has 3 lights"):
            dt.points_irradiance(scene, g, pp, nn, **_kw(lights=(1, 3)))
    finally:
        scene.close()
    _same(got, want, "lights %r" % (lights,))
    _counts(st, counts)
    if lights == (2, 0):   # the point light draws nothing: its column is slot 2's of the full prediction
        full = ref.planes(n_points=70, n_samples=2, gather_rays=1)[0]
        assert np.array_equal(_bits(want["direct"][:, 0]), _bits(full["direct"][:, 2]))


def test_direct_is_the_occlusion_calls_visibility_weighted_by_the_cosine():
    ref, p, n, desc, g, keep = _case()
    scene = dt.Scene(desc, g)
    try:
        irr, _ = dt.points_irradiance(scene, g, p, n, **_kw(gather_rays=0, planes=("direct",)))
        occ, _ = dt.points_occlusion(scene, g, p, n, frame=FRAME, n_samples=N_SAMPLES, ao_rays=0, lights=LIGHTS)
        irr1, _ = dt.points_irradiance(scene, g, p, n, **_kw(n_samples=1, gather_rays=0, planes=("direct",)))
        occ1, _ = dt.points_occlusion(scene, g, p, n, frame=FRAME, n_samples=1, ao_rays=0, lights=LIGHTS)
    finally:
        scene.close()
    assert not ((irr["direct"] > 0) & ~(occ["light"] > 0)).any()
    assert (irr["direct"] > 0).any()
    # the point light, one sample: direct == cosine x visibility exactly
    centre = np.array(list(desc.lights[2].center))
    cos = np.array([dt.irradiance_cosine(n[i], centre - p[i]) for i in range(N_POINTS)])
    vis = occ1["light"][:, 2]
    assert set(np.unique(vis)) <= {0.0, 1.0} and (vis == 1).any() and (vis == 0).any()
    assert np.array_equal(_bits(irr1["direct"][:, 2]), _bits((cos * vis.astype(np.float64)).astype(np.float32)))


def test_prismcyl_is_unsupported_and_no_points_is_ok():
    ref, p, n, desc, g, keep = _case()
    gp = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, gp)
    scene = dt.Scene(built, gp)
    try:
        with pytest.raises(dt.DTError,
                           match=r"dt_points_irradiance failed \(-4\): dt_points_irradiance: .*RectPrismWithCylinder"):
            dt.points_irradiance(scene, gp, p, n, lights=(0,))
    finally:
        scene.close()
    scene = dt.Scene(desc, g)
    try:
        for empty in (np.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.float64, device="cuda")):
            got, st = dt.points_irradiance(scene, g, empty, empty, **_kw())
            assert got["direct"].shape == (0, 3) and got["sky"].shape == (0,)
            assert st.shadow_rays == 0 and st.rays == 0 and st.kernel_ms == 0
    finally:
        scene.close()


def test_bake_irradiance_is_points_irradiance_on_the_texels():
    desc, g, keep = _unit()
    floor = 0   # scene_gen.features: the checkerboard floor
    assert desc.shapes[floor].type == scene_gen.CHECKER
    kw = dict(frame=FRAME, n_samples=2, lights=LIGHTS, gather_rays=1)
    scene = dt.Scene(desc, g)
    try:
        pts, nrm = dt.shape_texels(desc, floor, 8, 8)   # cross(B-A, D-A) points up, into the room
        assert (nrm == [0.0, 1.0, 0.0]).all()
        want, sw = dt.points_irradiance(scene, g, pts, nrm, **kw)
        got, sg = dt.bake_irradiance(scene, desc, g, floor, 8, 8, **kw)
    finally:
        scene.close()
    assert got["direct"].shape == (8, 8, 3) and got["direct_rgb"].shape == (8, 8, 3)
    assert got["indirect_rgb"].shape == (8, 8, 3) and got["sky"].shape == (8, 8)
    assert sg.shadow_rays == sw.shadow_rays > 0 and sg.rays == sw.rays > 0
    _same(got, want, "bake of the floor")
    assert (want["direct_rgb"] > 0).any() and (want["sky"] > 0).any()
    # ... and it is the prediction's bits
    ref = PointsIrradianceRef(desc, g, FRAME, pts, nrm, 2, LIGHTS, 1)
    _same(want, ref.planes()[0], "texels against the prediction")


def test_cli_bake_light_images(tmp_path):
    """dtrender final 30 --bake-light S ...: the PNGs are the bytes dt_write_png makes of bake_irradiance's planes
    through irradiance_images, and the frame is the file written without the flag"""
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
    subprocess.run(common + ["--out", with_b, "--bake-light", str(shape), "--bake-size", "%dx%d" % (BW, BH),
                             "--bake-out", prefix, "--bake-samples", "3", "--bake-gather", "2",
                             "--occlusion-lights", "0,1"],
                   check=True, timeout=120, stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_b, "rb").read()
    scene = dt.Scene(built, g)
    try:
        planes, _ = dt.bake_irradiance(scene, built, g, shape, BW, BH, frame=240, n_samples=3, lights=(0, 1),
                                       gather_rays=2)
    finally:
        scene.close()
    gb = g.copy()
    gb.xRes, gb.yRes = BW, BH
    imgs = dt.irradiance_images(gb, planes)
    assert sorted(imgs) == ["direct", "indirect", "sky"]
    for name, v in imgs.items():
        want = str(tmp_path / ("want.%s.png" % name))
        dt.write_png(want, gb, np.ascontiguousarray(v, np.float32))
        assert open("%s.%s.png" % (prefix, name), "rb").read() == open(want, "rb").read(), name
    assert imgs["direct"].max() > 0
    # a usage error: no lights
    r = subprocess.run(common + ["--out", with_b, "--bake-light", str(shape), "--bake-size", "8x4", "--bake-out", prefix],
                       timeout=120, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--occlusion-lights" in r.stderr
