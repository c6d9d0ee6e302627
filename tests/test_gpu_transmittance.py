"""Transmittance queries (include/dt.h dt_rays_transmittance, dt_points_occlusion_glass; dt_rayq_transmit_kernel,
dt_points_occl_glass_kernel) against the restatement of tests/transmittance_ref.py, bit for bit: int32 planes as
integers, float32 planes by bit pattern. The scenes, ray sets and points are the helper's; that they hold every
class of ray is asserted on the CPU by tests/test_transmittance_host.py. Predictions are computed once
(transmittance_ref.prediction, points_case) and shared."""
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import scene_gen
import transmittance_ref as T
from test_gpu_features import DTRENDER

pytestmark = pytest.mark.gpu


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _same_int(got, want, what):
    for k in want:
        a = _np(got[k])
        assert a.dtype == np.int32 and a.shape == want[k].shape, (what, k, a.shape, a.dtype)
        bad = np.nonzero((a != want[k]).reshape(len(a), -1).any(axis=1))[0] if a.size else np.array([], int)
        print("%s %s: %d of %d rays differ" % (what, k, bad.size, len(a)))
        assert bad.size == 0, "%s %s ray %d: device %r, prediction %r" % (what, k, bad[0], a[bad[0]], want[k][bad[0]])


def _bits(a):
    return np.ascontiguousarray(_np(a), np.float32).reshape(-1).view(np.uint32)


def _same_f32(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        g, w = _bits(got[k]), _bits(want[k])
        bad = np.nonzero(g != w)[0] if g.size == w.size else np.array([-1])
        print("%s %s: %d of %d entries differ" % (what, k, bad.size, w.size))
        assert bad.size == 0, "%s %s entry %d" % (what, k, bad[0])


@pytest.fixture(scope="module")
def scenes():
    made = {}
    for name in ("stack", "glass"):
        desc, g, keep, tr = T.scene(name)
        made[name] = (dt.Scene(desc, g), g, tr)
    yield made
    for sc, g, tr in made.values():
        sc.close()


@pytest.mark.parametrize("name", ["stack", "glass"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 3 + 7])
def test_ray_counts_host_and_device_arrays(scenes, name, n):
    scene, g, tr = scenes[name]
    s, d, sk = (np.ascontiguousarray(a[:n]) for a in T.ray_set(name))
    want = {k: v[:n] for k, v in T.prediction(name, 2).items()}
    host, sh = dt.rays_transmittance(scene, g, s, d, skip_shape=sk, k=2)
    dev, sd = dt.rays_transmittance(scene, g, _cuda(s), _cuda(d), skip_shape=_cuda(sk), k=2)
    assert isinstance(host["panes"], np.ndarray) and dev["panes"].is_cuda and dev["pane_shape"].shape == (n, 2)
    _same_int(host, want, "%s host %d" % (name, n))
    _same_int(dev, want, "%s device %d" % (name, n))
    assert sh.shadow_rays == sd.shadow_rays == n and sh.kernel_ms > 0
    d_ = sh.as_dict()
    assert all(v == 0 for k, v in d_.items() if k not in ("shadow_rays", "kernel_ms")), d_


@pytest.mark.parametrize("k", [0, 1, 2, 3, 8])
def test_values_of_k_on_the_pane_stack(scenes, k):
    """every list capacity (0, 1, 2, 4, 8), a k below its capacity (3), up to five panes crossed"""
    scene, g, tr = scenes["stack"]
    s, d, sk = T.ray_set("stack")
    want = T.prediction("stack", k)
    assert want["panes"].max() == 5
    got, _ = dt.rays_transmittance(scene, g, s.copy(), d.copy(), skip_shape=sk.copy(), k=k)
    assert got["pane_shape"].shape == (len(s), k)
    _same_int(got, want, "k = %d" % k)
    # each plane alone gives the full call's bits
    only, _ = dt.rays_transmittance(scene, g, s.copy(), d.copy(), skip_shape=sk.copy(), k=k, planes=("panes",))
    assert sorted(only) == ["panes"]
    _same_int(only, {"panes": want["panes"]}, "k = %d, panes alone" % k)
    if k > 0:
        only, _ = dt.rays_transmittance(scene, g, s.copy(), d.copy(), skip_shape=sk.copy(), k=k, planes=("pane_shape",))
        assert sorted(only) == ["pane_shape"]
        _same_int(only, {"pane_shape": want["pane_shape"]}, "k = %d, pane_shape alone" % k)


def test_void_rays_in_a_wave_leave_their_neighbours_alone(scenes):
    scene, g, tr = scenes["glass"]
    s, d, sk = (np.array(a[:130]) for a in T.ray_set("glass"))
    s[5, 1] = np.nan
    d[17] = 0.0
    d[40, 2] = np.inf
    s[70, 0] = -np.inf
    want = tr.transmittance(s, d, sk, 2)
    void = [5, 17, 40, 70]
    assert (want["panes"][void] == 0).all() and (want["pane_shape"][void] == -1).all()
    keep = np.setdiff1d(np.arange(130), void)
    assert np.array_equal(want["panes"][keep], T.prediction("glass", 2)["panes"][:130][keep])
    got, st = dt.rays_transmittance(scene, g, s, d, skip_shape=sk, k=2)
    _same_int(got, want, "void rays")
    assert st.shadow_rays == 130 - 4


def test_blocked_waves(scenes):
    """a wave where every lane is blocked early, and one where exactly one lane is not and walks on"""
    scene, g, tr = scenes["stack"]
    for n_clear in (0, 1):
        s, d, _ = T.blocked_wave_rays(n_clear)
        want = tr.transmittance(s, d, None, 8)
        assert (want["panes"] == -1).sum() == 64 - n_clear
        got, _ = dt.rays_transmittance(scene, g, s, d, k=8)
        _same_int(got, want, "blocked wave, %d clear" % n_clear)


@pytest.mark.parametrize("name", ["stack", "glass"])
def test_panes_nonzero_is_rays_occluded_on_the_device(scenes, name):
    scene, g, tr = scenes[name]
    s, d, sk = (_cuda(a) for a in T.ray_set(name))
    got, _ = dt.rays_transmittance(scene, g, s, d, skip_shape=sk, k=0)
    occ, _ = dt.rays_occluded(scene, g, s, d, skip_shape=sk)
    assert got["pane_shape"].shape == (len(s), 0)
    assert torch.equal(got["panes"] != 0, occ != 0) and occ.any() and not occ.all()


def test_order_gives_the_same_bits(scenes):
    for name in ("stack", "glass"):
        scene, g, tr = scenes[name]
        s, d, sk = T.ray_set(name)
        want = T.prediction(name, 2)
        got, _ = dt.rays_transmittance(scene, g, s.copy(), d.copy(), skip_shape=sk.copy(), k=2, order=True)
        _same_int(got, want, "%s order=True host" % name)
        got, _ = dt.rays_transmittance(scene, g, _cuda(s), _cuda(d), skip_shape=_cuda(sk), k=2, order=True)
        _same_int(got, want, "%s order=True device" % name)


def _final(W, H):
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes = W, H
    return g, built


def test_final_first_hits_towards_the_lights_and_the_scene_afterwards():
    """2048 camera rays of final(240), their first hits, and from there to every light's centre with the light's
    own shape skipped: (panes != 0) is rays_occluded on the device; a render afterwards is the render before"""
    g, built = _final(64, 32)
    g.antialias_samples = 1
    scene = dt.Scene(built, g)
    try:
        a = torch.zeros(3 * 64 * 32, device="cuda")
        b = torch.zeros_like(a)
        dt.render(scene, g, 240, a)
        start, dir = dt.camera_rays(g, 240, samples=(0, 1))
        start, dir = start.reshape(-1, 3), dir.reshape(-1, 3)
        assert len(start) == 2048
        hits, _ = dt.trace_rays(scene, g, start, dir, planes=("shape", "point"))
        assert int((hits["shape"] >= 0).sum()) > 1024
        blocked = clear = 0
        assert built.desc.n_lights == 5
        for li in range(built.desc.n_lights):
            L = built.desc.lights[li]
            centre = torch.tensor(list(L.center), dtype=torch.float64, device="cuda")
            seg = (centre[None, :] - hits["point"]).contiguous()
            skip = torch.full((2048,), int(L.shape_index), dtype=torch.int32, device="cuda")
            got, st = dt.rays_transmittance(scene, g, hits["point"], seg, skip_shape=skip, k=1)
            occ, so = dt.rays_occluded(scene, g, hits["point"], seg, skip_shape=skip)
            assert torch.equal(got["panes"] != 0, occ != 0), "light %d" % li
            assert st.shadow_rays == so.shadow_rays == 2048
            # a listed pane only where there is one
            assert torch.equal(got["pane_shape"][:, 0] >= 0, got["panes"] > 0)
            blocked += int((got["panes"] == -1).sum())
            clear += int((got["panes"] == 0).sum())
        print("final(240): %d blocked, %d clear of %d" % (blocked, clear, 5 * 2048))
        assert blocked > 0 and clear > 0
        st = dt.render(scene, g, 240, b)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and st.pixels == 64 * 32
    finally:
        scene.close()


def test_prismcyl_scene_is_unsupported_and_no_rays_launch_nothing(scenes):
    g = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, g)
    scene = dt.Scene(built, g)
    rays = np.ones((4, 3))
    try:
        with pytest.raises(dt.DTError, match=r"dt_rays_transmittance failed \(-4\).*RectPrismWithCylinder"):
            dt.rays_transmittance(scene, g, rays, rays)
        with pytest.raises(dt.DTError, match=r"dt_points_occlusion_glass failed \(-4\).*RectPrismWithCylinder"):
            dt.points_occlusion(scene, g, rays, rays, through_glass=1)
    finally:
        scene.close()
    scene, g, tr = scenes["stack"]
    got, st = dt.rays_transmittance(scene, g, np.zeros((0, 3)), np.zeros((0, 3)), k=2)
    assert got["panes"].shape == (0,) and got["pane_shape"].shape == (0, 2) and st.shadow_rays == 0 and st.kernel_ms == 0
    with pytest.raises(dt.DTError, match=r"dt_points_occlusion_glass: lights\[0\] = 7"):   # the scene is looked at last
        dt.points_occlusion(scene, g, rays, rays, lights=(7,), through_glass=1)


# ---------------------------------------------------------------------------------------------------
# points
# ---------------------------------------------------------------------------------------------------
def _pkw(**over):
    P = T.POINTS
    kw = dict(frame=P["frame"], n_samples=P["n_samples"], ao_rays=P["ao_rays"], ao_radius=P["ao_radius"],
              lights=P["lights"])
    kw.update(over)
    return kw


@pytest.mark.parametrize("n_points", [1, 65, 256])
@pytest.mark.parametrize("max_panes", [1, 8])
def test_points_against_the_restatement(scenes, n_points, max_panes):
    """256 points hold the void point (100) in the middle of the second wave"""
    scene, g, tr = scenes["glass"]
    ref, p, n = T.points_case()
    want, probes = ref.planes(max_panes, n_points=n_points)
    pp, nn = np.ascontiguousarray(p[:n_points]), np.ascontiguousarray(n[:n_points])
    host, sh = dt.points_occlusion(scene, g, pp, nn, through_glass=max_panes, **_pkw())
    dev, sd = dt.points_occlusion(scene, g, _cuda(pp), _cuda(nn), through_glass=max_panes, **_pkw())
    _same_f32(host, want, "host %d points" % n_points)
    _same_f32(dev, want, "device %d points" % n_points)
    assert sh.shadow_rays == sd.shadow_rays == probes
    if n_points == 256:
        assert (want["light_panes"] > 0).any() and (want["ao_panes"] > 0).any()
        for k in want:
            assert (_bits(host[k]).reshape(256, -1)[100] == 0).all(), k


@pytest.mark.parametrize("n_samples,ao_rays,lights", [(1, 4, (0, 1)), (5, 0, (0, 1)), (1, 4, ()), (5, 4, (1,))])
def test_points_samples_probes_and_lights(scenes, n_samples, ao_rays, lights):
    scene, g, tr = scenes["glass"]
    ref, p, n = T.points_case()
    pp, nn = np.ascontiguousarray(p[:130]), np.ascontiguousarray(n[:130])
    if lights == (1,):   # another light list: a prediction of its own, of 70 points
        pp, nn = np.ascontiguousarray(p[60:130]), np.ascontiguousarray(n[60:130])
        P = T.POINTS
        want, probes = T.PointsTransmitRef(None, g, P["frame"], pp, nn, n_samples, ao_rays, P["ao_radius"], lights,
                                           tr=tr).planes(1)
    else:
        want, probes = ref.planes(1, n_points=130, n_samples=n_samples, ao_rays=ao_rays)
        if not lights:
            want = {k: v for k, v in want.items() if k.startswith("ao")}
    got, st = dt.points_occlusion(scene, g, pp, nn, through_glass=1, **_pkw(n_samples=n_samples, ao_rays=ao_rays,
                                                                           lights=lights))
    _same_f32(got, want, "n_samples %d ao_rays %d lights %r" % (n_samples, ao_rays, lights))
    if lights != (1,) and lights:
        assert st.shadow_rays == probes


def test_points_max_panes_0_is_points_occlusion_on_the_device(scenes):
    scene, g, tr = scenes["glass"]
    ref, p, n = T.points_case()
    pd, nd = _cuda(p), _cuda(n)
    old, so = dt.points_occlusion(scene, g, pd, nd, **_pkw())
    new, sn = dt.points_occlusion(scene, g, pd, nd, through_glass=0, **_pkw())
    one, _ = dt.points_occlusion(scene, g, pd, nd, through_glass=1, **_pkw())
    assert sorted(old) == ["ao", "light"] and sorted(new) == ["ao", "ao_panes", "light", "light_panes"]
    _same_f32({k: new[k] for k in old}, {k: _np(v) for k, v in old.items()}, "max_panes = 0")
    assert so.shadow_rays == sn.shadow_rays > 0
    assert not new["ao_panes"].any() and not new["light_panes"].any()
    # a texel behind the pane: dark at 0, lit at 1
    lit = (new["light"] == 0) & (one["light"] > 0)
    print("texels lit through the pane:", int(lit.sum()))
    assert lit.any()


def test_pane_planes_alone_through_the_c_abi(scenes):
    """a row of probes runs for either of its two planes: light_panes wanted, light not (out wants ao only)"""
    import ctypes
    from distraytracer_amd._lib import Occlusion, OcclusionPanes
    scene, g, tr = scenes["glass"]
    ref, p, n = T.points_case()
    want, _ = ref.planes(1, n_points=65)
    pp, nn = np.ascontiguousarray(p[:65]), np.ascontiguousarray(n[:65])
    P = T.POINTS
    prm = dt.occlusion_params_default()
    prm.ao_rays, prm.ao_radius, prm.n_lights = P["ao_rays"], P["ao_radius"], 2
    prm.lights[0], prm.lights[1] = 0, 1
    ao, lp = np.full(65, 7, np.float32), np.full((65, 2), 7, np.float32)
    st = dt.Stats()
    dt.check(dt.lib.dt_points_occlusion_glass(scene.handle, ctypes.byref(g), P["frame"], 65, pp.ctypes.data, nn.ctypes.data,
                                              P["n_samples"], ctypes.byref(prm), 1,
                                              ctypes.byref(Occlusion(ao.ctypes.data, None)),
                                              ctypes.byref(OcclusionPanes(None, lp.ctypes.data)), 0, None, ctypes.byref(st)),
             "dt_points_occlusion_glass")
    _same_f32({"ao": ao, "light_panes": lp}, {"ao": want["ao"], "light_panes": want["light_panes"]}, "planes alone")


def test_bake_occlusion_through_glass(scenes):
    scene, g, tr = scenes["glass"]
    desc = T.scene("glass")[0]
    kw = _pkw(n_samples=2)
    pts, nrm = dt.shape_texels(desc, T.GLASS_FLOOR, 8, 8)
    assert (nrm == [0.0, 1.0, 0.0]).all()
    want, _ = dt.points_occlusion(scene, g, pts, nrm, through_glass=1, **kw)
    got, _ = dt.bake_occlusion(scene, desc, g, T.GLASS_FLOOR, 8, 8, through_glass=1, **kw)
    assert got["light_panes"].shape == (8, 8, 2) and got["ao_panes"].shape == (8, 8)
    _same_f32(got, want, "bake through glass")
    plain, _ = dt.bake_occlusion(scene, desc, g, T.GLASS_FLOOR, 8, 8, **kw)
    assert sorted(plain) == ["ao", "light"]


def test_cli_bake_through_glass_images(tmp_path):
    """dtrender final 30 --bake-occlusion S --bake-through-glass 1: the PNGs are dt_write_png's bytes of
    bake_occlusion(through_glass=1)'s planes through occlusion_images; without the flag, of through_glass=None's,
    and no pane image is written"""
    import os
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = 40, 24, 1, 2
    d = built.desc
    shape = next(i for i in range(d.n_shapes) if d.shapes[i].type in (scene_gen.RECTANGLE, scene_gen.CHECKER))
    BW, BH = 8, 4
    common = [DTRENDER, "final", "30", "--res", "40x24", "--spp", "1", "--depth", "2", "--bake-occlusion", str(shape),
              "--bake-size", "%dx%d" % (BW, BH), "--bake-samples", "3", "--ao-rays", "2", "--occlusion-lights", "0,1"]
    subprocess.run(common + ["--out", str(tmp_path / "a.png"), "--bake-out", str(tmp_path / "P")],
                   check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run(common + ["--out", str(tmp_path / "b.png"), "--bake-out", str(tmp_path / "G"), "--bake-through-glass", "1"],
                   check=True, timeout=120, stdout=subprocess.DEVNULL)
    assert open(tmp_path / "a.png", "rb").read() == open(tmp_path / "b.png", "rb").read()
    gb = g.copy()
    gb.xRes, gb.yRes = BW, BH
    scene = dt.Scene(built, g)
    try:
        for prefix, tg, names in (("P", None, ["ao", "light0", "light1"]),
                                  ("G", 1, ["ao", "ao_panes", "light0", "light1", "light_panes0", "light_panes1"])):
            planes, _ = dt.bake_occlusion(scene, built, g, shape, BW, BH, frame=240, n_samples=3, ao_rays=2, lights=(0, 1),
                                          through_glass=tg)
            imgs = dt.occlusion_images(gb, planes)
            assert sorted(imgs) == names
            written = sorted(f[len(prefix) + 1:-4] for f in os.listdir(tmp_path) if f.startswith(prefix + "."))
            assert written == names, written
            for name, v in imgs.items():
                want = str(tmp_path / ("want.%s.%s.png" % (prefix, name)))
                dt.write_png(want, gb, np.ascontiguousarray(v, np.float32))
                assert open(tmp_path / ("%s.%s.png" % (prefix, name)), "rb").read() == open(want, "rb").read(), (prefix, name)
    finally:
        scene.close()
    r = subprocess.run(common + ["--out", str(tmp_path / "c.png"), "--bake-out", str(tmp_path / "X"),
                                 "--bake-through-glass", "9"], timeout=120, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--bake-through-glass" in r.stderr
