"""Occlusion feature buffers (include/dt.h dt_render_occlusion; dt_occlusion_kernel) against the prediction of
tests/occlusion_ref.py, made on the CPU from the oracle's exports alone, bit for bit.

Every comparison is by bit pattern (oracle.geom.differs); counters as integers. The unit scene is
scene_gen.features at 24x16 with all three of its lights (sphere, rectangle, point) and 3 AO probes. A sample's
primary ray and probes depend on (pixel, sample) alone, not on spp, so one prediction of 128 samples serves the
cases at 64 spp, at 16 spp (the leading 16: four pixels per wave) and at 144 spp (spp is a square; n_samples 64
and 128: one and two chunks). The prediction costs one ctypes call per gathered shape and probe."""
import functools
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import scene_gen
from occlusion_ref import OcclusionRef, first_occluder
from oracle import geom as G
from test_gpu_features import DTRENDER, _final, _read_png, compare

pytestmark = pytest.mark.gpu

W, H = 24, 16
AO_RAYS, AO_RADIUS, LIGHTS = 3, 0.75, (0, 1, 2)   # the unit case: sphere, rectangle and point light


def _unit(aa):
    desc, g, keep = scene_gen.features(*scene_gen.CASES["unit"])
    g.xRes, g.yRes, g.antialias_samples = W, H, aa
    return desc, g, keep


@functools.lru_cache(maxsize=None)
def _unit_ref():
    desc, g, keep = _unit(144)
    return OcclusionRef(desc, g, 0, 128, AO_RAYS, AO_RADIUS, LIGHTS), desc, g, keep


def _image_order(g, planes):
    """full-frame image-layout planes (torch or numpy) -> arrays indexed [y, x(, slot)] like the prediction's"""
    out = {}
    for k, v in planes.items():
        a = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        a = a.reshape(g.yRes, g.xRes, -1) if k == "light" else a.reshape(g.yRes, g.xRes)
        out[k] = a[::-1].copy()
    return out


def _check(got, st, want, cnt, pixels, n, what):
    compare(got, {k: want[k] for k in got}, what)
    print(what, "stats: shadow_rays", st.shadow_rays, "prediction", cnt["shadow_rays"], "prism",
          st.prism_norm_fallback, cnt["prism_norm_fallback"])
    assert st.shadow_rays == cnt["shadow_rays"] and st.prism_norm_fallback == cnt["prism_norm_fallback"]
    assert st.pixels == pixels and st.samples == st.rays == pixels * n and st.kernel_ms > 0
    assert st.sky_pixels == st.nan_pixels == st.stack_overflows == st.tex_fetches == st.uv_out_of_range == 0


def _conditions(want):
    """what makes the comparison mean something, asserted of the prediction alone"""
    cov = want["coverage"]
    assert (cov < 1).any(), "no pixel with coverage < 1"
    if "ao" in want:
        assert ((want["ao"] > 0) & (want["ao"] < cov)).any(), "no covered pixel with 0 < ao < coverage"
    if "light" in want:
        for j in range(want["light"].shape[2]):
            v = want["light"][:, :, j]
            assert ((v > 0) & (v < cov)).any(), "no covered pixel with 0 < light %d < coverage" % j


@pytest.mark.parametrize("aa,n", [(64, 64), (16, 16), (144, 64), (144, 128)],
                         ids=["64spp", "16spp-4-pixels-per-wave", "144spp-1-chunk", "144spp-2-chunks"])
def test_unit_scene_planes_and_counters(aa, n):
    ref, desc, g0, keep = _unit_ref()
    want, cnt = ref.planes(n)
    _conditions(want)
    desc, g, keep2 = _unit(aa)
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.render_occlusion(scene, g, 0, n_samples=n, ao_rays=AO_RAYS, ao_radius=AO_RADIUS, lights=LIGHTS)
    finally:
        scene.close()
    _check(_image_order(g, got), st, want, cnt, W * H, n, "unit %d of %d spp" % (n, aa))
    assert st.shadow_rays <= cnt["hits"] * (AO_RAYS + len(LIGHTS))


@pytest.mark.parametrize("layout", [dt.DT_OUT_IMAGE, dt.DT_OUT_SLAB], ids=["image", "slab"])
def test_tile_share_host_and_device_arrays(layout):
    """world = 2, both ranks: a rank's own pixels hold the full-frame call's values, nothing else is written, host
    arrays come back as device arrays do, and the two ranks partition the frame"""
    ref, desc, g0, keep = _unit_ref()
    want, cnt = ref.planes(64)
    desc, g, keep2 = _unit(64)
    nl = len(LIGHTS)
    scene = dt.Scene(desc, g)
    owner = np.full(W * H, -1)
    kw = dict(n_samples=64, ao_rays=AO_RAYS, ao_radius=AO_RADIUS, lights=LIGHTS)
    try:
        full, _ = dt.render_occlusion(scene, g, 0, **kw)
        full = {k: v.cpu().numpy() for k, v in full.items()}
        for rank in range(2):
            tile = dt.tiles(tile_w=8, tile_h=8, rank=rank, world=2, layout=layout)
            n1 = dt.accum_doubles(g, tile) // 3
            dev = {"ao": torch.full((n1,), -77.0, device="cuda"), "light": torch.full((n1 * nl,), -77.0, device="cuda")}
            host = {"ao": np.full(n1, -77, np.float32), "light": np.full(n1 * nl, -77, np.float32)}
            _, sd = dt.render_occlusion(scene, g, 0, tile=tile, out=dev, **kw)
            _, sh = dt.render_occlusion(scene, g, 0, tile=tile, out=host, **kw)
            dev = {k: v.cpu().numpy() for k, v in dev.items()}
            tiles_x, n_tiles = 3, 6
            own_q, own_px = [], []
            for slot in range((n_tiles + 1) // 2):
                h = (slot * 2654435761) & 0xFFFFFFFF   # dt_scene_dev.h tile_of
                h ^= h >> 15
                h = (h * 0x2c1b3c6d) & 0xFFFFFFFF
                h ^= h >> 12
                t = slot * 2 + (rank + h % 2) % 2
                if t >= n_tiles:
                    continue
                ty, tx = divmod(t, tiles_x)
                for py in range(8):
                    for px in range(8):
                        e = (H - 1 - (ty * 8 + py)) * W + tx * 8 + px
                        own_px.append(e)
                        own_q.append(e if layout == dt.DT_OUT_IMAGE else slot * 64 + py * 8 + px)
            own_q, own_px = np.array(own_q), np.array(own_px)
            assert sd.pixels == sh.pixels == own_q.size and sd.shadow_rays == sh.shadow_rays > 0
            assert (owner[own_px] == -1).all()
            owner[own_px] = rank
            for k, per in (("ao", 1), ("light", nl)):
                a, b, f = dev[k].reshape(-1, per), host[k].reshape(-1, per), full[k].reshape(-1, per)
                assert not G.differs(a[own_q].reshape(-1), f[own_px].reshape(-1)).any(), (rank, k)
                assert not G.differs(dev[k], host[k]).any(), (rank, k)
                rest = np.ones(len(a), bool)
                rest[own_q] = False
                assert (a[rest] == -77).all() and (b[rest] == -77).all(), (rank, k)
        assert (owner >= 0).all()
    finally:
        scene.close()
    compare(_image_order(g, full), {k: want[k] for k in full}, "unit full frame")


def test_the_planes_hold_what_rays_occluded_answers():
    """without the oracle: the probes the prediction generated for one pixel row, handed to dt_rays_occluded, give
    the counts the planes hold (count = plane * the divisor, exact: the quotient of small integers rounds back)"""
    ref, desc, g0, keep = _unit_ref()
    want, _ = ref.planes(64)
    y = int(np.argmax(((want["ao"] > 0) & (want["ao"] < want["coverage"])).sum(axis=1)))
    desc, g, keep2 = _unit(64)
    # the hitting samples of row y among the leading 64: entries [y, x, i] of the prediction
    idx = np.arange(W * H * ref.n).reshape(H, W, ref.n)[y, :, :64].reshape(-1)
    sel = np.nonzero(np.isin(ref.at, idx))[0]
    x_of = (ref.at[sel] // ref.n) % W
    scene = dt.Scene(desc, g)
    try:
        got, _ = dt.render_occlusion(scene, g, 0, ao_rays=AO_RAYS, ao_radius=AO_RADIUS, lights=LIGHTS)
        got = _image_order(g, got)
        V = np.zeros(W, np.int64)
        for k in range(AO_RAYS + len(LIGHTS)):
            skip = None if k < AO_RAYS else np.full(len(sel), desc.lights[LIGHTS[k - AO_RAYS]].shape_index, np.int32)
            occ, _ = dt.rays_occluded(scene, g, np.ascontiguousarray(ref.p[sel]), np.ascontiguousarray(ref.dirs[k][sel]),
                                      skip_shape=skip)
            occ = np.asarray(occ.cpu() if hasattr(occ, "cpu") else occ)
            un = np.bincount(x_of[occ == 0], minlength=W)
            if k < AO_RAYS:
                V += un
            else:
                j = k - AO_RAYS
                assert np.array_equal(np.rint(got["light"][y, :, j].astype(np.float64) * 64).astype(np.int64), un), j
        assert np.array_equal(np.rint(got["ao"][y].astype(np.float64) * 64 * AO_RAYS).astype(np.int64), V)
        assert V.max() > 0
    finally:
        scene.close()


def test_edge_cases_of_the_plane_choice():
    """ao_rays = 0 with lights only; lights empty with AO only; a light listed twice gives two planes, equal for
    the point light (no draw) and different for the rectangle light (sub = j*16 differs); light indices outside
    the scene"""
    ref, desc, g0, keep = _unit_ref()
    want, cnt = ref.planes(64)
    desc, g, keep2 = _unit(64)
    scene = dt.Scene(desc, g)
    try:
        only_l, s_l = dt.render_occlusion(scene, g, 0, ao_rays=0, lights=LIGHTS)
        only_a, s_a = dt.render_occlusion(scene, g, 0, ao_rays=AO_RAYS, ao_radius=AO_RADIUS)
        twice, _ = dt.render_occlusion(scene, g, 0, ao_rays=0, lights=(2, 2, 1, 1))
        dflt, _ = dt.render_occlusion(scene, g, 0)   # occlusion_params_default: 4 probes, radius 1.0
        unit, _ = dt.render_occlusion(scene, g, 0, ao_rays=4, ao_radius=1.0)
        for bad in (-1, 3):
            with pytest.raises(dt.DTError, match=r"\(-1\): dt_render_occlusion: lights\[1\].*the scene has 3 lights"):
                dt.render_occlusion(scene, g, 0, ao_rays=0, lights=(1, bad))
        with pytest.raises(dt.DTError, match="at most 8"):
            dt.render_occlusion(scene, g, 0, lights=range(9), ao_radius=1.0)
        with pytest.raises(dt.DTError, match="every pointer is null"):
            dt.render_occlusion(scene, g, 0, ao_rays=0)
        p = dt.Progressive(scene, g, 0)
        with pytest.raises(dt.DTError, match="no window rendered"):
            p.occlusion()
        p.step()
        prog, _ = p.occlusion(AO_RAYS, AO_RADIUS, LIGHTS)
    finally:
        scene.close()
    assert list(only_l) == ["light"] and list(only_a) == ["ao"] and list(dflt) == ["ao"]
    compare(_image_order(g, only_l), {"light": want["light"]}, "lights only")
    compare(_image_order(g, only_a), {"ao": want["ao"]}, "ao only")
    compare(_image_order(g, prog), {k: want[k] for k in ("ao", "light")}, "Progressive.occlusion")
    assert s_l.shadow_rays + s_a.shadow_rays == cnt["shadow_rays"] and s_l.shadow_rays > 0 and s_a.shadow_rays > 0
    t = twice["light"].cpu().numpy().reshape(-1, 4)
    assert np.array_equal(t[:, 0].view(np.uint32), t[:, 1].view(np.uint32)) and (t[:, 0] > 0).any()
    assert not np.array_equal(t[:, 2], t[:, 3]) and (t[:, 2] > 0).any() and (t[:, 3] > 0).any()
    assert torch.equal(dflt["ao"].view(torch.int32), unit["ao"].view(torch.int32))
    assert (dflt["ao"] > 0).any() and float(dflt["ao"].max()) <= 1.0


def _types(desc, shapes):
    return {desc.shapes[int(i)].type for i in np.unique(shapes)}


def test_final_frame_is_the_prediction():
    """final(240) without the models at 40x24, 16 spp: the checkerboard floor with its hole, the checker cylinder
    and the textured shapes under the primary hits; 2 AO probes and the scene's first two lights"""
    g, built = _final(240, 40, 24, 16)
    lights = (0, 1)
    ref = OcclusionRef(built, g, 240, 16, 2, 1.0, lights)
    want, cnt = ref.planes(16)
    hit_shapes = np.unique(ref.shape[ref.hit])
    assert _types(built.desc, hit_shapes) & {6, 7, 8}, "no primary hit on a checkerboard shape"
    assert any(built.desc.shapes[int(i)].flags & 4 for i in hit_shapes), "no primary hit on a textured shape"
    assert ((want["ao"] > 0) & (want["ao"] < want["coverage"])).any()
    assert ((want["light"] > 0) & (want["light"] < want["coverage"][:, :, None])).any()
    scene = dt.Scene(built, g)
    try:
        got, st = dt.render_occlusion(scene, g, 240, ao_rays=2, ao_radius=1.0, lights=lights)
    finally:
        scene.close()
    _check(_image_order(g, got), st, want, cnt, 40 * 24, 16, "final(240)")


MESH_EYE, MESH_AT = (1.0, 3.0, 7.5), (3.2, 3.0, 4.7)   # in front of the column and bust at x = 2.8 .. 3.8
MESH_LIGHTS = (1, 2)                                    # two of the ceiling's rectangle lights


def _mesh_case():
    """final(240) with use_model = 1 (the column and bust meshes: 1664 of their triangles carry uv vertices), the eye moved in
    front of one column, 16x12 at 4 spp (sixteen pixels per wave): the prediction walks every node per ray, so
    the frame is as small as still shows the meshes"""
    g = dt.globals_default()
    g.use_model = 1
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples = 16, 12, 4
    for a in range(3):
        g.eye[a], g.lookingAt[a] = MESH_EYE[a], MESH_AT[a]
    return g, built


def test_final_frame_with_meshes_is_the_prediction():
    """the mesh path: primary hits on mesh triangles (their normals), and probes that mesh triangles stop
    (occluded_walk over the mesh's leaves), both asserted of the prediction alone"""
    g, built = _mesh_case()
    d = built.desc
    mesh = np.array([d.shapes[i].type == 3 and bool(d.shapes[i].flags & (1 << 6)) for i in range(d.n_shapes)])
    assert mesh.sum() > 1000
    ref = OcclusionRef(built, g, 240, 4, 2, 1.0, MESH_LIGHTS)
    want, cnt = ref.planes(4)
    on_mesh = int(mesh[ref.shape[ref.hit]].sum())
    stopped = []
    for k in range(2 + len(MESH_LIGHTS)):
        idx = np.nonzero(~ref.unocc[ref.at, k])[0]
        skip = None if k < 2 else np.full(len(idx), d.lights[MESH_LIGHTS[k - 2]].shape_index, np.int32)
        by = first_occluder(ref.rq, ref.p[idx], ref.dirs[k][idx], skip)
        assert (by >= 0).all()
        stopped.append(int(mesh[by].sum()))
    print("mesh case: primary hits on the meshes", on_mesh, "of", cnt["hits"], "; probes stopped by a mesh triangle",
          stopped)
    assert on_mesh > 100 and sum(stopped[:2]) > 0 and sum(stopped[2:]) > 0
    assert ((want["ao"] > 0) & (want["ao"] < want["coverage"])).any()
    assert ((want["light"] > 0) & (want["light"] < want["coverage"][:, :, None])).any()
    scene = dt.Scene(built, g)
    try:
        got, st = dt.render_occlusion(scene, g, 240, ao_rays=2, ao_radius=1.0, lights=MESH_LIGHTS)
    finally:
        scene.close()
    _check(_image_order(g, got), st, want, cnt, 16 * 12, 4, "final(240) with meshes")


def test_a_render_before_and_after_is_the_same_bytes():
    desc, g, keep = _unit(64)
    g.antialias_samples, g.max_depth = 4, 3
    scene = dt.Scene(desc, g)
    try:
        a = torch.zeros(3 * W * H, device="cuda")
        b = torch.zeros_like(a)
        dt.render(scene, g, 0, a)
        o, _ = dt.render_occlusion(scene, g, 0, ao_rays=AO_RAYS, ao_radius=AO_RADIUS, lights=LIGHTS)
        st = dt.render(scene, g, 0, b)
    finally:
        scene.close()
    assert (o["ao"] > 0).any() and (o["light"] > 0).any()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and st.pixels == W * H


def test_prismcyl_scene_is_unsupported():
    g = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, g)
    g.xRes, g.yRes, g.antialias_samples = 16, 12, 4
    scene = dt.Scene(built, g)
    try:
        with pytest.raises(dt.DTError, match=r"dt_render_occlusion failed \(-4\): dt_render_occlusion: .*RectPrismWithCylinder"):
            dt.render_occlusion(scene, g, 30, ao_radius=1.0)
    finally:
        scene.close()


def test_cli_occlusion_images(tmp_path):
    """dtrender final 30 --occlusion P at 40x24, 16 spp: P.ao.png and P.light<j>.png are the Python planes times
    255 (distraytracer_amd.occlusion_images), and the frame is the file written without the flag"""
    common = [DTRENDER, "final", "30", "--res", "40x24", "--spp", "16", "--depth", "2"]
    plain, with_o, prefix = str(tmp_path / "plain.png"), str(tmp_path / "occl.png"), str(tmp_path / "P")
    subprocess.run(common + ["--out", plain], check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run(common + ["--out", with_o, "--occlusion", prefix, "--ao-rays", "2", "--occlusion-lights", "0,1"],
                   check=True, timeout=120, stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_o, "rb").read()
    g = dt.globals_default()   # the CLI's globals: defaults, no models, buildFinal(240), then the options
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = 40, 24, 16, 2
    scene = dt.Scene(built, g)
    try:
        planes, _ = dt.render_occlusion(scene, g, 240, ao_rays=2, lights=(0, 1))
    finally:
        scene.close()
    imgs = dt.occlusion_images(g, {k: v.cpu().numpy() for k, v in planes.items()})
    assert sorted(imgs) == ["ao", "light0", "light1"]
    for name, v in imgs.items():
        png = _read_png("%s.%s.png" % (prefix, name))
        assert png.shape == (24, 40, 3)
        assert np.array_equal(png.reshape(-1), v.astype(np.uint8)), name
    # (this camera sees neither light unshadowed at 40x24; the light planes' values are the other cases' matter)
    assert imgs["ao"].max() > 0 and imgs["ao"].max() <= 255


def test_render_image_writes_the_occlusion_images(tmp_path):
    """renderImage(..., occlusion=prefix): the PNGs are render_occlusion's planes through occlusion_images, the
    frame is the file written without it, and upsample refuses the combination"""
    def globals_():
        g = dt.globals_default()
        g.use_model = 0
        g.xRes, g.yRes, g.antialias_samples, g.max_depth = 40, 24, 16, 2
        return g
    plain, with_o, prefix = str(tmp_path / "plain.png"), str(tmp_path / "occl.png"), str(tmp_path / "R")
    a, _ = dt.renderImage(plain, 240, "final", globals_())
    b, _ = dt.renderImage(with_o, 240, "final", globals_(), occlusion=prefix, ao_rays=2, ao_radius=0.5,
                          occlusion_lights=(1, 2))
    assert np.array_equal(a, b) and open(plain, "rb").read() == open(with_o, "rb").read()
    with pytest.raises(dt.DTError, match="upsample renders one low-resolution frame.*occlusion"):
        dt.renderImage(str(tmp_path / "u.png"), 240, "final", globals_(), upsample=2, occlusion=prefix)
    g = globals_()
    built = dt.build_scene("final", 240, g)
    scene = dt.Scene(built, g)
    try:
        planes, _ = dt.render_occlusion(scene, g, 240, ao_rays=2, ao_radius=0.5, lights=(1, 2))
    finally:
        scene.close()
    imgs = dt.occlusion_images(g, {k: v.cpu().numpy() for k, v in planes.items()})
    assert sorted(imgs) == ["ao", "light0", "light1"]
    for name, v in imgs.items():
        png = _read_png("%s.%s.png" % (prefix, name))
        assert png.shape == (24, 40, 3) and np.array_equal(png.reshape(-1), v.astype(np.uint8)), name
    assert imgs["ao"].max() > 0 and imgs["light0"].max() > 0
