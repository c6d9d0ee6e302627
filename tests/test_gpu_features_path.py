"""Specular-path feature buffers (include/dt.h dt_render_features_path; dt_features_path_kernel) against the
prediction of tests/features_path_ref.py, made on the CPU from the oracle's exports alone, bit for bit.

Every comparison is by bit pattern (oracle.geom.differs); shape ids and counters as integers. Each case first
asserts of its own prediction that it contains what it claims to exercise. The resolutions are the tests': the
prediction costs one ctypes call per gathered shape. One prediction per scene follows every sample for 8
bounces; the cases at fewer bounces and fewer samples are cuts of it (PathRef.planes)."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import scene_gen
from denoise_ref import denoise_ref_params
from features_path_ref import COUNTERS, GLASS, PLANES, REFRACT, STEEL, STOP, PathRef
from oracle import geom as G
from test_gpu_features import DTRENDER, _final, _read_png, compare, image_order

pytestmark = pytest.mark.gpu

GLASS_SPHERE, STEEL_SPHERE = 1, 2   # their indices in scene_gen.features


def _unit(aa):
    """scene_gen.features("unit") at 24x16; the eye moved closer to the two spheres, so that they fill enough
    of so small a frame for every kind of path the cases ask for (asserted where it is used)"""
    desc, g, keep = scene_gen.features(*scene_gen.CASES["unit"])
    g.xRes, g.yRes, g.antialias_samples = 24, 16, aa
    for a, v in enumerate((-2.2, 1.5, 3.2)):
        g.eye[a] = v
    for a, v in enumerate((-0.3, 0.8, 0.2)):
        g.lookingAt[a] = v
    return desc, g, keep


@functools.lru_cache(maxsize=None)
def _unit_paths():
    desc, g, keep = _unit(144)   # spp is a square: 144, of which the cases take the leading 64 and 128
    return PathRef(desc, g).trace(g, 0, 128, 8), desc, g, keep


@functools.lru_cache(maxsize=None)
def _final_paths(nogloss):
    g, built = _final(240, 40, 24, 64, nogloss=nogloss)
    return PathRef(built, g).trace(g, 240, 64, 2), built, g


def _device(scene, g, frame, n, K, **kw):
    st = dt.Stats()
    got = dt.render_features(scene, g, frame, n_samples=n, planes=PLANES, stats=st, specular_bounces=K, **kw)
    return image_order(g, got), st


def _check_stats(st, cnt, pixels, n):
    for k in COUNTERS:
        assert getattr(st, k) == cnt[k], (k, getattr(st, k), cnt[k])
    assert st.pixels == pixels and st.samples == pixels * n and st.kernel_ms > 0
    assert st.shadow_rays == st.sky_pixels == st.nan_pixels == st.stack_overflows == st.glossy_exhausted == 0


@pytest.mark.parametrize("what", ["final", "unit"])
def test_zero_bounces_is_render_features(what):
    """case 1: the tie to the existing kernel, every plane, device against device"""
    if what == "final":
        g, built = _final(240, 40, 24, 64)
        frame = 240
    else:
        built, g, keep = _unit(64)
        frame = 0
    scene = dt.Scene(built, g)
    try:
        s0, s1 = dt.Stats(), dt.Stats()
        first = dt.render_features(scene, g, frame, stats=s0)
        assert "bounces" not in first
        with pytest.raises(dt.DTError, match="unknown plane"):
            dt.render_features(scene, g, frame, planes=("bounces",))
        # max_bounces = 0 through the new export itself
        from distraytracer_amd._lib import Features
        n1 = g.xRes * g.yRes
        out = {k: (torch.full((n1,), -7, dtype=torch.int32, device="cuda") if k == "shape" else
                   torch.full((n1 * (3 if k in ("albedo", "normal") else 1),), -7.0, device="cuda")) for k in PLANES}
        f = Features(*[out[k].data_ptr() for k in PLANES[:5]])
        import ctypes
        dt.check(dt.lib.dt_render_features_path(scene.handle, ctypes.byref(g), frame, None, 64, 0, ctypes.byref(f),
                                                ctypes.c_void_p(out["bounces"].data_ptr()), 1, None, ctypes.byref(s1)),
                 "dt_render_features_path")
    finally:
        scene.close()
    for k in PLANES[:5]:
        assert torch.equal(out[k].view(torch.int32), first[k].view(torch.int32)), k
    assert (out["bounces"] == 0).all() and (first["coverage"] > 0).any()
    for k in ("pixels", "samples", "rays", "tex_fetches", "uv_out_of_range", "prism_norm_fallback", "reflect_errors"):
        assert getattr(s0, k) == getattr(s1, k), k


def test_the_unit_prediction_holds_every_path():
    """what cases 2 and 3 exercise, asserted of the prediction (CPU only, but it is the GPU cases' premise)"""
    ref, desc, g, keep = _unit_paths()
    s0, s1 = ref.seg[0], ref.seg[1]
    assert (s0["hit"] & (s0["shape"] == STEEL_SPHERE) & (s0["code"] == 1)).any(), "no reflection off the steel sphere"
    into = s0["hit"] & (s0["shape"] == GLASS_SPHERE) & (s0["code"] == REFRACT) & (s0["inside"] == 0)
    out_of = s1["hit"] & (s1["shape"] == GLASS_SPHERE) & (s1["code"] == REFRACT) & (s1["inside"] == 1)
    assert into.any() and out_of.any(), "no refraction into and out of the glass sphere"
    # cut off by max_bounces = 1 while still on glass: segment 1 hits the glass from inside and would go on
    assert out_of.sum() > 50
    assert (~s1["hit"]).any(), "no miss after a bounce"
    ended, followed = ref.per_sample(8)
    mixed = (followed.max(axis=2) != followed.min(axis=2)).sum()
    assert mixed > 0, "no pixels with a mix of path lengths"
    assert followed.max() >= 3 and len(ref.seg) >= 4
    print("unit prediction: segments per level", [int(s["traced"].sum()) for s in ref.seg], "mixed pixels", int(mixed))


@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("n", [64, 128])
def test_unit_scene_all_planes_and_counters(n, K):
    """case 2: the leading 64 samples are one chunk, 128 two (the sums carry in LDS)"""
    ref, desc, g, keep = _unit_paths()
    want, cnt = ref.planes(n, K)
    assert want["bounces"].max() > 0.5 and (want["bounces"] == 0).any()
    if K == 1:   # samples that end on the glass they are still inside of
        assert (want["shape"] == GLASS_SPHERE).any()
    scene = dt.Scene(desc, g)
    try:
        got, st = _device(scene, g, 0, n, K)
    finally:
        scene.close()
    compare(got, want, "unit %d spp, %d bounces" % (n, K))
    _check_stats(st, cnt, 24 * 16, n)
    assert st.rays > st.samples


def test_pixels_per_wave_layout():
    """case 3: 16 spp, four pixels per wave"""
    desc, g, keep = _unit(16)
    ref = PathRef(desc, g).trace(g, 0, 16, 2)
    want, cnt = ref.planes(16, 2)
    assert want["bounces"].max() > 0.5 and cnt["rays"] > 24 * 16 * 16
    scene = dt.Scene(desc, g)
    try:
        got, st = _device(scene, g, 0, 16, 2)
    finally:
        scene.close()
    compare(got, want, "unit 16 spp, 2 bounces")
    _check_stats(st, cnt, 24 * 16, 16)


@pytest.mark.parametrize("K", [2, 1])
def test_final_frame_mirrors_show_texels_borders_and_checkers(K):
    """case 4: final(240) with nogloss = 1: the textured floor, the doors and the checker cylinder are mirrors.
    At max_bounces = 2 the guide rays reach texels, borders and checker squares after a bounce (segment 1), but
    every surface that carries them is itself a mirror, so the ray goes on and no path of this room ends on one
    at segment 2 (the prediction counts tex_fetches = 0 from seven eyes tried); at max_bounces = 1 those hits are
    the paths' ends, and tex_fetches > 0 is asserted there."""
    ref, built, g = _final_paths(1)
    want, cnt = ref.planes(64, K)
    s1 = ref.seg[1]
    assert s1["tex"].sum() > 0 and s1["border"].sum() > 0 and s1["checker"].sum() > 0, "not reached after a bounce"
    if K == 1:
        assert cnt["tex_fetches"] > 0
    scene = dt.Scene(built, g)
    try:
        got, st = _device(scene, g, 240, 64, K)
    finally:
        scene.close()
    compare(got, want, "final(240) nogloss, %d bounces" % K)
    _check_stats(st, cnt, 40 * 24, 64)
    assert st.tex_fetches > 0 or K == 2
    if K == 1:
        return
    # with nogloss = 0 the same shapes are glossy: they stop the chain
    ref0, built0, g0 = _final_paths(0)
    mirrors = np.unique(ref.seg[0]["shape"][ref.seg[0]["hit"] & (ref.seg[0]["code"] != STOP)])
    assert mirrors.size > 0
    s0 = ref0.seg[0]
    on_them = s0["hit"] & np.isin(s0["shape"], mirrors)
    assert on_them.any() and (s0["code"][on_them] == STOP).all()
    want0, cnt0 = ref0.planes(64, 2)
    scene = dt.Scene(built0, g0)
    try:
        got0, st0 = _device(scene, g0, 240, 64, 2)
    finally:
        scene.close()
    compare(got0, want0, "final(240) gloss, 2 bounces")
    # pixels whose every first hit is on one of those shapes
    on_all = on_them.reshape(24, 40, 64).all(axis=2)
    assert on_all.any() and (got0["bounces"][on_all] == 0).all()
    assert (got["bounces"][on_all] > 0).any()


@pytest.mark.parametrize("layout", [dt.DT_OUT_IMAGE, dt.DT_OUT_SLAB], ids=["image", "slab"])
def test_tile_share_host_and_device_arrays(layout):
    """case 5: world = 2, rank = 1: its own pixels hold the full-frame call's values, nothing else is written,
    and host arrays come back as device arrays do"""
    desc, g, keep = _unit(64)
    scene = dt.Scene(desc, g)
    try:
        full = {k: v.cpu().numpy() for k, v in dt.render_features(scene, g, 0, planes=PLANES, specular_bounces=2).items()}
        tile = dt.tiles(tile_w=8, tile_h=8, rank=1, world=2, layout=layout)
        n3 = dt.accum_doubles(g, tile)
        size = {k: n3 if k in ("albedo", "normal") else n3 // 3 for k in PLANES}
        dev = {k: (torch.full((size[k],), -77, dtype=torch.int32, device="cuda") if k == "shape" else
                   torch.full((size[k],), -77.0, device="cuda")) for k in PLANES}
        host = {k: np.full(size[k], -77, np.int32 if k == "shape" else np.float32) for k in PLANES}
        sd, sh = dt.Stats(), dt.Stats()
        dt.render_features(scene, g, 0, tile=tile, out=dev, stats=sd, specular_bounces=2)
        dt.render_features(scene, g, 0, tile=tile, out=host, stats=sh, specular_bounces=2)
    finally:
        scene.close()
    dev = {k: v.cpu().numpy() for k, v in dev.items()}
    W, H = 24, 16
    tiles_x, n_tiles = 3, 6
    own_q, own_px = [], []
    for slot in range((n_tiles + 1) // 2):
        h = (slot * 2654435761) & 0xFFFFFFFF   # dt_scene_dev.h tile_of
        h ^= h >> 15
        h = (h * 0x2c1b3c6d) & 0xFFFFFFFF
        h ^= h >> 12
        t = slot * 2 + (1 + h % 2) % 2
        if t >= n_tiles:
            continue
        ty, tx = divmod(t, tiles_x)
        for py in range(8):
            for px in range(8):
                e = (H - 1 - (ty * 8 + py)) * W + tx * 8 + px
                own_px.append(e)
                own_q.append(e if layout == dt.DT_OUT_IMAGE else slot * 64 + py * 8 + px)
    own_q, own_px = np.array(own_q), np.array(own_px)
    assert sd.pixels == sh.pixels == own_q.size and sd.rays == sh.rays > sd.samples
    for k in PLANES:
        three = k in ("albedo", "normal")
        a, b = (dev[k].reshape(-1, 3), host[k].reshape(-1, 3)) if three else (dev[k], host[k])
        f = full[k].reshape(-1, 3) if three else full[k]
        assert not G.differs(a[own_q], f[own_px]).any(), k
        assert not G.differs(dev[k], host[k]).any(), k
        rest = np.ones(len(a), bool)
        rest[own_q] = False
        assert (a[rest] == -77).all() and (b[rest] == -77).all(), k
    assert (full["bounces"][own_px] > 0).any()


def test_a_render_before_and_after_is_the_same_bytes():
    """case 6"""
    desc, g, keep = _unit(64)
    g.antialias_samples, g.max_depth = 4, 3
    scene = dt.Scene(desc, g)
    try:
        a = torch.zeros(3 * 24 * 16, device="cuda")
        b = torch.zeros_like(a)
        dt.render(scene, g, 0, a)
        f = dt.render_features(scene, g, 0, planes=("bounces",), specular_bounces=8)
        st = dt.render(scene, g, 0, b)
    finally:
        scene.close()
    assert (f["bounces"] > 0).any()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and st.pixels == 24 * 16


def test_denoise_takes_path_guides_as_they_are():
    """case 7: drop-in: denoise(g, colour, path_feats) is tests/denoise_ref.py on the same planes"""
    g, built = _final(240, 40, 24, 64, nogloss=1)
    scene = dt.Scene(built, g)
    try:
        colour = torch.zeros(3 * 40 * 24, device="cuda")
        dt.render(scene, g, 240, colour)
        first = dt.render_features(scene, g, 240, planes=("albedo", "normal", "depth"))
        feats = dt.render_features(scene, g, 240, planes=("albedo", "normal", "depth"), specular_bounces=2)
        clean = dt.denoise(g, colour, feats).cpu().numpy()
        prog = dt.Progressive(scene, g, 240)
        prog.step()
        pf = prog.features(planes=("depth", "bounces"), specular_bounces=2)
    finally:
        scene.close()
    assert not torch.equal(first["depth"], feats["depth"])   # the guides are other guides
    assert torch.equal(pf["depth"].view(torch.int32), feats["depth"].view(torch.int32)) and (pf["bounces"] > 0).any()
    want = denoise_ref_params(40, 24, colour.cpu().numpy(), {k: v.cpu().numpy() for k, v in feats.items()},
                              dt.denoise_params_default())
    assert np.array_equal(clean.view(np.uint32), want.view(np.uint32))


def test_prismcyl_scene_is_unsupported():
    g = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, g)
    g.xRes, g.yRes, g.antialias_samples = 16, 12, 4
    scene = dt.Scene(built, g)
    try:
        with pytest.raises(dt.DTError, match=r"dt_render_features_path failed \(-4\): dt_render_features_path: .*RectPrismWithCylinder"):
            dt.render_features(scene, g, 30, specular_bounces=2)
    finally:
        scene.close()


def test_cli_guide_bounces(tmp_path):
    """case 8: dtrender final 30 --nogloss --features P --guide-bounces 2 at 40x24, 16 spp (case 4's scene: the
    mirrors of final need nogloss): the PNGs are the Python path planes
    through the CLI's formulas; without the flag the files are those of render_features; the frame file is the
    same bytes either way"""
    common = [DTRENDER, "final", "30", "--res", "40x24", "--spp", "16", "--depth", "2", "--nogloss"]
    plain, with_f, with_g = str(tmp_path / "plain.png"), str(tmp_path / "feat.png"), str(tmp_path / "guide.png")
    pf, pg = str(tmp_path / "F"), str(tmp_path / "G")
    subprocess.run(common + ["--out", plain], check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run(common + ["--out", with_f, "--features", pf], check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run(common + ["--out", with_g, "--features", pg, "--guide-bounces", "2"], check=True, timeout=120,
                   stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_f, "rb").read() == open(with_g, "rb").read()
    bad = subprocess.run(common + ["--guide-bounces", "9"], timeout=120, capture_output=True)
    assert bad.returncode == 2 and b"--guide-bounces" in bad.stderr
    g = dt.globals_default()   # the CLI's globals: defaults, no models, buildFinal(240), then the options
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth, g.nogloss = 40, 24, 16, 2, 1
    scene = dt.Scene(built, g)
    names = ("albedo", "normal", "depth", "coverage")
    try:
        first = dt.render_features(scene, g, 240, planes=names)
        path = dt.render_features(scene, g, 240, planes=names + ("bounces",), specular_bounces=2)
    finally:
        scene.close()
    assert (path.pop("bounces") > 0).any()
    differ = 0
    for prefix, feats in ((pf, first), (pg, path)):
        for name, v in dt.feature_images(g, {k: t.cpu().numpy() for k, t in feats.items()}).items():
            png = _read_png("%s.%s.png" % (prefix, name))
            assert png.shape == (24, 40, 3)
            assert np.array_equal(png.reshape(-1), v.astype(np.uint8)), (prefix, name)
            if prefix == pg:
                differ += int(not np.array_equal(png, _read_png("%s.%s.png" % (pf, name))))
    assert differ > 0, "the path images are the first-hit images"
