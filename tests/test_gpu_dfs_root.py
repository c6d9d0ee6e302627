"""The DFS root outside the stack (dt_kernels.hip run_pass): a sample's root node is no stack entry. Its
ray and origin wait in the nrec rows of the wave's LDS until the first DFS step, which is the root step
for the whole wave; the root's FINISH entry takes slot 0 and its children start at slot 1, as when the
root was pushed to slot 0 and popped at once. The cases are the smallest shapes at which that can go
wrong, each against the oracle with equal rays and shadow rays:

  * max_depth 1 (the root is the only node) and 0 (no root: the empty-pass image);
  * max_depth 2 and 4 below glass, mirror and glossy children, brdf_samples 2, depth of field on;
  * a camera that looks past the scene: whole waves of roots miss, the rows are never parked, and the
    next item's roots follow in the same rows;
  * several pixels per wave with idle lanes (4 and 16 spp at a width that is no multiple of the pixels
    per wave; a rank's slab of a 3-way tile split with partial tiles);
  * several passes over the same LDS: 256 spp as chunk items and as per-pixel items on a 16x8 window, and
    a motion-blur frame (several passes per sample);
  * the RectPrismWithCylinder build, which the common scenes do not launch;
  * the window and adaptive-window builds, bit for bit against the plain render of the same samples.
"""
import functools

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
import scene_gen as sg
from parity_check import assert_parity, log_equal

pytestmark = pytest.mark.gpu


def _floats(g, tile):
    return dt.slab_floats(g, tile) if tile.layout == dt.DT_OUT_SLAB else 3 * g.xRes * g.yRes


def _render(desc, g, frame, tile):
    n = _floats(g, tile)
    scene = dt.Scene(desc, g)
    try:
        out = torch.zeros(max(n, 1), dtype=torch.float32, device="cuda")
        st = dt.render(scene, g, frame, out, tile)
        return out.cpu().numpy()[:n], st
    finally:
        scene.close()


def _oracle(desc, g, frame, tile):
    n = _floats(g, tile)
    ref, rst = oracle.render(desc, g, frame, tile, out=np.zeros(max(n, 1), dtype=np.float32))
    return ref[:n], rst


def _check(label, desc, g, frame, tile, nan_ok=False):
    gpu, st = _render(desc, g, frame, tile)
    ref, rst = _oracle(desc, g, frame, tile)
    print("%s: pixels %d samples %d rays %d/%d shadow %d/%d" % (label, st.pixels, st.samples, st.rays, rst.rays,
                                                                 st.shadow_rays, rst.shadow_rays))
    assert st.pixels == rst.pixels and st.samples == rst.samples
    assert st.rays == rst.rays and st.shadow_rays == rst.shadow_rays
    assert st.stack_overflows == rst.stack_overflows == 0
    assert_parity("dfs root: " + label, gpu, ref, nan_ok=nan_ok)
    return gpu, ref, st


def _features(depth, spp=64, res=(48, 32)):
    """scene_gen's features family (glass, mirror, sphere light; brdf_samples 2, aperture 0.1)"""
    desc, g, keep, frame = sg.build("features", "unit")
    g.xRes, g.yRes = res
    g.antialias_samples, g.max_depth = spp, depth
    assert g.brdf_samples == 2 and g.aperture > 0
    return desc, g, keep, frame


@pytest.mark.parametrize("depth", [1, 0, 2, 4])
def test_depth(cuda, depth):
    """Depth 1: every sample is its root alone (no children: rays == samples). Depth 0: no root, every
    pass is empty. Depths 2 and 4: the root's FINISH entry in slot 0 under refraction, mirror and glossy
    children. 48x32 at 64 spp, the 5-wave build; the glass sphere's NaN pixels (Q25) must coincide."""
    desc, g, keep, frame = _features(depth)
    gpu, ref, st = _check("features depth %d" % depth, desc, g, frame, dt.tiles(), nan_ok=True)
    if depth == 0:
        assert st.rays == 0 and st.shadow_rays == 0
        assert np.ptp(ref) == 0   # the empty-pass image: one colour
    elif depth == 1:
        assert st.rays == st.samples and st.shadow_rays > 0
    else:
        assert st.rays > st.samples


def test_whole_waves_miss(cuda):
    """The features camera turned to the floor's back corner: about two thirds of the pixels, whole rows
    among them, see nothing (a wave is a pixel at 64 spp, so whole waves of roots miss and park nothing);
    the rest see the floor, the triangle and the mirror sphere."""
    desc, g, keep, frame = _features(4)
    g.lookingAt[0], g.lookingAt[1], g.lookingAt[2] = -3.0, 0.8, -3.0
    gpu, ref, st = _check("features looking past the scene", desc, g, frame, dt.tiles(), nan_ok=True)
    img = ref.reshape(g.yRes, g.xRes, 3)
    miss = (img == img[0, 0]).all(axis=2)   # the miss colour (image row 0 is the top)
    assert miss[0].all() and miss.all(axis=1).sum() >= 8 and 0.5 < miss.mean() < 0.8
    assert st.rays > st.samples and st.shadow_rays > 0   # the others hit, shade and reflect


@pytest.mark.parametrize("spp", [4, 16])
def test_pixels_per_wave(cuda, spp):
    """16 and 4 pixels per wave (4-wave builds) at 50x30: the last item of the frame has idle lanes, and
    a wave's pixels mix hits, misses and depths."""
    desc, g, keep, frame = _features(4, spp, (50, 30))
    _check("features 50x30 %d spp" % spp, desc, g, frame, dt.tiles(), nan_ok=True)


def test_slab_with_partial_tiles(cuda):
    """Rank 2's slab of a 3-way split of 50x30 in 8x8 tiles (partial tiles at the right and bottom
    edges: lanes of owned items without a pixel), 4 spp."""
    desc, g, keep, frame = _features(4, 4, (50, 30))
    tile = dt.tiles(tile_w=8, tile_h=8, rank=2, world=3, layout=dt.DT_OUT_SLAB)
    gpu, ref, st = _check("features 50x30 4 spp, slab 2/3", desc, g, frame, tile, nan_ok=True)
    assert st.pixels == 448 and st.rays > st.samples


def test_chunks_over_the_same_rows(cuda, monkeypatch):
    """256 spp on a 16x8 window: four chunks per pixel, as chunk items (an item per chunk) and as
    per-pixel items (one wave runs its pixel's four passes over the same rows, red in between)."""
    desc, g, keep, frame = _features(4, 256)
    tile = dt.tiles(x0=16, y0=10, x1=32, y1=18)
    monkeypatch.setenv("DT_CHUNK_ITEMS", "1")
    chunked, ref, st = _check("features 256 spp, chunk items", desc, g, frame, tile, nan_ok=True)
    assert st.samples == 16 * 8 * 256
    monkeypatch.setenv("DT_CHUNK_ITEMS", "0")
    whole, ref, st = _check("features 256 spp, per-pixel items", desc, g, frame, tile, nan_ok=True)
    log_equal("dfs root: 256 spp chunk items vs per-pixel items", chunked.view(np.uint32), whole.view(np.uint32))


def test_blur_passes(cuda):
    """The motion family at its blur frame (the blur build): samples that end on a moving shape run
    blur_samples more passes, each with a root of its own in the same rows."""
    desc, g, keep, frame = sg.build("motion-small", "unit")
    assert frame == sg.MOTION_FRAME
    g.xRes, g.yRes, g.antialias_samples = 48, 32, 64
    gpu, ref, st = _check("motion frame %d" % frame, desc, g, frame, dt.tiles())
    assert st.rays > 2 * st.samples   # the re-traces ran


def test_prismcyl_build(cuda):
    """One frame of the prismcyl scene (the RectPrismWithCylinder build) from an oblique eye, 48x32."""
    g = dt.globals_default()
    built = dt.build_scene("prismcyl", 0, g)
    g.xRes, g.yRes = 48, 32
    g.eye[0], g.eye[1], g.eye[2] = -5.0, 1.3, 2.2
    gpu, ref, st = _check("prismcyl oblique", built, g, 0, dt.tiles())
    assert ref.max() > 0


@functools.lru_cache(maxsize=None)
def _room_plain():
    """The room family at 48x32, 144 spp (windows of 64, 64 and 16 samples), rendered in one go"""
    desc, g, keep, frame = sg.build("room", "unit")
    g.xRes, g.yRes, g.antialias_samples = 48, 32, 144
    gpu, ref, st = _check("room 144 spp", desc, g, frame, dt.tiles())
    return desc, g, keep, frame, gpu


@pytest.mark.parametrize("adaptive", [False, True], ids=["window", "adaptive-window"])
def test_window_builds(cuda, adaptive):
    """The same samples through the *_win and *_awin builds, a 64-sample window at a time, against the
    plain render bit for bit. (Adaptive with min_samples = spp: no pixel may stop early, so every pixel
    is the mean of all its samples.)"""
    desc, g, keep, frame, plain = _room_plain()
    scene = dt.Scene(desc, g)
    try:
        p = dt.AdaptiveProgressive(scene, g, frame, tol=0.0, min_samples=144) if adaptive else dt.Progressive(scene, g, frame)
        steps = 0
        while not p.done:
            st = p.step()
            assert st.stack_overflows == 0
            steps += 1
        assert steps == 3 and p.samples_done == 144
        img = p.image().cpu().numpy()[:plain.size]
    finally:
        scene.close()
    log_equal("dfs root: room 144 spp %s vs plain render" % ("adaptive windows" if adaptive else "windows"),
              img.view(np.uint32), plain.view(np.uint32))
