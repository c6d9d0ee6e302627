"""Progressive rendering: sample windows into a resident f64 accumulator (include/dt.h dt_render_window
and dt_resolve, dt_kernels.hip DT_WINDOW, distraytracer_amd.Progressive).

A sample's colour depends only on (seed, frame, pixel, sample index) and the per-pixel sum is a
left-to-right chain of f64 adds in sample order (render_final_project.cpp:1062-1213: `color +=
tmp_color` per sample, then `/= sampled_n`), so windows applied in ascending order to a zeroed
accumulator must reproduce the one-shot render's bits: every comparison below is bit for bit
(log_equal) against dt.render, and at zero tolerance (assert_parity tol=0) against the oracle where
the one-shot render is. The cases are the paths of the item loop a window launch takes: the sky-item
relaunch, partial last chunks, several pixels per wave, motion-blur passes, the feature builds, the
RectPrismWithCylinder and work-sharing builds, slab shares, and state carried across scenes.
"""
import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
from parity_check import assert_parity, log_equal

pytestmark = pytest.mark.gpu


def _n_out(g, tile):
    return dt.slab_floats(g, tile) if tile.layout == dt.DT_OUT_SLAB else 3 * g.xRes * g.yRes


def _one_shot(scene, g, frame, tile):
    n = _n_out(g, tile)
    out = torch.zeros(max(n, 1), dtype=torch.float32, device="cuda")
    st = dt.render(scene, g, frame, out, tile)
    return out.cpu().numpy()[:n], st


def _oracle(built, g, frame, tile):
    n = _n_out(g, tile)
    ref, rst = oracle.render(built, g, frame, tile, out=np.zeros(max(n, 1), dtype=np.float32))
    return ref[:n], rst


def _windows(scene, g, frame, tile, chunks=None):
    """A fresh Progressive stepped to the end: `chunks` 64-sample chunks per step (a list), or one
    per step. Returns (resolved image, the windows' stats, the Progressive)."""
    p = dt.Progressive(scene, g, frame, tile)
    stats = []
    if chunks is None:
        while not p.done:
            stats.append(p.step())
    else:
        for c in chunks:
            stats.append(p.step(c))
    assert p.done and p.samples_done == p.spp
    return p.image().cpu().numpy()[:_n_out(g, tile)], stats, p


def _check_sums(stats, st, label):
    """the windows' counts add up to the one-shot render's"""
    for k in ("rays", "shadow_rays", "samples", "tex_fetches"):
        assert sum(getattr(s, k) for s in stats) == getattr(st, k), (label, k)
    assert all(s.pixels == st.pixels and s.stack_overflows == 0 for s in stats), label


def _spheres(aa, w=40, h=24, depth=3, cloud=1):
    g = dt.globals_default()
    built = dt.build_scene("spheres", 0, g)
    g.perlin_cloud = cloud
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = w, h, aa, depth
    return g, built


@pytest.fixture(scope="module")
def spheres256(cuda):
    """The spheres scene with clouds, 40x24, 256 spp, depth 3: its one-shot render and oracle image,
    shared by the tests that run windows over it (never modified)."""
    g, built = _spheres(256)
    tile = dt.tiles()
    scene = dt.Scene(built, g)
    img, st = _one_shot(scene, g, 0, tile)
    scene.close()
    ref, rst = _oracle(built, g, 0, tile)
    assert st.rays == rst.rays and st.shadow_rays == rst.shadow_rays
    assert_parity("spheres sky aa=256 one-shot vs oracle", img, ref)
    img.setflags(write=False)
    ref.setflags(write=False)
    return g, built, tile, img, st, ref


def test_sky_relaunch(spheres256):
    """Sky around the spheres: the still build lists every item with a missed sample and the *_sky
    build renders the item's window again, storing the accumulator then. Windows [0,64), [64,128),
    [128,256), twice on one scene with a fresh accumulator each time."""
    g, built, tile, one, st, ref = spheres256
    scene = dt.Scene(built, g)
    try:
        for k in range(2):
            img, stats, p = _windows(scene, g, 0, tile, chunks=[1, 1, 2])
            print("spheres sky windows #%d: rays %s sky %s" % (k, [s.rays for s in stats], [s.sky_pixels for s in stats]))
            assert [s.samples for s in stats] == [st.pixels * 64, st.pixels * 64, st.pixels * 128]
            _check_sums(stats, st, "spheres sky")
            assert all(s.sky_pixels > 0 for s in stats) and st.sky_pixels > 0
            assert p.nan_pixels == 0
            log_equal("spheres sky aa=256 windows #%d vs one-shot (bits)" % k, img.view(np.uint32), one.view(np.uint32))
            assert_parity("spheres sky aa=256 windows #%d vs oracle" % k, img, ref, tol=0)
    finally:
        scene.close()


def test_partial_last_chunk(cuda):
    """100 spp: windows [0,64) and [64,100), the last chunk holds 36 samples."""
    g, built = _spheres(100)
    tile = dt.tiles()
    scene = dt.Scene(built, g)
    try:
        one, st = _one_shot(scene, g, 0, tile)
        img, stats, _ = _windows(scene, g, 0, tile)
        assert [s.samples for s in stats] == [st.pixels * 64, st.pixels * 36]
        _check_sums(stats, st, "spheres aa=100")
        log_equal("spheres sky aa=100 windows vs one-shot (bits)", img.view(np.uint32), one.view(np.uint32))
    finally:
        scene.close()
    ref, rst = _oracle(built, g, 0, tile)
    assert_parity("spheres sky aa=100 windows vs oracle", img, ref, tol=0)


def test_prefix_pinned_to_oracle(cuda):
    """The window [0,64) of a 144-spp frame alone: each accumulator double is the left-to-right f64 sum
    of the oracle's colours of samples 0..63 of its pixel, exactly, and image() is
    clamp(float32(sum / 64)) * 255 -- for 24 pixels, some whose samples hit a sphere and some whose
    samples miss (the sky)."""
    g, built = _spheres(144, 16, 12, 2)
    scene = dt.Scene(built, g)
    try:
        p = dt.Progressive(scene, g, 0)
        st = p.step()
        assert p.samples_done == 64 and not p.done and st.samples == 16 * 12 * 64
        acc = p.accum.cpu().numpy()
        img = p.image().cpu().numpy()
    finally:
        scene.close()
    # 12 pixels whose sample 0 hits and 12 whose sample 0 misses, spread over the frame
    kind = {(x, y): oracle.sample_color(built, g, 0, x, y, 0)[1] for y in range(12) for x in range(16)}
    hits = [q for q in sorted(kind) if kind[q]]
    misses = [q for q in sorted(kind) if not kind[q]]
    assert hits and misses, "the frame must hold sphere pixels and sky pixels"
    n_miss = min(12, len(misses))
    n_hit = min(24 - n_miss, len(hits))
    n_miss = min(24 - n_hit, len(misses))
    pixels = [hits[(i * len(hits)) // n_hit] for i in range(n_hit)]
    pixels += [misses[(i * len(misses)) // n_miss] for i in range(n_miss)]
    assert len(pixels) == 24 and len(set(pixels)) == 24
    n_hit_samples = n_miss_samples = 0
    for (x, y) in pixels:
        s = np.zeros(3, dtype=np.float64)
        for i in range(64):
            col, hit = oracle.sample_color(built, g, 0, x, y, i)
            s = s + np.array(col, dtype=np.float64)   # componentwise, in sample order
            n_hit_samples += hit
            n_miss_samples += not hit
        off = 3 * ((g.yRes - 1 - y) * g.xRes + x)
        got = acc[off:off + 3]
        print("pixel (%d,%d): accum %s oracle sum %s" % (x, y, got, s))
        assert np.array_equal(got.view(np.uint64), s.view(np.uint64)), (x, y, got, s)
        want = np.clip(np.float32(s / 64), np.float32(0), np.float32(1)) * np.float32(255)
        assert np.array_equal(img[off:off + 3].view(np.uint32), want.view(np.uint32)), (x, y)
    assert n_hit_samples > 0 and n_miss_samples > 0


def _final(frame, models, w, h, aa, depth):
    g = dt.globals_default()
    g.use_model = models
    built = dt.build_scene("final", frame, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = w, h, aa, depth
    return g, built


def _product_case(label, g, built, frame, tile, kernel=None):
    scene = dt.Scene(built, g)
    if kernel is not None:
        scene.set_kernel(kernel)
    try:
        one, st = _one_shot(scene, g, frame, tile)
        img, stats, _ = _windows(scene, g, frame, tile)
        print("%s: pixels=%d rays=%d windows=%d" % (label, st.pixels, st.rays, len(stats)))
        _check_sums(stats, st, label)
        log_equal("%s one-chunk windows vs one-shot (bits)" % label, img.view(np.uint32), one.view(np.uint32))
    finally:
        scene.close()
    ref, rst = _oracle(built, g, frame, tile)
    assert st.rays == rst.rays and st.shadow_rays == rst.shadow_rays
    assert_parity("%s one-chunk windows vs oracle" % label, img, ref, tol=0)
    return st, img


@pytest.mark.parametrize("models", [0, 1])
def test_room_and_mesh_builds(cuda, models):
    """buildFinal(240) without and with the OBJ models (the room and mesh builds, 5 waves), 1920x1080,
    256 spp, depth 4, rank 1's slab of a 1024-way split in 16x16 tiles: four one-chunk windows."""
    g, built = _final(240, models, 1920, 1080, 256, 4)
    tile = dt.tiles(tile_w=16, tile_h=16, rank=1, world=1024, layout=dt.DT_OUT_SLAB)
    st, _ = _product_case("final(240) models=%d aa=256 1/1024" % models, g, built, 240, tile)
    assert st.samples == st.pixels * 256


def test_tunnel_blur_build(cuda):
    """The tunnel frame buildFinal(1200) (motion-blur passes, the tunnel build), 960x540, 100 spp,
    depth 4, rank 2 of 256."""
    g, built = _final(1200, 0, 960, 540, 100, 4)
    tile = dt.tiles(tile_w=16, tile_h=16, rank=2, world=256, layout=dt.DT_OUT_SLAB)
    st, _ = _product_case("tunnel 1200 aa=100 1/256", g, built, 1200, tile)
    assert st.rays > st.samples


def test_prismcyl_build(cuda):
    """BuildScenePrismCylinder: the RectPrismWithCylinder build, 40x24 at 100 spp, from an oblique eye
    (frame 0's own camera looks down the hole's axis: a black frame, tests/test_host.py)."""
    g = dt.globals_default()
    built = dt.build_scene("prismcyl", 0, g)
    g.xRes, g.yRes, g.antialias_samples = 40, 24, 100
    g.eye[0], g.eye[1], g.eye[2] = -5.0, 1.3, 2.2
    st, img = _product_case("prismcyl aa=100 oblique", g, built, 0, dt.tiles())
    assert img.max() > 0


def test_donate_build(spheres256):
    """The work-sharing build (dt_scene_set_kernel DT_KERNEL_DONATE) on the spheres scene with clouds."""
    g, built, tile, one, st, ref = spheres256
    scene = dt.Scene(built, g)
    scene.set_kernel(dt.DT_KERNEL_DONATE)
    try:
        img, stats, _ = _windows(scene, g, 0, tile)
        assert len(stats) == 4
        _check_sums(stats, st, "spheres donate")
        log_equal("spheres sky aa=256 work-sharing windows vs one-shot (bits)", img.view(np.uint32), one.view(np.uint32))
        assert_parity("spheres sky aa=256 work-sharing windows vs oracle", img, ref, tol=0)
    finally:
        scene.close()


@pytest.mark.parametrize("aa", [16, 1])
def test_spp_below_64(cuda, aa):
    """spp < 64: the single window [0, spp). 16 spp: four pixels per wave; 1 spp with clouds: 64
    pixels per wave, where the one-shot render defers the sky to dt_sky_miss_kernel and the window
    launch computes it in the sky-item launch."""
    g, built = _spheres(aa)
    tile = dt.tiles()
    scene = dt.Scene(built, g)
    try:
        one, st = _one_shot(scene, g, 0, tile)
        img, stats, p = _windows(scene, g, 0, tile)
        assert len(stats) == 1 and stats[0].samples == st.samples == st.pixels * aa
        assert stats[0].rays == st.rays and stats[0].shadow_rays == st.shadow_rays
        assert stats[0].sky_pixels > 0 and st.sky_pixels > 0
        log_equal("spheres sky aa=%d single window vs one-shot (bits)" % aa, img.view(np.uint32), one.view(np.uint32))
        with pytest.raises(dt.DTError):
            p.step()
    finally:
        scene.close()


def test_two_tile_shares(cuda):
    """A 40x24 frame split over two ranks in 8x8 tiles (DT_OUT_SLAB): each rank stepped in this
    process, resolved into its slab, the slabs unpacked with dt_unpack_slabs: the whole-frame
    one-shot render."""
    g, built = _spheres(256)
    scene = dt.Scene(built, g)
    try:
        one, st = _one_shot(scene, g, 0, dt.tiles())
        t0 = dt.tiles(tile_w=8, tile_h=8, rank=0, world=2, layout=dt.DT_OUT_SLAB)
        per = dt.slab_floats_max(g, t0)
        slabs = torch.zeros(2 * per, dtype=torch.float32, device="cuda")
        for r in range(2):
            tile = dt.tiles(tile_w=8, tile_h=8, rank=r, world=2, layout=dt.DT_OUT_SLAB)
            assert dt.accum_doubles(g, tile) == dt.slab_floats(g, tile) <= per
            p = dt.Progressive(scene, g, 0, tile).run()
            assert p.done
            p.image(out=slabs[r * per:r * per + p.accum.numel()])
        image = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        dt.unpack_slabs(g, t0, 2, slabs, image)
        log_equal("spheres sky aa=256 two slab shares, windows vs whole-frame one-shot (bits)",
                  image.cpu().numpy().view(np.uint32), one.view(np.uint32))
    finally:
        scene.close()


def test_resume_across_scenes(spheres256):
    """state() after 64 of 256 samples, the scene closed; a new scene and Progressive.restore run to
    the end: the one-shot image. A changed seed or resolution is refused."""
    g, built, tile, one, st, ref = spheres256
    scene = dt.Scene(built, g)
    p = dt.Progressive(scene, g, 0)
    p.step()
    state = p.state()
    scene.close()
    del p
    assert state["samples_done"] == 64 and state["spp"] == 256 and state["accum"].dtype == np.float64
    assert (state["xRes"], state["yRes"], state["frame"], state["seed"]) == (40, 24, 0, g.seed)
    scene2 = dt.Scene(built, g)
    try:
        q = dt.Progressive.restore(scene2, g, state)
        assert q.samples_done == 64 and not q.done
        changes = []
        prev = [q.image()]

        def until(pr):   # the early-stop measure, in torch: never true here, only recorded
            cur = pr.image()
            changes.append(dt.mean_abs_change(cur, prev[0]))
            prev[0] = cur
            return False
        q.run(until=until)
        assert q.done and len(changes) == 3 and all(c >= 0 for c in changes)
        log_equal("spheres sky aa=256 resumed after 64 samples vs one-shot (bits)",
                  q.image().cpu().numpy().view(np.uint32), one.view(np.uint32))
        g_seed = g.copy()
        g_seed.seed = g.seed + 1
        with pytest.raises(dt.DTError, match="seed"):
            dt.Progressive.restore(scene2, g_seed, state)
        g_res = g.copy()
        g_res.xRes = 48
        with pytest.raises(dt.DTError, match="xRes"):
            dt.Progressive.restore(scene2, g_res, state)
    finally:
        scene2.close()


def test_device_resolve_matches_host_resolve(spheres256):
    """dt_resolve_kernel against dt_resolve's host loop on a rendered accumulator, at every window
    boundary's sample count, and on one with NaN pixels: the same bits, the same NaN count."""
    g, built, tile, one, st, ref = spheres256
    scene = dt.Scene(built, g)
    try:
        p = dt.Progressive(scene, g, 0).run()
    finally:
        scene.close()
    acc_h = p.accum.cpu().numpy()
    for n in (64, 100, 256):
        dev = torch.empty(p.accum.numel(), dtype=torch.float32, device="cuda")
        host = np.empty(acc_h.size, dtype=np.float32)
        assert dt.resolve(g, p.accum, n, dev) == dt.resolve(g, acc_h, n, host) == 0
        log_equal("resolve n=%d device vs host (bits)" % n, dev.cpu().numpy().view(np.uint32), host.view(np.uint32))
    log_equal("resolve n=256 vs one-shot (bits)", host.view(np.uint32), one.view(np.uint32))
    bad = acc_h.copy()
    bad[0] = np.nan                 # pixel 0: one channel
    bad[3 * 70:3 * 70 + 3] = np.nan   # pixel 70 (the second wave): all three
    bad[-1] = np.nan                # the last pixel
    bad[5] = -7.0
    bad[10] = 1e9
    dev = torch.empty(bad.size, dtype=torch.float32, device="cuda")
    host = np.empty(bad.size, dtype=np.float32)
    n_dev = dt.resolve(g, torch.from_numpy(bad).cuda(), 256, dev)
    n_host = dt.resolve(g, bad, 256, host)
    assert n_dev == n_host == 3
    log_equal("resolve with NaN pixels device vs host (bits)", dev.cpu().numpy().view(np.uint32), host.view(np.uint32))
