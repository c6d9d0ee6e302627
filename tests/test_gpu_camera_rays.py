"""Camera rays as arrays and their way back to pixels on the device (include/dt.h dt_camera_rays, dt_rays_resolve;
dt_camera_rays_kernel, dt_rays_resolve_kernel), bit for bit against the oracle's or_primary_ray, the project's own
dt_intersect_primary and dt_render_features, and the numpy restatement of tests/camera_rays_ref.py.

Frames: final at 70x37 and spheres at 33x20, neither a multiple of 32 or 64, so the last tile and the last wave
are partial; aperture 0 and the scene's own (forced positive where the builder leaves it 0).
All comparisons are by bit pattern (oracle.geom.differs); shape ids as integers."""
import os
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
from oracle import geom as G

import camera_rays_ref as R

from test_gpu_features import DTRENDER, _read_png

pytestmark = pytest.mark.gpu

SIZES = {"final": (70, 37, 240), "spheres": (33, 20, 0)}
RANGES = [(0, 1), (5, 13), (64, 66)]   # (5, 13) crosses the 8-sample block of the oracle's numbering
SENTINEL = -12345.0


def _scene(name, aperture, aa=9, **kw):
    """(g, built, frame): the variant tests/test_gpu_features.py uses (no OBJ models)"""
    W, H, frame = SIZES[name]
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene(name, frame, g)
    g.xRes, g.yRes, g.antialias_samples = W, H, aa
    if aperture == 0:
        g.aperture = 0.0
    elif not g.aperture > 0:
        g.aperture = 0.2
    for k, v in kw.items():
        setattr(g, k, v)
    return g, built, frame


def _shares():
    return [("whole", None), ("image", dt.tiles(tile_w=32, tile_h=32, rank=1, world=2)),
            ("slab", dt.tiles(tile_w=32, tile_h=32, rank=1, world=2, layout=dt.DT_OUT_SLAB))]


_oracle_rays = {}


def _oracle(name, aperture):
    """or_primary_ray's rays 0 .. 9*W*H*8 - 1 (samples 0..71 of every pixel) for the scene's globals, computed once"""
    key = (name, aperture)
    if key not in _oracle_rays:
        g, _, frame = _scene(name, aperture)
        _oracle_rays[key] = G.or_primary_ray(g, frame, 0, 9 * g.xRes * g.yRes * 8)
    return _oracle_rays[key]


def _same(a, b, what):
    bad = np.nonzero(G.differs(a, b))[0]
    print("%s: %d of %d rows differ" % (what, bad.size, len(a)))
    assert bad.size == 0, "%s row %d: device %r, expected %r" % (what, bad[0], a[bad[0]], b[bad[0]])


@pytest.mark.parametrize("aperture", [0, 1], ids=["pinhole", "lens"])
@pytest.mark.parametrize("name", ["final", "spheres"])
def test_rays_equal_the_oracle(name, aperture):
    """whole image and a tile share in both layouts, three sample ranges: owned rows are or_primary_ray's rays
    under dt_intersect_primary's numbering, unowned rows keep the sentinel, host arrays hold the device's bits"""
    g, _, frame = _scene(name, aperture)
    assert (g.aperture > 0) == bool(aperture)
    ostart, odir = _oracle(name, aperture)
    for share, tile in _shares():
        for rng in RANGES:
            ns = rng[1] - rng[0]
            num, own = R.ray_numbers(g, rng, tile)
            slots = dt.accum_doubles(g, tile) // 3
            assert num.shape == (slots, ns) and dt.camera_rays_rows(g, rng, tile) == slots * ns
            assert own.all() if tile is None else (own.any() and not own.all())
            start = torch.full((slots, ns, 3), SENTINEL, dtype=torch.float64, device="cuda")
            dirs = torch.full((slots, ns, 3), SENTINEL, dtype=torch.float64, device="cuda")
            dt.camera_rays(g, frame, samples=rng, tile=tile, out=(start, dirs))
            s, d = start.cpu().numpy(), dirs.cpu().numpy()
            what = "%s %s %s %s" % (name, "lens" if aperture else "pinhole", share, rng)
            want_s = np.where(own[..., None], ostart[num], SENTINEL)
            want_d = np.where(own[..., None], odir[num], SENTINEL)
            _same(s.reshape(-1, 3), want_s.reshape(-1, 3), what + " start")
            _same(d.reshape(-1, 3), want_d.reshape(-1, 3), what + " dir")
            hs, hd = np.full((slots, ns, 3), SENTINEL), np.full((slots, ns, 3), SENTINEL)
            dt.camera_rays(g, frame, samples=rng, tile=tile, out=(hs, hd))
            _same(hs.reshape(-1, 3), s.reshape(-1, 3), what + " host start")
            _same(hd.reshape(-1, 3), d.reshape(-1, 3), what + " host dir")
    # the default arrays: CUDA, zero-filled, so unowned rows are void rays; host=True: numpy, the same bits
    tile = _shares()[2][1]
    s, d = dt.camera_rays(g, frame, samples=(0, 2), tile=tile)
    assert s.is_cuda and s.dtype == torch.float64 and tuple(s.shape) == (dt.accum_doubles(g, tile) // 3, 2, 3)
    _, own = R.ray_numbers(g, (0, 2), tile)
    assert (d.cpu().numpy()[~own] == 0).all() and (d.cpu().numpy()[own] != 0).any(axis=-1).all()
    hs, hd = dt.camera_rays(g, frame, samples=(0, 2), tile=tile, host=True)
    assert isinstance(hs, np.ndarray)
    _same(hs.reshape(-1, 3), s.cpu().numpy().reshape(-1, 3), "host=True start")
    _same(hd.reshape(-1, 3), d.cpu().numpy().reshape(-1, 3), "host=True dir")


@pytest.mark.parametrize("aperture", [0, 1], ids=["pinhole", "lens"])
def test_frame_and_seed_move_the_eye_sample_iff_there_is_a_lens(aperture):
    g, _, frame = _scene("final", aperture)
    s0, d0 = dt.camera_rays(g, frame, samples=(0, 4))
    s1, d1 = dt.camera_rays(g, frame + 1, samples=(0, 4))
    g.seed += 1
    s2, d2 = dt.camera_rays(g, frame, samples=(0, 4))
    for s, d in ((s1, d1), (s2, d2)):
        assert bool(torch.equal(s, s0)) == (not aperture)
        assert bool(torch.equal(d, d0)) == (not aperture)
    if aperture:   # nearly every eye sample moves, not a few
        assert (s1 != s0).any(dim=-1).float().mean() > 0.99 and (s2 != s0).any(dim=-1).float().mean() > 0.99


@pytest.mark.parametrize("name", ["final", "spheres"])
def test_traced_camera_rays_are_intersect_primary(name):
    """trace_rays(camera_rays(samples 0..7)) gives the shape and t of dt_intersect_primary's rays 0 .. W*H*8 - 1"""
    g, built, frame = _scene(name, 1)
    W, H = g.xRes, g.yRes
    scene = dt.Scene(built, g)
    try:
        start, dirs = dt.camera_rays(g, frame, samples=(0, 8))
        hits, _ = dt.trace_rays(scene, g, start.view(-1, 3), dirs.view(-1, 3), planes=("shape", "t"))
        shape = torch.zeros(W * H * 8, dtype=torch.int32, device="cuda")
        t = torch.zeros(W * H * 8, dtype=torch.float32, device="cuda")
        dt.intersect_primary(scene, g, frame, 0, shape, t)
    finally:
        scene.close()
    num, _ = R.ray_numbers(g, (0, 8))
    num = num.reshape(-1)
    got_shape, got_t = hits["shape"].cpu().numpy(), hits["t"].cpu().numpy()
    assert (got_shape >= 0).any()
    _same(got_shape, shape.cpu().numpy()[num], name + " shape")
    _same(got_t, t.cpu().numpy()[num], name + " t")


def _round_trip(scene, g, frame, n, tile):
    start, dirs = dt.camera_rays(g, frame, samples=(0, n), tile=tile)
    hits, _ = dt.trace_rays(scene, g, start.view(-1, 3), dirs.view(-1, 3), planes=("shape", "albedo", "normal"))
    albedo, cov = dt.rays_resolve(g, hits["albedo"], n, shape=hits["shape"], tile=tile, coverage=True)
    normal = dt.rays_resolve(g, hits["normal"], n, shape=hits["shape"], tile=tile)
    return {"albedo": albedo, "normal": normal, "coverage": cov, "shape": hits["shape"].view(-1, n)[:, 0].contiguous()}


@pytest.mark.parametrize("share", ["whole", "slab"])
def test_round_trip_reproduces_render_features(share):
    """camera_rays(samples 0..spp) -> trace_rays(shape, albedo, normal) -> rays_resolve equals render_features'
    albedo, normal and coverage planes, and shape for sample 0: by include/dt.h's definitions, bit for bit"""
    g, built, frame = _scene("final", 1, aa=9)
    n = 9
    tile = dict(_shares())[share]
    scene = dt.Scene(built, g)
    try:
        want = dt.render_features(scene, g, frame, tile=tile, planes=("albedo", "normal", "coverage", "shape"))
        got = _round_trip(scene, g, frame, n, tile)
    finally:
        scene.close()
    cov = want["coverage"].cpu().numpy()
    assert (cov > 0).any()
    for k in ("albedo", "normal", "coverage", "shape"):
        a, b = got[k].cpu().numpy().reshape(-1), want[k].cpu().numpy().reshape(-1)
        _same(a, b, "%s %s" % (share, k))
    if tile is not None:
        _, own = R.ray_numbers(g, (0, 1), tile)
        assert (got["albedo"].cpu().numpy()[~own[:, 0]] == 0).all()


@pytest.mark.parametrize("n", [1, 9, 64])
@pytest.mark.parametrize("width", [1, 3])
def test_device_resolve_equals_the_restatement(n, width):
    """random f64 rows of mixed magnitude, shape with runs of misses; 37x13 pixels is 481 * width elements: the
    last block and the last wave are partial"""
    g = dt.globals_default()
    g.xRes, g.yRes = 37, 13
    slots = 37 * 13
    rng = np.random.default_rng(1000 * n + width)
    v = rng.standard_normal((slots, n, width)) * np.exp(rng.uniform(-12, 12, (slots, n, width)))
    shape = rng.integers(0, 40, (slots, n)).astype(np.int32)
    run = rng.integers(0, n + 1, slots)
    shape[np.arange(n)[None, :] < run[:, None]] = -1   # a leading run of misses per pixel, whole pixels too
    shape[5] = -1
    assert ((shape < 0).all(axis=1)).any()
    vd, sd = torch.from_numpy(v).cuda(), torch.from_numpy(shape).cuda()
    for mode in ("mean", "hit_mean"):
        for sh_h, sh_d in ((None, None), (shape, sd)):
            got, cov = dt.rays_resolve(g, vd, n, shape=sh_d, mode=mode, coverage=True)
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (slots, width)
            want, wcov = R.resolve_ref(v, n, width, shape=sh_h, mode=mode)
            _same(got.cpu().numpy().reshape(-1), want.reshape(-1), "%s shape=%s" % (mode, sh_h is not None))
            _same(cov.cpu().numpy(), wcov, "coverage")
    # a tile share in both layouts: only owned pixels are written
    for _, tile in _shares()[1:]:
        _, _, own = R.slot_pixels(g, tile)
        k = len(own)
        out = torch.full((k, width), SENTINEL, dtype=torch.float32, device="cuda")
        cov = torch.full((k,), SENTINEL, dtype=torch.float32, device="cuda")
        vv = np.resize(v, (k, n, width))
        ss = np.resize(shape, (k, n))
        dt.rays_resolve(g, torch.from_numpy(vv).cuda(), n, shape=torch.from_numpy(ss).cuda(), mode="hit_mean", tile=tile,
                        coverage=True, out=(out, cov))
        want, wcov = R.resolve_ref(vv, n, width, shape=ss, mode="hit_mean", owned=own,
                                   out=np.full((k, width), SENTINEL, np.float32), coverage=np.full(k, SENTINEL, np.float32))
        _same(out.cpu().numpy().reshape(-1), want.reshape(-1), "share plane")
        _same(cov.cpu().numpy(), wcov, "share coverage")


def test_peel_layers():
    """k = 2 on final, one ray per pixel: layer 0 is the round trip's albedo plane; layer 1 is non-zero somewhere
    (behind the panes) and zero wherever trace_rays_multi's count < 2"""
    g, built, frame = _scene("final", 1)
    W, H = g.xRes, g.yRes
    scene = dt.Scene(built, g)
    try:
        layers = dt.peel_layers(scene, g, frame, k=2)
        first = _round_trip(scene, g, frame, 1, None)
        start, dirs = dt.camera_rays(g, frame, samples=(0, 1))
        hits, _ = dt.trace_rays_multi(scene, g, start.view(-1, 3), dirs.view(-1, 3), k=2, planes=("count",))
    finally:
        scene.close()
    assert layers["albedo"].shape == (2, H, W, 3) and layers["coverage"].shape == (2, H, W)
    assert layers["albedo"].dtype == layers["coverage"].dtype == np.float32
    count = hits["count"].cpu().numpy()
    _same(layers["albedo"][0].reshape(-1, 3), first["albedo"].cpu().numpy(), "layer 0 albedo")
    _same(layers["coverage"][0].reshape(-1), first["coverage"].cpu().numpy(), "layer 0 coverage")
    a1, c1 = layers["albedo"][1].reshape(-1, 3), layers["coverage"][1].reshape(-1)
    print("layer 1: %d of %d pixels have a second surface" % (int((count >= 2).sum()), count.size))
    assert (a1 != 0).any() and (count < 2).any()
    assert (a1[count < 2] == 0).all()
    _same(c1, (count >= 2).astype(np.float32), "layer 1 coverage")


def test_cli_peel_images(tmp_path):
    """dtrender final 30 --peel 2 --peel-out P --peel-samples 3 at 40x24: P.layer<j>.png is peel_layers' albedo of
    layer j times 255, and the frame is the file written without the flag"""
    common = [DTRENDER, "final", "30", "--res", "40x24", "--spp", "4", "--depth", "2"]
    plain, with_p, prefix = str(tmp_path / "plain.png"), str(tmp_path / "peel.png"), str(tmp_path / "P")
    subprocess.run(common + ["--out", plain], check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run(common + ["--out", with_p, "--peel", "2", "--peel-out", prefix, "--peel-samples", "3"], check=True,
                   timeout=120, stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_p, "rb").read()
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("P.")) == ["P.layer0.png", "P.layer1.png"]
    bad = subprocess.run(common + ["--out", plain, "--peel", "9", "--peel-out", prefix], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode == 2 and "usage: --peel" in bad.stderr
    # the CLI's globals: defaults, no models, buildFinal(240), then the options
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = 40, 24, 4, 2
    scene = dt.Scene(built, g)
    try:
        layers = dt.peel_layers(scene, g, 240, k=2, n_samples=3)
    finally:
        scene.close()
    for j in range(2):
        png = _read_png("%s.layer%d.png" % (prefix, j))
        want = np.clip(layers["albedo"][j] * np.float32(255), 0, 255).astype(np.uint8)
        assert png.shape == (24, 40, 3) and np.array_equal(png, want), j
    assert _read_png(prefix + ".layer1.png").any()
