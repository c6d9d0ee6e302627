"""Path ray queries (include/dt.h dt_trace_rays_path; dt_rayq_path_kernel) against the prediction of
tests/raypath_ref.py, made on the CPU from PathRef._segment and bounce_rule alone, bit for bit.

Every comparison is by bit pattern (oracle.geom.differs for floating-point planes, integers as integers). The
scene is the 24x16 "unit" scene of tests/test_gpu_features_path.py (a glass and a steel sphere over a checker
floor) with nogloss = 1; the rays are raypath_ref.ray_set(): 64 * 3 camera rays and 17 hand-made ones, a partial
last wave. What the ray set holds is asserted of the prediction in tests/test_raypath_host.py and again, in
short, before the comparison here. One prediction per K, shared and never written to."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import raypath_ref as R
from oracle import geom as G

pytestmark = pytest.mark.gpu

DTRENDER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distraytracer_amd", "dtrender")
COUNTERS = R.COUNTERS
ZERO_COUNTERS = ("pixels", "samples", "shadow_rays", "sky_pixels", "nan_pixels", "stack_overflows", "glossy_exhausted")


def _np(a):
    return a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)


def _same(got, want, name, what):
    got, want = _np(got), np.asarray(want)
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    if want.dtype.kind == "f":
        bad = G.differs(got, want)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    else:
        assert np.array_equal(got, want), (what, name, np.argwhere(got != want)[:4].tolist())


def _check_stats(st, cnt, what):
    for k in COUNTERS:
        assert getattr(st, k) == cnt[k], (what, k, getattr(st, k), cnt[k])
    for k in ZERO_COUNTERS:
        assert getattr(st, k) == 0, (what, k)
    assert st.kernel_ms > 0


@pytest.fixture(scope="module")
def unit():
    ref, desc, g, keep = R.unit_ref()
    scene = dt.Scene(desc, g)
    yield scene, g, desc
    scene.close()


def test_zero_bounces_is_trace_rays(unit):
    """case 1: K = 0 is dt_trace_rays in shape, point, normal, albedo and every counter; length = (double)t * |dir|"""
    scene, g, desc = unit
    s, d, names = R.ray_set()
    hits, st0 = dt.trace_rays(scene, g, s, d)
    paths, st1 = dt.trace_rays_path(scene, g, s, d, max_bounces=0, planes=R.PLANES)
    for name in ("shape", "point", "normal", "albedo"):
        _same(paths[name], hits[name], name, "K = 0")
    for k in COUNTERS + ZERO_COUNTERS:
        assert getattr(st0, k) == getattr(st1, k), k
    assert st1.rays == len(s) - 3 and (hits["shape"] >= 0).sum() > 100 and (hits["shape"] < 0).any()
    t = hits["t"].astype(np.float64)
    want = np.where(hits["shape"] >= 0, t * np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]), 0.0)
    _same(paths["length"], want, "length", "K = 0")
    hit = hits["shape"] >= 0
    assert set(paths["end"][hit].tolist()) == {R.CUT} and set(paths["end"][~hit].tolist()) == {R.VOID, R.MISS}
    _same(paths["seg_shape"][:, 0], hits["shape"], "seg_shape", "K = 0")
    _same(paths["seg_point"][:, 0], hits["point"], "seg_point", "K = 0")
    # the counters belong to the planes, as dt_trace_rays's do
    _, sa = dt.trace_rays(scene, g, s, d, planes=("shape",))
    _, sb = dt.trace_rays_path(scene, g, s, d, max_bounces=0, planes=("shape",))
    for k in COUNTERS:
        assert getattr(sa, k) == getattr(sb, k), k


@pytest.mark.parametrize("K", [1, 2, 8])
def test_all_planes_and_counters_against_the_prediction(unit, K):
    """case 2: every plane and counter, 64 * 3 + 17 rays; then one ray alone"""
    scene, g, desc = unit
    s, d, names = R.ray_set()
    want, cnt, log = R.prediction(K)
    assert set(want["end"].tolist()) == {R.VOID, R.MISS, R.SURFACE, R.CUT}
    assert {R.REFLECT, R.REFRACT} <= R.codes_seen(log)
    i = names["through_centre"][0]
    assert want["end"][i] == R.VOID and want["segments"][i] == 1
    ins = names["inside"]
    assert (log[0]["seg"]["inside"][ins] == 1).all() and (log[0]["rule"]["chk"][ins] < 0).any()
    got, st = dt.trace_rays_path(scene, g, s, d, max_bounces=K, planes=R.PLANES)
    for name in R.PLANES:
        _same(got[name], want[name], name, "K = %d" % K)
    _check_stats(st, cnt, "K = %d" % K)
    assert st.rays > len(s)
    # n = 1: a ray that bounces, alone in its wave
    j = int(np.argmax(want["segments"]))
    one, st1 = dt.trace_rays_path(scene, g, s[j:j + 1], d[j:j + 1], max_bounces=K, planes=R.PLANES)
    for name in R.PLANES:
        _same(one[name], want[name][j:j + 1], name, "K = %d, n = 1" % K)
    assert st1.rays == want["segments"][j] >= 2
    # without the normal and albedo planes their counters stay 0 at the cut, the rest is the same
    few = ("end", "segments", "shape", "length", "point", "last_dir", "seg_shape")
    lean, cnt2, _ = R.prediction(K, normal=False, albedo=False)
    got2, st2 = dt.trace_rays_path(scene, g, s, d, max_bounces=K, planes=few)
    assert sorted(got2) == sorted(few + ("start",))
    for name in few:
        _same(got2[name], lean[name], name, "K = %d, few planes" % K)
    _check_stats(st2, cnt2, "K = %d, few planes" % K)


def test_wave_mates_do_not_matter(unit):
    """case 3: a fixed random permutation of the rays gives the same per-ray answers, and so does order=True"""
    scene, g, desc = unit
    s, d, names = R.ray_set()
    K = 8
    want, cnt, log = R.prediction(K)
    perm = np.random.RandomState(12345).permutation(len(s))
    assert (perm != np.arange(len(s))).sum() > 190
    got, st = dt.trace_rays_path(scene, g, s[perm].copy(), d[perm].copy(), max_bounces=K, planes=R.PLANES)
    for name in R.PLANES:
        _same(got[name], want[name][perm], name, "permuted")
    _check_stats(st, cnt, "permuted")
    for side in ("host", "device"):
        ss, dd = (s, d) if side == "host" else (torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda())
        got, st = dt.trace_rays_path(scene, g, ss, dd, max_bounces=K, planes=R.PLANES, order=True)
        for name in R.PLANES:
            _same(got[name], want[name], name, "order=True, " + side)
        _check_stats(st, cnt, "order=True, " + side)


def test_resolved_camera_rays_are_the_path_feature_buffers(unit):
    """case 4: camera_rays -> trace_rays_path(2) -> rays_resolve is render_features(specular_bounces=2) in albedo,
    normal, coverage, depth and bounces, 64 samples per pixel. Depth is included: rays_resolve's hit mean is the
    kernel's expression, the f64 sum of L over the samples that ended on a shape divided by their count as a
    double, cast to float."""
    scene, g, desc = unit
    n, K = 64, 2
    gg = type(g).from_buffer_copy(g)
    gg.antialias_samples = n
    st = dt.Stats()
    want = dt.render_features(scene, gg, 0, n_samples=n, planes=("albedo", "normal", "depth", "coverage", "bounces"),
                              stats=st, specular_bounces=K)
    assert (want["bounces"] > 0).any() and (want["coverage"] > 0).any()
    start, dir = dt.camera_rays(gg, 0, samples=(0, n))
    paths, pst = dt.trace_rays_path(scene, gg, start.view(-1, 3), dir.view(-1, 3), max_bounces=K,
                                    planes=("end", "segments", "shape", "length", "normal", "albedo"))
    shape = paths["shape"]
    alb, cov = dt.rays_resolve(gg, paths["albedo"], n, shape=shape, coverage=True)
    nrm = dt.rays_resolve(gg, paths["normal"], n, shape=shape)
    dep = dt.rays_resolve(gg, paths["length"], n, shape=shape, mode="hit_mean")
    fol = torch.clamp(paths["segments"] - 1, min=0) + ((paths["end"] == R.VOID) & (paths["segments"] >= 1))
    assert torch.equal(fol, torch.clamp(paths["segments"] - 1, min=0)), "a void successor among camera rays"
    bnc = dt.rays_resolve(gg, fol.double(), n)
    for name, got in (("albedo", alb), ("normal", nrm), ("coverage", cov), ("depth", dep), ("bounces", bnc)):
        assert torch.equal(got.reshape(-1).view(torch.int32), want[name].reshape(-1).view(torch.int32)), name
    for k in COUNTERS:
        assert getattr(pst, k) == getattr(st, k), k


def test_host_and_device_arrays_and_only_the_planes_asked_for(unit):
    """case 5: host arrays come back as device arrays do, and a plane that was not asked for is not written"""
    scene, g, desc = unit
    s, d, names = R.ray_set()
    K, n = 2, len(s)
    want, cnt, log = R.prediction(K)
    sd, dd = torch.from_numpy(s).cuda(), torch.from_numpy(d).cuda()
    dev, std = dt.trace_rays_path(scene, g, sd, dd, max_bounces=K, planes=R.PLANES)
    host, sth = dt.trace_rays_path(scene, g, s, d, max_bounces=K, planes=R.PLANES)
    for name in R.PLANES:
        assert dev[name].is_cuda and isinstance(host[name], np.ndarray)
        assert dev[name].cpu().numpy().tobytes() == host[name].tobytes(), name
        _same(host[name], want[name], name, "host")
    _check_stats(std, cnt, "device")
    _check_stats(sth, cnt, "host")
    # through the export itself: one buffer per plane filled with a sentinel, the planes asked for in turns
    from distraytracer_amd._lib import RayPaths
    SENT = 0x5A
    asked_sets = (("end", "seg_point"), ("length", "last_start", "seg_shape"), ("segments", "shape", "point", "normal",
                                                                                "albedo", "last_dir"))
    for on_device in (0, 1):
        for asked in asked_sets:
            bufs = {}
            for name in R.PLANES:
                nbytes = want[name].nbytes
                bufs[name] = (torch.full((nbytes,), SENT, dtype=torch.uint8, device="cuda") if on_device else
                              np.full(nbytes, SENT, np.uint8))
            h = RayPaths(**{name: (bufs[name].data_ptr() if on_device else bufs[name].ctypes.data) for name in asked})
            sp, dp = (sd.data_ptr(), dd.data_ptr()) if on_device else (s.ctypes.data, d.ctypes.data)
            st = dt.Stats()
            dt.check(dt.lib.dt_trace_rays_path(scene.handle, ctypes.byref(g), n, ctypes.c_void_p(sp), ctypes.c_void_p(dp),
                                               K, ctypes.byref(h), on_device, None, ctypes.byref(st)), "dt_trace_rays_path")
            for name in R.PLANES:
                raw = _np(bufs[name]).tobytes()
                if name in asked:
                    assert raw == want[name].tobytes(), (on_device, name)
                else:
                    assert raw == bytes([SENT]) * len(raw), (on_device, name)
            assert st.rays == cnt["rays"]


def test_a_render_before_and_after_is_the_same_bytes():
    """case 6"""
    desc, g, keep = R.unit_scene(4)
    g.max_depth = 3
    s, d, names = R.ray_set()
    scene = dt.Scene(desc, g)
    try:
        a = torch.zeros(3 * 24 * 16, device="cuda")
        b = torch.zeros_like(a)
        dt.render(scene, g, 0, a)
        paths, pst = dt.trace_rays_path(scene, g, s, d, max_bounces=8)
        st = dt.render(scene, g, 0, b)
    finally:
        scene.close()
    assert paths["segments"].max() >= 4 and (a != 0).any()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and st.pixels == 24 * 16


def test_empty_and_zero_rays(unit):
    scene, g, desc = unit
    paths, st = dt.trace_rays_path(scene, g, np.zeros((0, 3)), np.zeros((0, 3)), max_bounces=3, planes=R.PLANES)
    assert paths["seg_point"].shape == (0, 4, 3) and paths["end"].shape == (0,) and st.rays == 0 and st.kernel_ms == 0


def test_prismcyl_scene_is_unsupported():
    """case 7"""
    g = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, g)
    g.xRes, g.yRes, g.antialias_samples = 16, 12, 4
    scene = dt.Scene(built, g)
    try:
        with pytest.raises(dt.DTError, match=r"dt_trace_rays_path failed \(-4\): dt_trace_rays_path: .*RectPrismWithCylinder"):
            dt.trace_rays_path(scene, g, np.zeros((2, 3)), np.ones((2, 3)))
    finally:
        scene.close()


def test_pick_and_polyline(unit):
    """pick() is trace_rays_path on sample 0's camera ray of the pixel; ray_polyline walks its vertices"""
    scene, g, desc = unit
    start, dir = dt.camera_rays(g, 0, samples=(0, 1), host=True)
    all_paths, _ = dt.trace_rays_path(scene, g, start.reshape(-1, 3), dir.reshape(-1, 3), max_bounces=4, planes=R.PLANES)
    first = all_paths["seg_shape"][:, 0].reshape(g.yRes, g.xRes)
    ys, xs = np.nonzero((first == R.STEEL_SPHERE) & (all_paths["segments"].reshape(g.yRes, g.xRes) >= 2))
    assert len(ys) > 0, "no pixel of the steel sphere"
    x, y = int(xs[0]), int(ys[0])
    q = y * g.xRes + x
    paths, st = dt.pick(scene, g, 0, x, y)
    for name in R.PLANES:
        _same(paths[name], all_paths[name][q:q + 1], name, "pick")
    assert paths["shape"][0].item() != R.STEEL_SPHERE
    poly = dt.ray_polyline(paths, 0)
    hits = _np(paths["seg_shape"][0]) >= 0
    assert poly.shape == (1 + hits.sum(), 3) and poly.shape[0] >= 2
    assert np.array_equal(poly[0], start.reshape(-1, 3)[q]) and np.array_equal(poly[1], all_paths["seg_point"][q, 0])


def test_cli_pick(tmp_path):
    """case 8: dtrender final 30 --nogloss --pick X,Y on a pixel of a steel reflector prints at least two segments
    and ends on another shape, as trace_rays_path says; the frame file is the same bytes with and without the flag"""
    STEEL = 2
    g = dt.globals_default()   # the CLI's globals: defaults, no models, buildFinal(240), then the options
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth, g.nogloss = 40, 24, 4, 2, 1
    desc = built.desc
    scene = dt.Scene(built, g)
    try:
        start, dir = dt.camera_rays(g, 240, samples=(0, 1), host=True)
        allp, _ = dt.trace_rays_path(scene, g, start.reshape(-1, 3), dir.reshape(-1, 3), max_bounces=4,
                                     planes=("end", "segments", "shape", "length", "seg_shape", "seg_point"))
    finally:
        scene.close()
    first = allp["seg_shape"][:, 0]
    # (final's steel is its two doors, mirrors under nogloss; it holds no steel sphere)
    steel = [i for i in range(desc.n_shapes) if desc.shapes[i].material == STEEL]
    assert steel, "final has no steel shape"
    cand = (allp["segments"] >= 2) & (allp["shape"] >= 0) & (allp["shape"] != first)
    assert cand.any(), "no pixel of a mirror whose path ends on another shape"
    on_steel = cand & np.isin(first, steel)   # a door where one is in view, else any mirror
    q = int(np.nonzero(on_steel if on_steel.any() else cand)[0][0])
    y, x = divmod(q, g.xRes)
    common = [DTRENDER, "final", "30", "--res", "40x24", "--spp", "4", "--depth", "2", "--nogloss"]
    plain, picked = str(tmp_path / "plain.png"), str(tmp_path / "picked.png")
    a = subprocess.run(common + ["--out", plain], check=True, timeout=120, capture_output=True)
    b = subprocess.run(common + ["--out", picked, "--pick", "%d,%d" % (x, y)], check=True, timeout=120,
                       capture_output=True)
    assert open(plain, "rb").read() == open(picked, "rb").read()
    lines = [l for l in b.stdout.decode().splitlines() if l.startswith("pick ")]
    assert not [l for l in a.stdout.decode().splitlines() if l.startswith("pick ")]
    segs = [re.match(r"pick %d,%d: segment (\d+) shape (-?\d+) material (-?\d+)" % (x, y), l) for l in lines[:-1]]
    assert all(segs) and len(segs) == allp["segments"][q] >= 2
    assert [int(m.group(1)) for m in segs] == list(range(len(segs)))
    assert [int(m.group(2)) for m in segs] == allp["seg_shape"][q, :len(segs)].tolist()
    assert [int(m.group(3)) for m in segs] == [desc.shapes[int(m.group(2))].material for m in segs]
    assert int(segs[-1].group(2)) == allp["shape"][q] != int(segs[0].group(2))
    end = re.match(r"pick %d,%d: end (\w+) L (\S+)$" % (x, y), lines[-1])
    assert end and end.group(1) == ("void", "miss", "surface", "cut")[allp["end"][q]]
    assert float("%.9g" % allp["length"][q]) == float(end.group(2))
    bad = subprocess.run(common + ["--pick", "40,0"], timeout=120, capture_output=True)
    assert bad.returncode == 2 and b"--pick" in bad.stderr
    bad = subprocess.run(common + ["--pick", "1,1", "--pick-bounces", "9"], timeout=120, capture_output=True)
    assert bad.returncode == 2 and b"--pick" in bad.stderr
    # the one mode that renders no scene refuses the flag instead of ignoring it
    bad = subprocess.run([DTRENDER, "perlin", "0", "--pick", "1,1"], timeout=120, capture_output=True)
    assert bad.returncode == 2 and b"--pick" in bad.stderr
