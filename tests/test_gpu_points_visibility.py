"""Mutual visibility of two point sets (include/dt.h dt_points_visibility; dt_points_vis_kernel and its weight
reduction) against the prediction of tests/points_visibility_ref.py, made on the CPU from the oracle's exports and
the host export dt_irradiance_cosine, bit for bit: integers as integers, weight_a by the bit pattern of its doubles.

The fixture is that module's scene and point sets: 64*2 + 7 sources (a tail wave) against 256 + 37 targets (a
second, shorter tile and a partial last word), one void source in the middle of the second wave, one void target,
one target that is a source (the void-ray pair), skip_b the panel for the targets on it and -1 for those in front
of it. One prediction, 39555 pairs answered once on the CPU, serves every case; a pair depends on nothing else, so
the smaller shapes and the split of the targets are cuts of it."""
import numpy as np
import pytest
import torch

import distraytracer_amd as dt
from points_visibility_ref import (N_A, N_B, NAN_A, NAN_B, PLANES, SAME_A, SAME_B, TILE, VisibilityRef, case, pairs,
                                   reference)

pytestmark = pytest.mark.gpu


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        g, w = np.ascontiguousarray(_np(got[k])), np.ascontiguousarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        g = g.view(np.uint64 if k == "weight_a" else np.uint32).reshape(-1)
        w = w.view(np.uint64 if k == "weight_a" else np.uint32).reshape(-1)
        bad = np.nonzero(g != w)[0]
        print("%s %s: %d of %d entries differ" % (what, k, bad.size, w.size))
        assert bad.size == 0, "%s %s entry %d" % (what, k, bad[0])


def _stats(st, traced, what=""):
    print(what, "shadow_rays", st.shadow_rays, "prediction", traced)
    assert st.shadow_rays == traced, what
    d = st.as_dict()   # everything else is 0
    assert all(v == 0 for k, v in d.items() if k not in ("shadow_rays", "kernel_ms")), d


def _call(scene, g, falloff=0, planes=PLANES, rows=slice(None), cols=slice(None), device=False):
    a, na, b, nb, skip, desc, _, keep, panel = case()
    arrs = [np.ascontiguousarray(x) for x in (a[rows], b[cols], skip[cols], na[rows], nb[cols])]
    if device:
        arrs = [torch.from_numpy(x.copy()).cuda() for x in arrs]
    return dt.points_visibility(scene, g, arrs[0], arrs[1], skip_b=arrs[2], normals_a=arrs[3], normals_b=arrs[4],
                                falloff=bool(falloff), planes=planes)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("falloff", [0, 1])
def test_all_planes_are_the_prediction(falloff, device):
    ref, _, _ = reference()
    want, traced = ref.planes(falloff)
    a, na, b, nb, skip, desc, g, keep, panel = case()
    scene = dt.Scene(desc, g)
    try:
        got, st = _call(scene, g, falloff, device=device)
    finally:
        scene.close()
    if device:
        assert all(v.is_cuda for v in got.values()) and got["bits"].dtype == torch.int32
    else:
        assert all(isinstance(v, np.ndarray) for v in got.values()) and got["bits"].dtype == np.uint32
    assert tuple(got["bits"].shape) == (N_A, (N_B + 31) // 32) and tuple(got["weight_a"].shape) == (N_A,)
    _same(got, want, "falloff %d %s" % (falloff, "device" if device else "host"))
    _stats(st, traced)
    assert st.kernel_ms > 0
    # the void points and the void-ray pair, on the device's answer
    vis = dt.visibility_matrix(got["bits"], N_B)
    assert not vis[NAN_A].any() and not vis[:, NAN_B].any() and vis[SAME_A, SAME_B]
    assert _np(got["count_a"])[NAN_A] == 0 and _np(got["count_b"])[NAN_B] == 0 and _np(got["weight_a"])[NAN_A] == 0
    assert (_np(got["bits"]).view(np.uint32)[:, -1] >> np.uint32(N_B % 32) == 0).all()   # the unused high bits


def test_bits_are_rays_occluded_on_the_materialised_pairs():
    """through the existing call, not the restatement: visible == 1 - occluded"""
    a, na, b, nb, skip, desc, g, keep, panel = case()
    start, dir = pairs(a, b)
    scene = dt.Scene(desc, g)
    try:
        got, st = _call(scene, g, planes=("bits",))
        occ, so = dt.rays_occluded(scene, g, start, dir, skip_shape=np.tile(skip, N_A))
    finally:
        scene.close()
    vis = dt.visibility_matrix(got["bits"], N_B)
    live = np.isfinite(a).all(axis=1)[:, None] & np.isfinite(b).all(axis=1)[None, :]
    want = (occ.reshape(N_A, N_B) == 0) & live   # a void ray reports "not occluded"; a void point sees nothing
    bad = np.nonzero(vis != want)
    print("bits against rays_occluded: %d of %d pairs differ" % (len(bad[0]), vis.size))
    assert len(bad[0]) == 0
    assert st.shadow_rays == so.shadow_rays > 0
    assert 10 * want.sum() >= want.size and 10 * (~want).sum() >= want.size


def test_counts_are_the_row_and_column_sums_of_the_bits():
    a, na, b, nb, skip, desc, g, keep, panel = case()
    scene = dt.Scene(desc, g)
    try:
        got, _ = _call(scene, g, planes=("bits", "count_a", "count_b"), device=True)
    finally:
        scene.close()
    vis = dt.visibility_matrix(got["bits"], N_B)
    assert np.array_equal(_np(got["count_a"]), vis.sum(axis=1)) and np.array_equal(_np(got["count_b"]), vis.sum(axis=0))
    assert vis.any() and not vis.all()


@pytest.mark.parametrize("planes", [("bits",), ("count_a",), ("count_b",), ("weight_a",), ("count_b", "weight_a")])
def test_fewer_planes_leave_the_others_answers_unchanged(planes):
    ref, _, _ = reference()
    want, traced = ref.planes(1, want=planes)
    a, na, b, nb, skip, desc, g, keep, panel = case()
    scene = dt.Scene(desc, g)
    try:
        got, st = _call(scene, g, 1, planes=planes)
    finally:
        scene.close()
    _same(got, want, "+".join(planes))
    _stats(st, traced)
    # (the normals are finite here, so the pairs traced do not depend on weight_a being asked for)
    assert traced == ref.planes(1)[1]


def test_the_answer_does_not_depend_on_how_the_targets_are_split():
    ref, _, _ = reference()
    a, na, b, nb, skip, desc, g, keep, panel = case()
    scene = dt.Scene(desc, g)
    try:
        full, sf = _call(scene, g, 1)
        left, sl = _call(scene, g, 1, cols=slice(0, TILE))
        right, sr = _call(scene, g, 1, cols=slice(TILE, N_B))
    finally:
        scene.close()
    _same(left, ref.planes(1, cols=slice(0, TILE))[0], "the first 256 targets")
    _same(right, ref.planes(1, cols=slice(TILE, N_B))[0], "the last 37 targets")
    vis = np.hstack([dt.visibility_matrix(left["bits"], TILE), dt.visibility_matrix(right["bits"], N_B - TILE)])
    assert np.array_equal(vis, dt.visibility_matrix(full["bits"], N_B))
    assert np.array_equal(left["count_a"] + right["count_a"], full["count_a"])
    assert np.array_equal(np.concatenate([left["count_b"], right["count_b"]]), full["count_b"])
    # the fixed order: the full call's (0.0 + tile 0) + tile 1 is the sum of the two calls' weights, bit for bit
    assert (left["weight_a"] + right["weight_a"]).tobytes() == full["weight_a"].tobytes()
    assert (left["weight_a"] > 0).any() and (right["weight_a"] > 0).any()
    assert sl.shadow_rays + sr.shadow_rays == sf.shadow_rays


@pytest.mark.parametrize("rows,cols", [(slice(20, 21), slice(250, 283)), (slice(32, 97), slice(270, 271)),
                                       (slice(0, N_A), slice(TILE - 1, TILE + 1))],
                         ids=["1x33", "65x1", "135x2"])
def test_the_smallest_shapes(rows, cols):
    """one source against 33 targets (63 tail lanes, a partial second word); 65 sources against one target (a second
    wave of one lane, and that lane the void source: a wave that runs no walk); the two targets on either side of
    the big case's tile border as a call of their own, whose tiles start at its own target 0"""
    a, na, b, nb, skip, desc, g, keep, panel = case()
    ref, _, _ = reference()
    sub = VisibilityRef(desc, g, a[rows], b[cols], skip[cols], na[rows], nb[cols], rq=ref.rq)
    want, traced = sub.planes(1)
    scene = dt.Scene(desc, g)
    try:
        got, st = _call(scene, g, 1, rows=rows, cols=cols)
        dev, sd = _call(scene, g, 1, rows=rows, cols=cols, device=True)
    finally:
        scene.close()
    _same(got, want, "host")
    _same(dev, want, "device")
    _stats(st, traced)
    _stats(sd, traced)
    assert want["count_a"].sum() > 0
    # ... and the cut of the big prediction says the same of bits and counts
    big = dt.visibility_matrix(ref.planes(1)[0]["bits"], N_B)[rows, cols]
    assert np.array_equal(dt.visibility_matrix(got["bits"], big.shape[1]), big)


def test_a_void_normal_voids_its_point_only_when_the_weight_is_wanted():
    a, na, b, nb, skip, desc, g, keep, panel = case()
    ref, _, _ = reference()
    na2, nb2 = na.copy(), nb.copy()
    na2[70, 0] = np.inf
    nb2[5, 1] = np.nan
    sub = VisibilityRef(desc, g, a, b, skip, na2, nb2, rq=ref.rq)
    scene = dt.Scene(desc, g)
    try:
        with_w, sw = dt.points_visibility(scene, g, a, b, skip_b=skip, normals_a=na2, normals_b=nb2, planes=PLANES)
        without, so = dt.points_visibility(scene, g, a, b, skip_b=skip, normals_a=na2, normals_b=nb2,
                                           planes=("bits", "count_a", "count_b"))
    finally:
        scene.close()
    want_w, traced_w = sub.planes(0)
    want_o, traced_o = sub.planes(0, want=("bits", "count_a", "count_b"))
    _same(with_w, want_w, "weight wanted")
    _same(without, want_o, "weight not wanted")
    _stats(sw, traced_w)
    _stats(so, traced_o)
    assert traced_w < traced_o
    vis = dt.visibility_matrix(with_w["bits"], N_B)
    assert not vis[70].any() and not vis[:, 5].any() and with_w["weight_a"][70] == 0
    assert dt.visibility_matrix(without["bits"], N_B)[70].any()


def test_no_skip_shapes_hides_the_panels_own_texels():
    a, na, b, nb, skip, desc, g, keep, panel = case()
    _, none, _ = reference()
    want, traced = none.planes(0, want=("bits", "count_a", "count_b"))
    scene = dt.Scene(desc, g)
    try:
        got, st = dt.points_visibility(scene, g, a, b)
    finally:
        scene.close()
    _same(got, want, "skip_b None")
    _stats(st, traced)


def test_a_render_before_and_after_is_the_same_bytes():
    a, na, b, nb, skip, desc, g, keep, panel = case()
    g = g.copy()
    g.antialias_samples, g.max_depth = 4, 3
    n_px = g.xRes * g.yRes
    scene = dt.Scene(desc, g)
    try:
        before = torch.zeros(3 * n_px, device="cuda")
        after = torch.zeros_like(before)
        dt.render(scene, g, 0, before)
        got, _ = _call(scene, g, 1)
        st = dt.render(scene, g, 0, after)
    finally:
        scene.close()
    assert (got["count_a"] > 0).any()
    assert torch.equal(before.view(torch.int32), after.view(torch.int32)) and st.pixels == n_px and (before != 0).any()


def test_prismcyl_is_unsupported_and_no_pairs_is_ok():
    a, na, b, nb, skip, desc, g, keep, panel = case()
    gp = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, gp)
    scene = dt.Scene(built, gp)
    try:
        with pytest.raises(dt.DTError,
                           match=r"dt_points_visibility failed \(-4\): dt_points_visibility: .*RectPrismWithCylinder"):
            dt.points_visibility(scene, gp, a, b)
    finally:
        scene.close()
    scene = dt.Scene(desc, g)
    try:
        for dev in (False, True):
            mk = (lambda x: torch.from_numpy(np.array(x)).cuda()) if dev else np.ascontiguousarray
            some, no3 = mk(a[:5]), mk(np.zeros((0, 3)))
            five_n, no_n = mk(na[:5]), mk(np.zeros((0, 3)))
            # (the wrapper's planes are new arrays: test_no_pairs_zeroes_the_callers_planes shows the zeroing)
            got, st = dt.points_visibility(scene, g, some, no3, normals_a=five_n, normals_b=no_n, planes=PLANES)
            assert tuple(got["bits"].shape) == (5, 0) and tuple(got["count_b"].shape) == (0,)
            assert (_np(got["count_a"]) == 0).all() and (_np(got["weight_a"]) == 0).all()
            assert st.shadow_rays == 0 and st.kernel_ms == 0
            got, st = dt.points_visibility(scene, g, no3, some, normals_a=no_n, normals_b=five_n, planes=PLANES)
            assert tuple(got["bits"].shape) == (0, 1) and tuple(got["count_a"].shape) == (0,)
            assert (_np(got["count_b"]) == 0).all() and tuple(got["count_b"].shape) == (5,)
            assert st.shadow_rays == 0 and st.kernel_ms == 0
    finally:
        scene.close()


def test_no_pairs_zeroes_the_callers_planes():
    """through the C ABI with planes that held something: count_a and weight_a of 5 sources against no target"""
    import ctypes
    from distraytracer_amd._lib import Visibility, VisibilityParams
    a, na, b, nb, skip, desc, g, keep, panel = case()
    src = np.ascontiguousarray(a[:5])
    nrm = np.ascontiguousarray(na[:5])
    count_a, weight_a = np.full(5, 77, np.int32), np.full(5, 3.5)
    p = VisibilityParams()
    p.normal_a = p.normal_b = nrm.ctypes.data
    out = Visibility(None, count_a.ctypes.data, None, weight_a.ctypes.data)
    scene = dt.Scene(desc, g)
    try:
        rc = dt.lib.dt_points_visibility(scene.handle, ctypes.byref(g), 5, src.ctypes.data, 0, src.ctypes.data,
                                         ctypes.byref(p), ctypes.byref(out), 0, None, None)
    finally:
        scene.close()
    assert rc == 0 and (count_a == 0).all() and (weight_a == 0).all()


def test_bake_visibility_is_points_visibility_on_the_texels():
    a, na, b, nb, skip, desc, g, keep, panel = case()
    floor = 0
    scene = dt.Scene(desc, g)
    try:
        pa, nra = dt.shape_texels(desc, floor, 6, 4)
        pb, nrb = dt.shape_texels(desc, panel, 5, 3)
        want, sw = dt.points_visibility(scene, g, pa, pb, skip_b=np.full(15, panel, np.int32), normals_a=nra,
                                        normals_b=nrb, falloff=True, planes=("count_a", "weight_a"))
        got, sg = dt.bake_visibility(scene, desc, g, floor, panel, 6, 4, target_size=(5, 3), falloff=True,
                                     planes=("weight_a",))
    finally:
        scene.close()
    assert got["visible"].shape == (4, 6) and got["visible"].dtype == np.float32 and got["weight"].shape == (4, 6)
    assert np.array_equal(got["visible"].reshape(-1), (want["count_a"].astype(np.float64) / 15.0).astype(np.float32))
    assert got["weight"].reshape(-1).tobytes() == want["weight_a"].tobytes()
    assert sg.shadow_rays == sw.shadow_rays == 24 * 15
    assert 0 < got["visible"].max() <= 1 and (got["visible"] < got["visible"].max()).any()


def test_cli_bake_visible_image(tmp_path):
    """dtrender final 30 --bake-visible A,B ...: the PNG is the bytes dt_write_png makes of bake_visibility's image
    times 255, and the frame is the file written without the flag"""
    import subprocess

    import scene_gen
    from test_gpu_features import DTRENDER
    g = dt.globals_default()   # the CLI's globals: defaults, no models, buildFinal(240), then the options
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = 40, 24, 16, 2
    d = built.desc
    flat = [i for i in range(d.n_shapes) if d.shapes[i].type in (scene_gen.RECTANGLE, scene_gen.CHECKER)]
    sa, sb = flat[0], flat[-1]
    assert sa != sb
    BW, BH, TW, TH = 8, 4, 5, 3
    common = [DTRENDER, "final", "30", "--res", "40x24", "--spp", "16", "--depth", "2"]
    plain, with_b, prefix = str(tmp_path / "plain.png"), str(tmp_path / "bake.png"), str(tmp_path / "V")
    subprocess.run(common + ["--out", plain], check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run(common + ["--out", with_b, "--bake-visible", "%d,%d" % (sa, sb), "--bake-size", "%dx%d" % (BW, BH),
                             "--bake-target-size", "%dx%d" % (TW, TH), "--bake-out", prefix],
                   check=True, timeout=120, stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_b, "rb").read()
    scene = dt.Scene(built, g)
    try:
        imgs, st = dt.bake_visibility(scene, built, g, sa, sb, BW, BH, target_size=(TW, TH))
    finally:
        scene.close()
    assert st.shadow_rays == BW * BH * TW * TH
    gb = g.copy()
    gb.xRes, gb.yRes = BW, BH
    want = str(tmp_path / "want.png")
    dt.write_png(want, gb, np.repeat(imgs["visible"].reshape(-1) * np.float32(255), 3))
    assert open(prefix + ".visible.png", "rb").read() == open(want, "rb").read()
    # a usage error: no target size
    r = subprocess.run(common + ["--out", with_b, "--bake-visible", "%d,%d" % (sa, sb), "--bake-size", "8x4",
                                 "--bake-out", prefix], timeout=120, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--bake-target-size" in r.stderr
