"""Ray ordering on the device (include/dt.h dt_ray_order, dt_permute_rows; csrc/dt_rayorder.hip) against the host
path and the numpy restatement of tests/rayorder_ref.py, which tests/test_rayorder_host.py pins to each other.
Everything is compared exactly (integers, bit patterns).

The issue lists B = 1, 8, 9 and 30 for the sort; B = 3*origin_bits + 2*dir_bits cannot be 1. The cases here
are B = 2 (the smallest, one pass), 7 (8 sorted bits: the largest single pass), 8 (9 sorted bits, the void
key's bit 8: two passes), 9 (two) and 30 (four)."""
import functools

import numpy as np
import pytest
import torch

import distraytracer_amd as dt

import rayorder_ref as R
from test_rayorder_host import key_inputs, params

pytestmark = pytest.mark.gpu

T = dt.DT_RAY_ORDER_TILE
SIZES = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 37, 64 * T + 37]
UNIT = (np.zeros(3), np.ones(3))
# B -> (origin_bits, dir_bits), passes
SORT_CONFIGS = {2: ((0, 1), 1), 7: ((1, 2), 1), 8: ((0, 4), 2), 9: ((3, 0), 2), 30: ((10, 0), 4)}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=lambda c: "ob%d-db%d-%s" % (c[0], c[1], "dir" if c[2] else "origin"))
def test_device_keys_box_and_order_equal_the_host_path(cfg):
    """1: on the inputs of the host test"""
    ob, db, major = cfg
    for name, start, dir, box in key_inputs():
        p = params(ob, db, major, box)
        host = dt.ray_order(start, dir, params=p, keys=True)
        dev = dt.ray_order(_cuda(start), _cuda(dir), params=p, keys=True)
        assert dev.perm.is_cuda and dev.keys.is_cuda and dev.kernel_ms > 0
        assert np.array(dev.box).tobytes() == np.array(host.box).tobytes(), (name, dev.box, host.box)
        k = _np(dev.keys).view(np.uint32)
        bad = np.nonzero(k != host.keys)[0]
        assert bad.size == 0, "%s ray %d: device key %d, host %d" % (name, bad[0], k[bad[0]], host.keys[bad[0]])
        assert np.array_equal(_np(dev.perm).view(np.uint32), host.perm), name


def _pool(n, ob, rng):
    """n rays in the unit box: starts at cell centres (so that half a box further is the same cell with its top
    bit flipped), any direction"""
    cells = 1 << ob
    start = (rng.integers(0, cells, (n, 3)) + 0.5) / cells
    return start, rng.normal(size=(n, 3))


def _key_sets(n, B, rng):
    """name -> (start, dir, keys, check): the key patterns of the issue for one size, with what each must hold"""
    (ob, db), passes = SORT_CONFIGS[B]
    top = 8 * (passes - 1)
    ps, pd = _pool(n + 1, ob, rng)
    keys = lambda s, d: R.keys_of(s, d, ob, db, 0, *UNIT)
    sets = {}
    sets["all equal"] = (np.tile(ps[:1], (n, 1)), np.tile(pd[:1], (n, 1)))
    s2, d2 = ps[:2].copy(), pd[:2].copy()
    d2[1] = -d2[0]   # the opposite direction: another key (origin cells alone: the far corner's)
    s2[1] = 1.0 - s2[0]
    pick = rng.integers(0, 2, n)
    sets["two values"] = (s2[pick], d2[pick])
    asc = np.argsort(keys(ps[:n], pd[:n]), kind="stable")
    sets["ascending"] = (ps[asc], pd[asc])
    sets["descending"] = (ps[asc[::-1]], pd[asc[::-1]])
    st, dt_ = np.tile(ps[:1], (n, 1)), np.tile(pd[:1], (n, 1))
    if ob >= 3:   # the top bit of the z cell is key bit B - 1, in the top digit
        st[1::2, 2] += np.where(st[1::2, 2] < 0.5, 0.5, -0.5)
    else:         # the top digit holds the void bit alone: key 0 (the first cell of either map) against 1 << B
        st[:] = 0.5 / (1 << ob)
        dt_[:] = (-0.05, -0.05, -0.9)
        dt_[1::2] = 0.0
    sets["top digit only"] = (st, dt_)
    sv, dv = ps[asc[::-1]].copy(), pd[asc[::-1]].copy()
    dv[::3] = 0.0
    sv[1::7, 0] = np.nan
    sets["void interleaved"] = (sv, dv)
    out = {}
    for name, (s, d) in sets.items():
        k = keys(s, d)
        distinct = len(np.unique(k))
        if name == "all equal":
            assert distinct == 1
        elif name == "two values" and n > 8:
            assert distinct == 2, (B, n, distinct)
        elif name in ("ascending", "descending") and n > 1:
            assert distinct >= min(n, 1 << B) // 4, (B, n, distinct)
            assert (np.diff(k.astype(np.int64)) >= 0).all() if name == "ascending" else (np.diff(k.astype(np.int64)) <= 0).all()
        elif name == "top digit only" and n > 1 and passes > 1:
            assert distinct == 2 and ((k[0] ^ k[1]) & ((1 << top) - 1)) == 0 and (k[0] ^ k[1]) >> top, (B, k[:2])
        elif name == "void interleaved":
            assert (k[::3] == 1 << B).all() and (n < 3 or (k != 1 << B).any())
        out[name] = (np.ascontiguousarray(s), np.ascontiguousarray(d), k)
    return out


@pytest.mark.parametrize("B", sorted(SORT_CONFIGS))
def test_device_perm_is_the_stable_argsort(B):
    """2: every size and key pattern; one, one, two, two and four passes"""
    (ob, db), passes = SORT_CONFIGS[B]
    assert 3 * ob + 2 * db == B and passes == (B + 1 + 7) // 8
    assert 256 * -(-SIZES[-1] // T) > 2048 * 8   # the last size needs more than one level of the histogram scan
    p = params(ob, db, 0, UNIT)
    rng = np.random.default_rng(1000 + B)
    for n in SIZES:
        for name, (s, d, k) in _key_sets(n, B, rng).items():
            dev = dt.ray_order(_cuda(s), _cuda(d), params=p, keys=True)
            assert np.array_equal(_np(dev.keys).view(np.uint32), k), (B, n, name)
            got, want = _np(dev.perm).view(np.uint32), R.order_of(k)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, "B %d, n %d, %s: place %d holds ray %d, argsort(kind='stable') %d (%d places differ)" % (
                B, n, name, bad[0], got[bad[0]], want[bad[0]], bad.size)
            assert dev.box == (0.0, 0.0, 0.0, 1.0, 1.0, 1.0)


def test_device_order_without_keys_or_timing_and_of_no_rays():
    ss, sd = key_inputs()[0][1:3]
    host = dt.ray_order(ss, sd)
    dev = dt.ray_order(_cuda(ss), _cuda(sd))
    assert dev.keys is None and np.array_equal(_np(dev.perm).view(np.uint32), host.perm)
    # the plain C call: no keys, no box, no timing -- enqueue only, on the null stream
    import ctypes
    s, d = _cuda(ss), _cuda(sd)
    perm = torch.zeros(len(ss), dtype=torch.int32, device="cuda")
    work = torch.empty(int(dt.lib.dt_ray_order_workspace_bytes(len(ss))), dtype=torch.uint8, device="cuda")
    p = dt.ray_order_params_default()
    dt.check(dt.lib.dt_ray_order(len(ss), s.data_ptr(), d.data_ptr(), ctypes.byref(p), perm.data_ptr(), None, None,
                                 work.data_ptr(), 1, None, None), "dt_ray_order")
    torch.cuda.synchronize()
    assert np.array_equal(_np(perm).view(np.uint32), host.perm)
    none = dt.ray_order(torch.zeros(0, 3, dtype=torch.float64, device="cuda"),
                        torch.zeros(0, 3, dtype=torch.float64, device="cuda"), keys=True)
    assert none.n == 0 and none.perm.numel() == 0 and none.box == (0.0,) * 6


@pytest.mark.parametrize("row", [1, 4, 24])
def test_device_permute_rows(row):
    """3: gather and inverse at n = 2T + 37 against numpy indexing"""
    n = 2 * T + 37
    rng = np.random.default_rng(row)
    s, d = _pool(n, 10, rng)
    order = dt.ray_order(_cuda(s), _cuda(d))
    perm = _np(order.perm).view(np.uint32)
    assert np.array_equal(np.sort(perm), np.arange(n))
    a = {1: rng.integers(0, 256, n).astype(np.uint8), 4: rng.normal(size=n).astype(np.float32), 24: s}[row]
    assert a.nbytes == row * n
    got = order.apply(_cuda(a))
    assert got.is_cuda and _np(got).tobytes() == a[perm].tobytes()
    want_back = np.zeros_like(a)
    want_back[perm] = a
    back = order.restore(_cuda(a))
    assert _np(back).tobytes() == want_back.tobytes()
    assert _np(order.restore(got)).tobytes() == a.tobytes()


@functools.lru_cache(maxsize=None)
def _final():
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes = 1920, 1080
    return g, built


def _same(a, b, what):
    a = _np(a) if hasattr(a, "cpu") else a
    b = _np(b) if hasattr(b, "cpu") else b
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def test_ordered_queries_equal_the_plain_ones_bit_for_bit():
    """4: final(240), the scattered rays, device and host arrays, every plane; stats.rays unchanged"""
    g, built = _final()
    ss, sd = key_inputs()[0][1:3]
    scene = dt.Scene(built, g)
    try:
        plain, st0 = dt.trace_rays(scene, g, _cuda(ss), _cuda(sd))
        hit = _np(plain["shape"]) >= 0
        assert hit.any() and (~hit).any() and st0.rays == len(ss)
        order = dt.ray_order(_cuda(ss), _cuda(sd))
        assert not np.array_equal(_np(order.perm), np.arange(len(ss)))   # the order does move rays
        for how, o in (("order=True", True), ("a RayOrder", order)):
            got, st = dt.trace_rays(scene, g, _cuda(ss), _cuda(sd), order=o)
            assert set(got) == set(dt.RAY_PLANES) and st.rays == st0.rays
            assert (st.tex_fetches, st.uv_out_of_range, st.prism_norm_fallback) == (
                st0.tex_fetches, st0.uv_out_of_range, st0.prism_norm_fallback)
            for k in dt.RAY_PLANES:
                assert got[k].is_cuda
                _same(got[k], plain[k], "device arrays, %s, %s" % (how, k))
        host, st = dt.trace_rays(scene, g, ss, sd, order=True)
        assert st.rays == st0.rays
        for k in dt.RAY_PLANES:
            assert isinstance(host[k], np.ndarray)
            _same(host[k], plain[k], "host arrays, %s" % k)
        two = {"t": torch.full((len(ss),), -1.0, dtype=torch.float32, device="cuda")}
        dt.trace_rays(scene, g, _cuda(ss), _cuda(sd), out=two, order=order)
        _same(two["t"], plain["t"], "out=")

        # visibility from the hit points towards the lights, each ray skipping the shape its light is
        desc = built.desc
        pts = _np(plain["point"])[hit]
        li = np.arange(len(pts)) % desc.n_lights
        centre = np.array([list(desc.lights[i].center) for i in range(desc.n_lights)])
        skip = np.array([desc.lights[i].shape_index for i in range(desc.n_lights)], np.int32)
        a = (np.ascontiguousarray(pts), np.ascontiguousarray(centre[li] - pts), np.ascontiguousarray(skip[li]))
        occ0, so0 = dt.rays_occluded(scene, g, _cuda(a[0]), _cuda(a[1]), skip_shape=_cuda(a[2]))
        frac = float(_np(occ0).mean())
        assert 0.05 < frac < 0.95 and len(set(a[2].tolist())) > 2, frac
        occ, so = dt.rays_occluded(scene, g, _cuda(a[0]), _cuda(a[1]), skip_shape=_cuda(a[2]), order=True)
        assert occ.is_cuda and so.shadow_rays == so0.shadow_rays == len(pts) and so.rays == so0.rays
        _same(occ, occ0, "rays_occluded, device arrays")
        occ, so = dt.rays_occluded(scene, g, *a[:2], skip_shape=a[2], order=True)
        assert isinstance(occ, np.ndarray) and so.shadow_rays == so0.shadow_rays
        _same(occ, occ0, "rays_occluded, host arrays")
        occ, _ = dt.rays_occluded(scene, g, _cuda(a[0]), _cuda(a[1]), order=True)   # no skip_shape
        _same(occ, dt.rays_occluded(scene, g, _cuda(a[0]), _cuda(a[1]))[0], "rays_occluded, no skip_shape")
    finally:
        scene.close()
