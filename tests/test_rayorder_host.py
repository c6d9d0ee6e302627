"""Ray ordering, the host half (include/dt.h dt_ray_order_key, dt_ray_order, dt_permute_rows). No GPU.

1. dt_ray_order_key and the keys and the box of the host dt_ray_order equal the numpy restatement
   (tests/rayorder_ref.py) by bit pattern, on the scattered rays of tests/test_gpu_rayquery.py's recipe and on
   hand-made vectors, for each bit configuration; the test first asserts that its inputs hold each case.
2. perm is numpy's stable argsort of the keys; dt_permute_rows gathers and puts back rows of 1, 4 and 24 bytes
   and refuses a perm entry that is out of range.
3. Every argument error returns its code and a message with the function's prefix that names the argument.
(The issue asks the GPU test for B = 1; 3*origin_bits + 2*dir_bits cannot be 1, the smallest B is 2.)"""
import ctypes
import functools
import re

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd import _lib
from distraytracer_amd._lib import EXPORTS, RayOrderParams

import rayorder_ref as R

INVALID, LIMIT = -1, -6
key_inputs = functools.lru_cache(maxsize=None)(R.key_inputs)


def params(ob, db, major, box=None):
    p = dt.ray_order_params_default()
    p.origin_bits, p.dir_bits, p.dir_major = ob, db, major
    if box is not None:
        p.box_given = 1
        for k in range(3):
            p.box_lo[k], p.box_hi[k] = box[0][k], box[1][k]
    return p


def _err():
    return dt.lib.dt_last_error().decode()


def test_exports_struct_and_defaults():
    for name in ("dt_ray_order_params_default", "dt_ray_order_key", "dt_ray_order_workspace_bytes", "dt_ray_order",
                 "dt_permute_rows"):
        assert name in EXPORTS and hasattr(dt.lib, name)
    assert dt.lib.dt_abi_version() == 8
    assert ctypes.sizeof(RayOrderParams) == 4 * 4 + 6 * 8
    p = dt.ray_order_params_default()
    assert (p.origin_bits, p.dir_bits, p.dir_major, p.box_given) == (5, 6, 0, 0)
    hdr = open(_lib.REPO_ROOT + "/include/dt.h").read()
    assert int(re.search(r"#define DT_RAY_ORDER_TILE (\d+)", hdr).group(1)) == dt.DT_RAY_ORDER_TILE
    assert dt.lib.dt_ray_order_workspace_bytes(0) == 0
    n = 64 * dt.DT_RAY_ORDER_TILE + 37
    assert dt.lib.dt_ray_order_workspace_bytes(n) >= 12 * n + 4 * 256 * 65


def test_the_inputs_hold_each_case():
    hs, hd, tags = R.hand_made_rays()
    void = R.void_rays(hs, hd)
    assert {t for t in tags[void]} == {"void nan start", "void inf start", "void nan dir", "void inf dir", "void zero dir"}
    live = ~void
    assert (hd[live][:, 2] < 0).sum() >= 4
    assert {tuple(np.nonzero(d)[0]) for d in hd[tags == "axis-aligned"]} == {(0,), (1,), (2,)}
    with np.errstate(all="ignore"):
        s = np.abs(hd).sum(axis=1)
        u, v = hd[:, 0] / s, hd[:, 1] / s
        assert {1.0, -1.0} <= set(u[live].tolist()) and {1.0, -1.0} <= set(v[live].tolist())
        assert np.isinf(s[tags == "huge s"]).all() and np.isfinite(hd[tags == "huge s"]).all()
        lo, hi = R.box_of(hs, hd)
        assert np.isinf(hi - lo).all() and np.isfinite(hs[live]).all()   # e and o - lo overflow
        assert np.isinf(hs[tags == "huge o - lo"] - lo).any()
    room = key_inputs()[3][3]
    assert (hs[live] < room[0]).any() and (hs[live] > room[1]).any()   # outside the given box on either side
    eq = key_inputs()[5][1]
    assert (eq == eq[0]).all()
    ss, sd = key_inputs()[0][1:3]
    assert len(ss) == 4096 + 37 and not R.void_rays(ss, sd).any() and (sd[:, 2] < 0).any() and (sd[:, 2] > 0).any()
    assert R.void_rays(*key_inputs()[6][1:3]).all()


@pytest.mark.parametrize("cfg", R.CONFIGS, ids=lambda c: "ob%d-db%d-%s" % (c[0], c[1], "dir" if c[2] else "origin"))
def test_keys_box_and_order_equal_the_restatement(cfg):
    ob, db, major = cfg
    for name, start, dir, box in key_inputs():
        p = params(ob, db, major, box)
        lo, hi = box if box is not None else R.box_of(start, dir)
        want = R.keys_of(start, dir, ob, db, major, lo, hi)
        order = dt.ray_order(start, dir, params=p, keys=True)
        assert order.keys.dtype == np.uint32 and order.perm.dtype == np.uint32 and order.kernel_ms == 0.0
        assert np.array(order.box).tobytes() == np.concatenate([lo, hi]).tobytes(), (name, order.box, lo, hi)
        bad = np.nonzero(order.keys != want)[0]
        assert bad.size == 0, "%s ray %d (%r, %r): library %d, restatement %d" % (
            name, bad[0], start[bad[0]], dir[bad[0]], order.keys[bad[0]], want[bad[0]])
        assert (want <= np.uint32(1 << (3 * ob + 2 * db))).all()
        assert ((want == np.uint32(1 << (3 * ob + 2 * db))) == R.void_rays(start, dir)).all()
        assert np.array_equal(order.perm, R.order_of(want)), name
        if len(start) < 100:   # the single-ray export, ray by ray
            for i in range(len(start)):
                assert dt.ray_order_key(p, lo, hi, start[i], dir[i]) == want[i], (name, i)
    ss, sd = key_inputs()[0][1:3]
    lo, hi = R.box_of(ss, sd)
    want = R.keys_of(ss, sd, ob, db, major, lo, hi)
    p = params(ob, db, major)
    for i in range(0, len(ss), 97):
        assert dt.ray_order_key(p, lo, hi, ss[i], sd[i]) == want[i]
    assert len(set(want.tolist())) > (100 if 3 * ob + 2 * db >= 16 else 1)   # the keys do tell the scattered rays apart


def test_order_without_keys_and_of_no_rays():
    ss, sd = key_inputs()[0][1:3]
    a, b = dt.ray_order(ss, sd), dt.ray_order(ss, sd, keys=True)
    assert a.keys is None and np.array_equal(a.perm, b.perm)
    none = dt.ray_order(np.zeros((0, 3)), np.zeros((0, 3)), keys=True)
    assert none.n == 0 and len(none.perm) == 0 and len(none.keys) == 0 and none.box == (0.0,) * 6
    assert len(none.apply(np.zeros((0, 3)))) == 0


@pytest.mark.parametrize("row", [1, 4, 24])
def test_permute_rows_gather_then_inverse_is_the_identity(row):
    ss, sd = key_inputs()[0][1:3]
    order = dt.ray_order(ss, sd)
    n = order.n
    rng = np.random.default_rng(row)
    a = {1: rng.integers(0, 256, n).astype(np.uint8), 4: rng.integers(-5, 60, n).astype(np.int32), 24: ss}[row]
    assert a.nbytes == row * n
    got = order.apply(a)
    assert np.array_equal(got, a[order.perm]) and got.dtype == a.dtype and got.shape == a.shape
    back = order.restore(got)
    assert back.tobytes() == a.tobytes()
    out = np.empty_like(a)
    assert order.restore(got, out=out) is out and out.tobytes() == a.tobytes()
    flat = order.apply(a.reshape(-1))   # flat arrays are rows as well
    assert flat.tobytes() == got.tobytes()


def test_permute_rows_odd_sizes_and_unaligned_rows():
    rng = np.random.default_rng(5)
    n = 1000
    perm = rng.permutation(n).astype(np.uint32)
    for row in (3, 12, 20, 64):
        a = rng.integers(0, 256, (n, row)).astype(np.uint8)
        out = np.zeros_like(a)
        assert dt.lib.dt_permute_rows(n, row, perm.ctypes.data, a.ctypes.data, out.ctypes.data, 0, 0, None) == 0
        assert np.array_equal(out, a[perm])
        back = np.zeros_like(a)
        assert dt.lib.dt_permute_rows(n, row, perm.ctypes.data, out.ctypes.data, back.ctypes.data, 1, 0, None) == 0
        assert np.array_equal(back, a)


def test_permute_rows_errors():
    n = 8
    perm = np.arange(n, dtype=np.uint32)
    a, b = np.zeros((n, 3)), np.zeros((n, 3))
    pp, pa, pb = (ctypes.c_void_p(x.ctypes.data) for x in (perm, a, b))

    def call(n=n, row=24, perm=pp, src=pa, dst=pb, inverse=0):
        return dt.lib.dt_permute_rows(n, row, perm, src, dst, inverse, 0, None)

    for kw, word in [(dict(perm=None), "null perm"), (dict(src=None), "null src"), (dict(dst=None), "null dst"),
                     (dict(n=-1), "n < 0"), (dict(row=0), "row_bytes"), (dict(row=65), "row_bytes"),
                     (dict(inverse=2), "inverse"), (dict(dst=pa), "overlap"),
                     (dict(dst=ctypes.c_void_p(a.ctypes.data + 24)), "overlap")]:
        assert call(**kw) == INVALID, word
        assert _err().startswith("dt_permute_rows: ") and word in _err(), (word, _err())
    perm[5] = n   # out of range: refused on the host, nothing is written
    b[:] = 7.0
    assert call() == INVALID and _err().startswith("dt_permute_rows: ") and "perm[5]" in _err(), _err()
    assert call(inverse=1) == INVALID and "perm[5]" in _err()
    assert (b == 7.0).all()
    assert call(n=0) == 0


def test_ray_order_errors_before_any_device_work():
    n = 4
    rays = np.ones((n, 3))
    pr = ctypes.c_void_p(rays.ctypes.data)
    perm = np.zeros(n, np.uint32)
    pp = ctypes.c_void_p(perm.ctypes.data)
    fake_ws = ctypes.c_void_p(256)   # never dereferenced: the argument checks come first

    def call(n=n, start=pr, dir=pr, p=dt.ray_order_params_default(), perm=pp, ws=None, dev=0):
        return dt.lib.dt_ray_order(n, start, dir, ctypes.byref(p) if p is not None else None, perm, None, None, ws, dev,
                                   None, None)

    def bad_box(lo, hi):
        return params(5, 6, 0, (lo, hi))

    cases = [(dict(start=None), "null start"), (dict(dir=None), "null dir"), (dict(p=None), "null params"),
             (dict(perm=None), "null perm"), (dict(dev=1, ws=None), "null workspace"), (dict(n=-1), "n_rays < 0"),
             (dict(p=params(11, 0, 0)), "origin_bits"), (dict(p=params(-1, 6, 0)), "origin_bits"),
             (dict(p=params(0, 9, 0)), "dir_bits"), (dict(p=params(0, -1, 0)), "dir_bits"),
             (dict(p=params(0, 0, 0)), "key bits"), (dict(p=params(10, 1, 0)), "key bits"),
             (dict(p=params(5, 6, 2)), "dir_major"),
             (dict(p=bad_box((0, 0, np.nan), (1, 1, 1))), "not finite"),
             (dict(p=bad_box((0, 0, 0), (1, np.inf, 1))), "not finite"),
             (dict(p=bad_box((0, 2, 0), (1, 1, 1))), "box_lo > box_hi")]
    for dev in (0, 1):
        for kw, word in cases:
            kw = dict(kw)
            kw.setdefault("dev", dev)
            if kw["dev"]:
                kw.setdefault("ws", fake_ws)
            assert call(**kw) == INVALID, word
            assert _err().startswith("dt_ray_order: ") and word in _err(), (word, _err())
        assert call(n=(1 << 30) + 1, dev=dev, ws=fake_ws) == LIMIT
        assert _err().startswith("dt_ray_order: ") and "n_rays" in _err()
        assert call(n=0, dev=dev, ws=fake_ws) == 0   # nothing is launched
    key = ctypes.c_uint32()
    D3 = _lib.D3
    assert dt.lib.dt_ray_order_key(ctypes.byref(params(11, 0, 0)), D3(), D3(), D3(), D3(), ctypes.byref(key)) == INVALID
    assert _err().startswith("dt_ray_order_key: ") and "origin_bits" in _err()
    assert dt.lib.dt_ray_order_key(None, D3(), D3(), D3(), D3(), ctypes.byref(key)) == INVALID
    assert dt.lib.dt_ray_order_key(ctypes.byref(params(5, 6, 0)), D3(), D3(), D3(), D3(), None) == INVALID


class _NoScene:
    handle = None


def test_wrappers_check_their_arguments():
    ss, sd = key_inputs()[0][1:3]
    g = dt.globals_default()
    order = dt.ray_order(ss[:100].copy(), sd[:100].copy())
    with pytest.raises(dt.DTError, match="order must be True or a RayOrder"):
        dt.trace_rays(_NoScene, g, ss, sd, order=order)   # an order of other rays
    with pytest.raises(dt.DTError, match="order must be True or a RayOrder"):
        dt.rays_occluded(_NoScene, g, ss, sd, order=order.perm)
    with pytest.raises(dt.DTError, match="rows of 1..64 bytes"):
        order.apply(np.zeros((100, 9)))
    with pytest.raises(dt.DTError, match="rows of 1..64 bytes"):
        order.apply(np.zeros(99))
    with pytest.raises(dt.DTError, match="contiguous"):
        order.apply(np.zeros((100, 6))[:, ::2])
    with pytest.raises(dt.DTError, match="out must be"):
        order.restore(np.zeros(100, np.float32), out=np.zeros(100, np.int32))
    with pytest.raises(dt.DTError, match="3 doubles per ray"):
        dt.ray_order(np.zeros(10), np.zeros(10))
    # with an order the rays are gathered and reach the library, which refuses the null scene
    with pytest.raises(dt.DTError, match="dt_trace_rays: null scene"):
        dt.trace_rays(_NoScene, g, ss, sd, order=True)
    with pytest.raises(dt.DTError, match="dt_rays_occluded: null scene"):
        dt.rays_occluded(_NoScene, g, ss, sd, skip_shape=np.full(len(ss), -1, np.int32), order=dt.ray_order(ss, sd))
