"""Ray queries, the host half (include/dt.h dt_trace_rays, dt_rays_occluded). No GPU.

1. The prediction the GPU tests compare with (tests/rayquery_ref.py: the numpy restatement of the oracle's slab
   test and stack-order gather over oracle.bvh, the oracle's own shape tests) is pinned to the oracle's
   own loop: on the rays of or_primary_ray its shape and t equal oracle.primary_hit in every bit.
2. Every argument error returns its code and a message that starts with the function's name and names
   the argument, before any device work. Both calls check every argument before they look at the scene
   (dt_api.cpp): where a check other than the scene's is meant, the scene is a stand-in address that is
   never dereferenced, as in tests/test_features_host.py."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
import oracle
from distraytracer_amd._lib import EXPORTS, RayHits
from oracle import geom as G

from rayquery_ref import RayQueryRef
from test_gpu_features import MIXED_AT, MIXED_EYE

INVALID = -1


def _final(W, H):
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes = W, H
    return g, built


def _pinned(g, built, first, n):
    start, ray = G.or_primary_ray(g, 240, first, n)
    want_s, want_t = oracle.primary_hit(built, g, 240, first, n)
    got, _ = RayQueryRef(built, g).trace(start, ray, attrs=False)
    bad = np.nonzero(G.differs(got["shape"], want_s) | G.differs(got["t"], want_t))[0]
    print("rays %d..%d: %d hits, %d misses, %d differ" % (first, first + n, int((want_s >= 0).sum()),
                                                         int((want_s < 0).sum()), bad.size))
    assert bad.size == 0, "ray %d: restatement (%d, %r), or_primary_hit (%d, %r)" % (
        first + bad[0], got["shape"][bad[0]], got["t"][bad[0]], want_s[bad[0]], want_t[bad[0]])
    return want_s


def test_restatement_is_the_oracles_loop_c3_window():
    """final(240) at 1920x1080: 2048 rays from the middle of the frame"""
    g, built = _final(1920, 1080)
    shape = _pinned(g, built, 1920 * 1080 * 8 // 2, 2048)
    assert (shape >= 0).any()


def test_restatement_is_the_oracles_loop_mixed_camera():
    """the 40x24 camera of tests/test_gpu_features.py whose lens straddles a wall: hits and misses"""
    g, built = _final(40, 24)
    for a in range(3):
        g.eye[a], g.lookingAt[a] = MIXED_EYE[a], MIXED_AT[a]
    shape = _pinned(g, built, 0, 40 * 24 * 8)
    assert (shape >= 0).any() and (shape < 0).any()


def test_exports_and_struct():
    assert "dt_trace_rays" in EXPORTS and "dt_rays_occluded" in EXPORTS
    assert hasattr(dt.lib, "dt_trace_rays") and hasattr(dt.lib, "dt_rays_occluded")
    assert dt.lib.dt_abi_version() == 8
    assert ctypes.sizeof(RayHits) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert [f for f, _ in RayHits._fields_] == ["shape", "t", "point", "normal", "albedo"]


def _err():
    return dt.lib.dt_last_error().decode()


def test_trace_rays_argument_errors_before_any_device_work():
    g = dt.globals_default()
    fake = ctypes.c_void_p(64)
    rays = np.zeros((4, 3))
    p = ctypes.c_void_p(rays.ctypes.data)
    shape = np.zeros(4, np.int32)
    h = RayHits()
    h.shape = shape.ctypes.data
    st = dt.Stats()

    def call(scene, gg, n, start, dir, out):
        return dt.lib.dt_trace_rays(scene, ctypes.byref(gg) if gg is not None else None, n, start, dir,
                                    ctypes.byref(out) if out is not None else None, 0, None, ctypes.byref(st))

    for args, word in [((None, g, 4, p, p, h), "null scene"), ((fake, None, 4, p, p, h), "null globals"),
                       ((fake, g, 4, None, p, h), "null start"), ((fake, g, 4, p, None, h), "null dir"),
                       ((fake, g, 4, p, p, None), "null out"), ((fake, g, 4, p, p, RayHits()), "no plane"),
                       ((fake, g, -1, p, p, h), "n_rays < 0")]:
        assert call(*args) == INVALID, word
        assert _err().startswith("dt_trace_rays: ") and word in _err(), (word, _err())


def test_rays_occluded_argument_errors_before_any_device_work():
    g = dt.globals_default()
    fake = ctypes.c_void_p(64)
    rays = np.zeros((4, 3))
    p = ctypes.c_void_p(rays.ctypes.data)
    occ = np.zeros(4, np.uint8)
    o = ctypes.c_void_p(occ.ctypes.data)
    st = dt.Stats()

    def call(scene, gg, n, start, dir, out):
        return dt.lib.dt_rays_occluded(scene, ctypes.byref(gg) if gg is not None else None, n, start, dir, None, out,
                                       0, None, ctypes.byref(st))

    for args, word in [((None, g, 4, p, p, o), "null scene"), ((fake, None, 4, p, p, o), "null globals"),
                       ((fake, g, 4, None, p, o), "null start"), ((fake, g, 4, p, None, o), "null dir"),
                       ((fake, g, 4, p, p, None), "null occluded"), ((fake, g, -1, p, p, o), "n_rays < 0")]:
        assert call(*args) == INVALID, word
        assert _err().startswith("dt_rays_occluded: ") and word in _err(), (word, _err())


class _NoScene:
    handle = None


class _StandIn:   # never dereferenced: the argument checks come first
    handle = ctypes.c_void_p(64)


def test_wrappers_check_their_arrays():
    g = dt.globals_default()
    ok = np.zeros((4, 3))
    with pytest.raises(dt.DTError, match="float64"):
        dt.trace_rays(_NoScene, g, ok.astype(np.float32), ok)
    with pytest.raises(dt.DTError, match="3 doubles per ray"):
        dt.trace_rays(_NoScene, g, np.zeros(10), np.zeros(10))
    with pytest.raises(dt.DTError, match="same number of rays"):
        dt.rays_occluded(_NoScene, g, ok, np.zeros((5, 3)))
    with pytest.raises(dt.DTError, match="unknown plane"):
        dt.trace_rays(_NoScene, g, ok, ok, planes=("depth",))
    with pytest.raises(dt.DTError, match="t holds"):
        dt.trace_rays(_NoScene, g, ok, ok, out={"t": np.zeros(3, np.float32)})
    with pytest.raises(dt.DTError, match="int32"):
        dt.rays_occluded(_NoScene, g, ok, ok, skip_shape=np.zeros(4, np.int64))
    with pytest.raises(dt.DTError, match="uint8"):
        dt.rays_occluded(_NoScene, g, ok, ok, out=np.zeros(4, np.int32))
    # rightly shaped arrays, (n, 3) or flat, reach the library, which refuses the null scene
    with pytest.raises(dt.DTError, match="dt_trace_rays: null scene"):
        dt.trace_rays(_NoScene, g, ok, ok.reshape(-1))
    with pytest.raises(dt.DTError, match="dt_rays_occluded: null scene"):
        dt.rays_occluded(_NoScene, g, ok.reshape(-1), ok, skip_shape=np.full(4, -1, np.int32))
    with pytest.raises(dt.DTError, match="dt_trace_rays: out wants no plane"):
        dt.trace_rays(_StandIn, g, ok, ok, planes=())
