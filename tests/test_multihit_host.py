"""Multi-hit ray queries, the host half (include/dt.h dt_trace_rays_multi). No GPU.

1. The struct layout against gcc, the export, the ABI version.
2. Every argument error returns its code and a message that starts with the function's name and names the
   argument, before any device work: the scene is a stand-in address that is never dereferenced where another
   check is meant (tests/test_rayquery_host.py). DT_E_UNSUPPORTED on prismcyl and n_rays == 0 read the scene,
   and a scene cannot be made without a device: they are in tests/test_gpu_multihit.py, as its neighbours'.
3. The wrappers reject bad shapes, dtypes and k before the library sees them.
4. The prediction the GPU tests compare with (tests/multihit_ref.py) against the project's pinned loop: on the
   rays tests/test_rayquery_host.py pins to the oracle, k = 1 equals RayQueryRef.trace's shape and t on every
   ray whose smallest t is unique and that saw no edge-on return -- at least 99% of the hitting rays, so the
   check cannot pass by exclusion."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd import _lib
from distraytracer_amd._lib import EXPORTS, RayMultiHits
from oracle import geom as G

import multihit_ref
from rayquery_ref import FLT_MAX, RayQueryRef
from test_gpu_features import MIXED_AT, MIXED_EYE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "dt.h")
INVALID = -1
FIELDS = ["count", "shape", "t", "point", "normal", "albedo"]


def test_export_struct_and_version():
    assert "dt_trace_rays_multi" in EXPORTS and hasattr(dt.lib, "dt_trace_rays_multi")
    assert dt.lib.dt_abi_version() == 8
    assert _lib.DT_MULTIHIT_MAX == 8
    assert [f for f, _ in RayMultiHits._fields_] == FIELDS


def test_struct_layout_matches_c(tmp_path):
    """offsetof/sizeof of every field and DT_MULTIHIT_MAX, from gcc on include/dt.h, vs the ctypes mirror"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){",
             'printf("size %zu\\n", sizeof(dt_ray_multihits));', 'printf("max %d\\n", DT_MULTIHIT_MAX);']
    for f in FIELDS:
        lines.append('printf("%s %%zu\\n", offsetof(dt_ray_multihits, %s));' % (f, f))
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(c)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(RayMultiHits)
    assert int(got["max"]) == _lib.DT_MULTIHIT_MAX
    for f in FIELDS:
        assert int(got[f]) == getattr(RayMultiHits, f).offset, f


def _err():
    return dt.lib.dt_last_error().decode()


def _call(scene, gg, n, start, dir, k, out, st):
    return dt.lib.dt_trace_rays_multi(scene, ctypes.byref(gg) if gg is not None else None, n, start, dir, k,
                                      ctypes.byref(out) if out is not None else None, 0, None, ctypes.byref(st))


def test_argument_errors_before_any_device_work():
    g = dt.globals_default()
    fake = ctypes.c_void_p(64)
    rays = np.zeros((4, 3))
    p = ctypes.c_void_p(rays.ctypes.data)
    count = np.zeros(4, np.int32)
    h = RayMultiHits()
    h.count = count.ctypes.data
    st = dt.Stats()
    for args, word in [((None, g, 4, p, p, 2, h), "null scene"), ((fake, None, 4, p, p, 2, h), "null globals"),
                       ((fake, g, 4, None, p, 2, h), "null start"), ((fake, g, 4, p, None, 2, h), "null dir"),
                       ((fake, g, 4, p, p, 2, None), "null out"), ((fake, g, 4, p, p, 2, RayMultiHits()), "no plane"),
                       ((fake, g, -1, p, p, 2, h), "n_rays < 0"), ((fake, g, 4, p, p, 0, h), "k = 0"),
                       ((fake, g, 4, p, p, 9, h), "k = 9"), ((fake, g, 4, p, p, -3, h), "k = -3")]:
        assert _call(*args, st) == INVALID, word
        assert _err().startswith("dt_trace_rays_multi: ") and word in _err(), (word, _err())


class _NoScene:
    handle = None


def test_wrappers_check_their_arguments():
    g = dt.globals_default()
    ok = np.zeros((4, 3))
    with pytest.raises(dt.DTError, match="float64"):
        dt.trace_rays_multi(_NoScene, g, ok.astype(np.float32), ok)
    with pytest.raises(dt.DTError, match="3 doubles per ray"):
        dt.trace_rays_multi(_NoScene, g, np.zeros(10), np.zeros(10))
    with pytest.raises(dt.DTError, match="same number of rays"):
        dt.trace_rays_multi(_NoScene, g, ok, np.zeros((5, 3)))
    with pytest.raises(dt.DTError, match="unknown plane"):
        dt.trace_rays_multi(_NoScene, g, ok, ok, planes=("depth",))
    for k in (0, 9, -1, 2.0, True, None):
        with pytest.raises(dt.DTError, match="k must be an integer in 1..8"):
            dt.trace_rays_multi(_NoScene, g, ok, ok, k=k)
    with pytest.raises(dt.DTError, match="order must be True or a RayOrder"):
        dt.trace_rays_multi(_NoScene, g, ok, ok, order=3)
    # rightly shaped arrays, (n, 3) or flat, reach the library, which refuses the null scene
    with pytest.raises(dt.DTError, match="dt_trace_rays_multi: null scene"):
        dt.trace_rays_multi(_NoScene, g, ok, ok.reshape(-1), k=8)
    with pytest.raises(dt.DTError, match="dt_trace_rays_multi: out wants no plane"):
        dt.trace_rays_multi(type("S", (), {"handle": ctypes.c_void_p(64)}), g, ok, ok, planes=())


def _final(W, H):
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes = W, H
    return g, built


def _k1_against_the_pinned_loop(g, built, first, n):
    start, ray = G.or_primary_ray(g, 240, first, n)
    ref = RayQueryRef(built, g)
    want, _ = ref.trace(start, ray, attrs=False)
    hits, edge = multihit_ref.all_hits(ref, start, ray)
    got, seen = multihit_ref.predict(ref, start, ray, 1, attrs=False, hits_edge=(hits, edge))
    ts = [sorted(h[0] for h in hs or ()) for hs in hits]
    unique = np.array([len(t) < 2 or t[0] < t[1] for t in ts])
    keep = unique & (edge == 0)
    hitting = want["shape"] >= 0
    print("rays %d..%d: %d hit, %d of them kept (%d tied at the front, %d saw an edge-on return)" % (
        first, first + n, int(hitting.sum()), int((keep & hitting).sum()), int((~unique).sum()), int((edge > 0).sum())))
    assert hitting.any() and (keep & hitting).sum() >= 0.99 * hitting.sum()
    bad = np.nonzero(keep & (G.differs(got["shape"][:, 0], want["shape"]) | G.differs(got["t"][:, 0], want["t"])))[0]
    assert bad.size == 0, "ray %d: multihit_ref (%d, %r), RayQueryRef.trace (%d, %r)" % (
        first + bad[0], got["shape"][bad[0], 0], got["t"][bad[0], 0], want["shape"][bad[0]], want["t"][bad[0]])
    assert ((got["count"] == 1) == (seen["total"] > 0)).all()
    assert (got["t"][got["count"] == 0, 0] == FLT_MAX).all()
    return hitting


def test_k1_is_the_pinned_loop_c3_window():
    """final(240) at 1920x1080: the 2048 rays from the middle of the frame that tests/test_rayquery_host.py pins"""
    g, built = _final(1920, 1080)
    _k1_against_the_pinned_loop(g, built, 1920 * 1080 * 8 // 2, 2048)


def test_k1_is_the_pinned_loop_mixed_camera():
    """the 40x24 camera whose lens straddles a wall: hits and misses"""
    g, built = _final(40, 24)
    for a in range(3):
        g.eye[a], g.lookingAt[a] = MIXED_EYE[a], MIXED_AT[a]
    hitting = _k1_against_the_pinned_loop(g, built, 0, 40 * 24 * 8)
    assert (~hitting).any()
