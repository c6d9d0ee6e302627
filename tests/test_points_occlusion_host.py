"""Occlusion queries at surface points, the host half (include/dt.h dt_points_occlusion; distraytracer_amd
shape_texels): the export, the DT_E_INVALID checks, which come before any device work, and the texel centres and
normals of shape_texels against values computed by hand. No GPU.

dt_points_occlusion checks its arguments in the order scene, globals, point, normal, params, out, n_points,
n_samples, then dt_render_occlusion's rules for params and out, and looks at the scene only after those (the
light indices, the RectPrismWithCylinder). The scene is a stand-in address that is never dereferenced, as in
tests/test_occlusion_host.py. The light indices, DT_E_UNSUPPORTED and n_points == 0 need a scene, and a scene
needs a device: tests/test_gpu_points_occlusion.py."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
import scene_gen
from distraytracer_amd._lib import DT_POCCL_MAX_SAMPLES, EXPORTS, Occlusion

INVALID = -1


def test_the_export_exists():
    assert "dt_points_occlusion" in EXPORTS and hasattr(dt.lib, "dt_points_occlusion")
    assert dt.lib.dt_abi_version() == 8 and DT_POCCL_MAX_SAMPLES == 1024
    for name in ("points_occlusion", "shape_texels", "bake_occlusion"):
        assert name in dt.__all__ and callable(getattr(dt, name))


def _call(scene, g, n_points, point, normal, n_samples, p, o):
    st = dt.Stats()
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    return dt.lib.dt_points_occlusion(scene, ctypes.byref(g) if g is not None else None, 0, n_points, ptr(point),
                                      ptr(normal), n_samples, ctypes.byref(p) if p is not None else None,
                                      ctypes.byref(o) if o is not None else None, 0, None, ctypes.byref(st))


def test_argument_errors_come_before_any_device_work():
    g = dt.globals_default()
    N = 5
    pt, nm = np.zeros((N, 3)), np.tile([0.0, 1.0, 0.0], (N, 1))
    ao, light = np.zeros(N, np.float32), np.zeros(N * 8, np.float32)
    scene = ctypes.c_void_p(0x1000)   # a stand-in: never dereferenced by the checks below

    def params(**kw):
        p = dt.occlusion_params_default()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    both = Occlusion(ao.ctypes.data, light.ctypes.data)
    only_ao = Occlusion(ao.ctypes.data, None)
    ok = dict(scene=scene, g=g, n_points=N, point=pt, normal=nm, n_samples=4, p=params(), o=only_ao)
    cases = [
        (dict(scene=None), b"null scene"),
        (dict(g=None), b"null globals"),
        (dict(point=None), b"null point"),
        (dict(normal=None), b"null normal"),
        (dict(p=None), b"null params"),
        (dict(o=None), b"null out"),
        (dict(n_points=-1), b"n_points < 0"),
        (dict(n_points=2 ** 32), b"n_points >= 2^32"),
        (dict(n_points=2 ** 40), b"n_points >= 2^32"),
        (dict(n_samples=0), b"n_samples 0 outside 1..1024"),
        (dict(n_samples=-3), b"n_samples -3 outside 1..1024"),
        (dict(n_samples=1025), b"n_samples 1025 outside 1..1024"),
        (dict(p=params(ao_rays=-1)), b"ao_rays"),
        (dict(p=params(ao_rays=17)), b"ao_rays"),
        (dict(p=params(n_lights=-1)), b"n_lights"),
        (dict(p=params(n_lights=9)), b"n_lights"),
        (dict(p=params(ao_radius=0.0)), b"ao_radius"),
        (dict(p=params(ao_radius=-1.0)), b"ao_radius"),
        (dict(p=params(ao_radius=float("inf"))), b"ao_radius"),
        (dict(p=params(ao_radius=float("nan"))), b"ao_radius"),
        (dict(p=params(ao_rays=0, n_lights=1), o=both), b"out->ao given with ao_rays == 0"),
        (dict(o=both), b"out->light given with n_lights == 0"),
        (dict(o=Occlusion(None, None)), b"every pointer is null"),
        # the errors also come before the n_points == 0 shortcut
        (dict(n_points=0, n_samples=0), b"n_samples"),
    ]
    for change, msg in cases:
        assert _call(**dict(ok, **change)) == INVALID, msg
        err = dt.lib.dt_last_error()
        assert err.startswith(b"dt_points_occlusion: ") and msg in err, (msg, err)


def _scene():
    """a unit rectangle in the plane y = 0, a triangle in the plane z = 0 and a sphere"""
    b = scene_gen._Builder(1.0, (0.0, 0.0, 0.0))
    rect = scene_gen._rect(b, (0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1), (0.5, 0.5, 0.5))
    tri = scene_gen._triangle(b, (0, 0, 0), (2, 0, 0), (0, 2, 0), (0.5, 0.5, 0.5))
    sph = b.shape(scene_gen.SPHERE, v=[(0, 1, 0)], radius=0.5, color=(1, 1, 1), center=(0, 1, 0))
    checker = b.shape(scene_gen.CHECKER, v=[(1, 1, 1), (3, 1, 1), (3, 1, 5), (1, 1, 5)], color=(0.5, 0.5, 0.5),
                      color1=(1, 1, 1), color2=(0, 0, 0), S=1.0, length=2.0, width=4.0, center=(2, 1, 3))
    desc, keep = b.desc()
    return desc, keep, rect, tri, sph, checker


def test_shape_texels_of_a_unit_rectangle():
    desc, keep, rect, tri, sph, checker = _scene()
    p, n = dt.shape_texels(desc, rect, 2, 2)
    assert p.dtype == n.dtype == np.float64 and p.shape == n.shape == (4, 3)
    # texel (u, v) at row v*2 + u: A + ((u+0.5)/2)*(B-A) + ((v+0.5)/2)*(D-A), B-A = +x, D-A = +z
    assert np.array_equal(p, [[0.25, 0, 0.25], [0.75, 0, 0.25], [0.25, 0, 0.75], [0.75, 0, 0.75]])
    # cross(+x, +z) = -y
    assert np.array_equal(n, np.tile([0.0, -1.0, 0.0], (4, 1)))
    p2, n2 = dt.shape_texels(desc, rect, 2, 2, side=-1)
    assert np.array_equal(p2, p) and np.array_equal(n2, np.tile([0.0, 1.0, 0.0], (4, 1)))
    # a 4 x 1 strip: width divides e1 only
    p3, _ = dt.shape_texels(desc, rect, 4, 1)
    assert np.array_equal(p3, [[0.125, 0, 0.5], [0.375, 0, 0.5], [0.625, 0, 0.5], [0.875, 0, 0.5]])


def test_shape_texels_of_a_checkerboard():
    desc, keep, rect, tri, sph, checker = _scene()
    p, n = dt.shape_texels(desc, checker, 2, 4)
    assert p.shape == (8, 3)
    # A = (1, 1, 1), B - A = (2, 0, 0), D - A = (0, 0, 4): texel (1, 2) at row 5
    assert np.array_equal(p[0], [1.5, 1, 1.5]) and np.array_equal(p[5], [2.5, 1, 3.5])
    assert np.array_equal(n, np.tile([0.0, -1.0, 0.0], (8, 1)))


def test_shape_texels_of_a_triangle_drops_the_texels_outside():
    desc, keep, rect, tri, sph, checker = _scene()
    p, n = dt.shape_texels(desc, tri, 2, 2)
    # frame B-A = (2, 0, 0), C-A = (0, 2, 0); (a, b) = (.25, .25), (.75, .25), (.25, .75) lie inside or on the
    # edge a + b = 1, (.75, .75) lies outside
    assert np.array_equal(p, [[0.5, 0.5, 0], [1.5, 0.5, 0], [0.5, 1.5, 0]])
    assert np.array_equal(n, np.tile([0.0, 0.0, 1.0], (3, 1)))
    p4, _ = dt.shape_texels(desc, tri, 4, 4)
    assert len(p4) == 10 and (p4[:, 0] / 2 + p4[:, 1] / 2 <= 1).all()   # 4 + 3 + 2 + 1 texel centres


def test_shape_texels_refuses_other_shapes():
    desc, keep, rect, tri, sph, checker = _scene()
    with pytest.raises(dt.DTError, match="shape_texels: shape %d is a sphere" % sph):
        dt.shape_texels(desc, sph, 2, 2)
    with pytest.raises(dt.DTError, match="the scene has 4 shapes"):
        dt.shape_texels(desc, 4, 2, 2)
    with pytest.raises(dt.DTError, match="width and height"):
        dt.shape_texels(desc, rect, 0, 2)
