"""Occlusion feature buffers, the host half (include/dt.h dt_occlusion_ao_ray, dt_occlusion_light_ray,
dt_occlusion_params_default, dt_render_occlusion): the two probe generators' host exports against their numpy
restatement (tests/occlusion_ref.py) bit for bit, and the DT_E_INVALID checks of dt_render_occlusion, which come
before any device work. No GPU.

dt_render_occlusion checks its arguments in the order scene, globals, params, out, n_samples, ao_rays, n_lights,
ao_radius, the planes, and looks at the scene only then (the light indices, the RectPrismWithCylinder). Where a
check other than the scene's is meant, the scene is a stand-in address that is never dereferenced, as in
tests/test_features_host.py. The light indices and DT_E_UNSUPPORTED need a scene, and a scene needs a device:
tests/test_gpu_occlusion.py."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
import occlusion_ref as R
from distraytracer_amd._lib import EXPORTS, LightDesc, Occlusion, OcclusionParams
from oracle import geom as G

INVALID = -1
N = 3000
D3 = ctypes.c_double * 3
SEED, FRAME = 12345, 7


def _inputs(seed):
    rng = np.random.default_rng(seed)
    pixel = rng.integers(0, 1920 * 1080, N)
    sample = rng.integers(0, 256, N)
    p = rng.uniform(-5, 5, size=(N, 3))
    n = rng.normal(size=(N, 3))
    n /= np.sqrt((n * n).sum(axis=1))[:, None]
    return rng, pixel, sample, p, n


def _light(kind):
    L = LightDesc()
    L.type, L.shape_index, L.radius = kind, 3, 0.3
    for a, (c, A, B, D) in enumerate(zip((0.25, 3.5, 1.0), (-1.0, 4.0, -1.0), (1.0, 4.0, -1.0), (-1.0, 4.0, 1.5))):
        L.center[a], L.A[a], L.B[a], L.D[a] = c, A, B, D
    return L


def _host_ao(pixel, sample, r, radius, p, n):
    out = np.zeros((len(pixel), 3))
    for i in range(len(pixel)):
        d = D3()
        assert dt.lib.dt_occlusion_ao_ray(SEED, FRAME, int(pixel[i]), int(sample[i]), int(r[i]), radius, D3(*p[i]),
                                          D3(*n[i]), d) == 0
        out[i] = tuple(d)
    return out


def test_ao_ray_is_the_numpy_rule():
    rng, pixel, sample, p, n = _inputs(1)
    r = rng.integers(0, 16, N)
    radius = 0.37
    want = R.ao_dir(SEED, FRAME, pixel, sample, r, radius, n)
    got = _host_ao(pixel, sample, r, radius, p, n)
    assert not G.differs(got.reshape(-1), want.reshape(-1)).any()
    # the probe points into the ball resting on the surface: |dir/R - n| <= 1
    v = want / float(np.float32(radius)) - n
    assert ((v * v).sum(axis=1) <= 1 + 1e-12).all() and (want != 0).any(axis=1).all()
    # the Python wrapper is the same call
    g = dt.globals_default()
    g.seed = SEED
    assert dt.occlusion_ao_ray(g, FRAME, pixel[0], sample[0], r[0], radius, p[0], n[0]) == tuple(want[0])


@pytest.mark.parametrize("kind", [R.POINT, R.SPHERE, R.RECT], ids=["point", "sphere", "rect"])
def test_light_ray_is_the_numpy_rule(kind):
    rng, pixel, sample, p, n = _inputs(2 + kind)
    j = rng.integers(0, 8, N)
    L = _light(kind)
    want = R.light_dir(SEED, FRAME, pixel, sample, j, L, p)
    got = np.zeros((N, 3))
    for i in range(N):
        d = D3()
        assert dt.lib.dt_occlusion_light_ray(SEED, FRAME, int(pixel[i]), int(sample[i]), int(j[i]), ctypes.byref(L),
                                             D3(*p[i]), d) == 0
        got[i] = tuple(d)
    assert not G.differs(got.reshape(-1), want.reshape(-1)).any()
    T = want + p
    C = np.array(list(L.center))
    if kind == R.POINT:
        assert (np.abs(T - C) < 1e-12).all()
    elif kind == R.SPHERE:   # a point of the light's volume, and not one point
        d2 = ((T - C) ** 2).sum(axis=1)
        assert (d2 <= float(np.float32(0.3)) ** 2 * (1 + 1e-9)).all() and len(np.unique(T[:, 0])) > N // 2
    else:                    # a point of the rectangle's frame: y = 4, x in [-1, 1], z in [-1, 1.5]
        e = 1e-9   # T is dir + p again: one more rounding
        assert (np.abs(T[:, 1] - 4.0) < e).all() and (np.abs(T[:, 0]) <= 1 + e).all()
        assert (T[:, 2] >= -1 - e).all() and (T[:, 2] <= 1.5 + e).all()
        # slot j enters the counter: the same sample under two slots aims at two points
        other = R.light_dir(SEED, FRAME, pixel, sample, (j + 1) % 8, L, p)
        assert (other != want).any(axis=1).all()
    g = dt.globals_default()
    g.seed = SEED
    assert dt.occlusion_light_ray(g, FRAME, pixel[0], sample[0], j[0], L, p[0]) == tuple(want[0])


def test_a_rejected_first_try_moves_to_the_next_draw():
    """the retry index: a sample whose try 0 lies outside the ball (s > 1), found by search"""
    pixel, sample = np.full(64, 4242), np.arange(64)
    v, tries = R.ball(SEED, FRAME, pixel, sample, R.P_AO, 5)
    assert (tries > 0).any() and (tries == 0).any() and (tries < R.TRIES).all()
    i = int(np.nonzero(tries > 0)[0][0])
    o = R.words(SEED, FRAME, [4242], [i], R.P_AO, 5 * 16)[0].astype(np.float64) * 2.0 ** -31 - 1.0
    assert (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2] > 1.0
    o = R.words(SEED, FRAME, [4242], [i], R.P_AO, 5 * 16 + int(tries[i]))[0].astype(np.float64) * 2.0 ** -31 - 1.0
    assert tuple(o[:3]) == tuple(v[i]) and (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2] <= 1.0
    n = np.array([[0.0, 1.0, 0.0]])
    d = D3()
    assert dt.lib.dt_occlusion_ao_ray(SEED, FRAME, 4242, i, 5, 2.0, D3(0, 0, 0), D3(*n[0]), d) == 0
    assert tuple(d) == tuple(R.ao_rule(2.0, n, v[i:i + 1])[0])


def test_the_void_probe():
    """v = -n gives a zero direction, which dt_rays_occluded's rule never traces"""
    from rayquery_ref import void_rays
    v = np.array([[0.25, -0.5, 0.75], [0.0, 0.0, 0.0]])
    d = R.ao_rule(1.5, -v, v)
    assert (d == 0).all() and void_rays(np.zeros((2, 3)), d).all()
    assert not void_rays(np.zeros((1, 3)), R.ao_rule(1.5, [[0, 1.0, 0]], [[0, 0, 0]])).any()


def test_generator_argument_errors():
    v = D3(0, 0, 1)
    args = [SEED, FRAME, 1, 2, 0, 1.0, v, v, v]
    for k in (6, 7, 8):
        a = list(args)
        a[k] = None
        assert dt.lib.dt_occlusion_ao_ray(*a) == INVALID and b"dt_occlusion_ao_ray: null" in dt.lib.dt_last_error()
    for r in (-1, 16):
        a = list(args)
        a[4] = r
        assert dt.lib.dt_occlusion_ao_ray(*a) == INVALID and b"dt_occlusion_ao_ray: r " in dt.lib.dt_last_error()
    L = _light(R.POINT)
    args = [SEED, FRAME, 1, 2, 0, ctypes.byref(L), v, v]
    for k in (5, 6, 7):
        a = list(args)
        a[k] = None
        assert dt.lib.dt_occlusion_light_ray(*a) == INVALID and b"dt_occlusion_light_ray: null" in dt.lib.dt_last_error()
    for j in (-1, 8):
        a = list(args)
        a[4] = j
        assert dt.lib.dt_occlusion_light_ray(*a) == INVALID and b"dt_occlusion_light_ray: j " in dt.lib.dt_last_error()


def test_params_default_and_exports():
    p = dt.occlusion_params_default()
    assert (p.ao_rays, p.n_lights, p.ao_radius) == (4, 0, 1.0) and list(p.lights) == [0] * 8
    dt.lib.dt_occlusion_params_default(None)   # a null pointer is ignored
    for name in ("dt_occlusion_params_default", "dt_render_occlusion", "dt_occlusion_ao_ray", "dt_occlusion_light_ray"):
        assert name in EXPORTS and hasattr(dt.lib, name)
    assert dt.lib.dt_abi_version() == 8
    assert ctypes.sizeof(OcclusionParams) == 12 + 4 * 8 and ctypes.sizeof(Occlusion) == 16


def _call(scene, g, n, p, o):
    st = dt.Stats()
    return dt.lib.dt_render_occlusion(scene, ctypes.byref(g) if g is not None else None, 0, None, n,
                                      ctypes.byref(p) if p is not None else None,
                                      ctypes.byref(o) if o is not None else None, 0, None, ctypes.byref(st))


def test_argument_errors_come_before_any_device_work():
    g = dt.globals_default()
    g.xRes, g.yRes, g.antialias_samples = 40, 24, 256
    ao, light = np.zeros(40 * 24, np.float32), np.zeros(40 * 24 * 8, np.float32)
    scene = ctypes.c_void_p(0x1000)   # a stand-in: never dereferenced by the checks below

    def params(**kw):
        p = dt.occlusion_params_default()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    both = Occlusion(ao.ctypes.data, light.ctypes.data)
    only_ao = Occlusion(ao.ctypes.data, None)
    cases = [
        (None, g, 64, params(), only_ao, b"null scene"),
        (scene, None, 64, params(), only_ao, b"null globals"),
        (scene, g, 64, None, only_ao, b"null params"),
        (scene, g, 64, params(), None, b"null out"),
        (scene, g, 100, params(), only_ao, b"n_samples"),
        (scene, g, 0, params(), only_ao, b"n_samples"),
        (scene, g, 64, params(ao_rays=-1), only_ao, b"ao_rays"),
        (scene, g, 64, params(ao_rays=17), only_ao, b"ao_rays"),
        (scene, g, 64, params(n_lights=-1), only_ao, b"n_lights"),
        (scene, g, 64, params(n_lights=9), only_ao, b"n_lights"),
        (scene, g, 64, params(ao_radius=0.0), only_ao, b"ao_radius"),
        (scene, g, 64, params(ao_radius=-1.0), only_ao, b"ao_radius"),
        (scene, g, 64, params(ao_radius=float("inf")), only_ao, b"ao_radius"),
        (scene, g, 64, params(ao_radius=float("nan")), only_ao, b"ao_radius"),
        (scene, g, 64, params(ao_rays=0, n_lights=1), both, b"out->ao given with ao_rays == 0"),
        (scene, g, 64, params(), both, b"out->light given with n_lights == 0"),
        (scene, g, 64, params(), Occlusion(None, None), b"every pointer is null"),
    ]
    for sc, gg, n, p, o, msg in cases:
        assert _call(sc, gg, n, p, o) == INVALID, msg
        err = dt.lib.dt_last_error()
        assert err.startswith(b"dt_render_occlusion: ") and msg in err, (msg, err)
