"""Irradiance queries at surface points (include/dt.h dt_points_irradiance), what needs no GPU: the exports and
constants, the two host exports dt_irradiance_gather_ray and dt_irradiance_cosine against numpy restatements,
every argument check that comes before the scene is looked at (shown as tests/test_aux_args_host.py shows it: a
stand-in scene that is never dereferenced, and the caller's stats left alone), and the prediction of
tests/points_irradiance_ref.py on a scene whose answer is known in closed form."""
import ctypes
import math

import numpy as np
import pytest

import distraytracer_amd as dt
import scene_gen
from distraytracer_amd import _lib
from distraytracer_amd._lib import (DT_OCCL_MAX_AO_RAYS, DT_OCCL_MAX_LIGHTS, DT_OCCL_TRIES, DT_POCCL_MAX_SAMPLES, EXPORTS,
                                    Irradiance, IrradianceParams)
from occlusion_ref import ball
from points_irradiance_ref import P_GATHER, PointsIrradianceRef

INVALID = -1
N = 5
STAND_IN = ctypes.c_void_p(0x1000)   # a scene that is never dereferenced
D3 = ctypes.c_double * 3


def test_exports_and_constants():
    for name in ("dt_points_irradiance", "dt_irradiance_gather_ray", "dt_irradiance_cosine"):
        assert name in EXPORTS and hasattr(dt.lib, name)
    assert dt.lib.dt_abi_version() == 8
    assert (DT_OCCL_MAX_AO_RAYS, DT_OCCL_MAX_LIGHTS, DT_OCCL_TRIES, DT_POCCL_MAX_SAMPLES) == (16, 8, 16, 1024)
    # dt_irradiance_params: n_lights, light[8], gather_rays; dt_irradiance: four pointers
    assert ctypes.sizeof(IrradianceParams) == 4 * (1 + DT_OCCL_MAX_LIGHTS + 1)
    assert IrradianceParams.gather_rays.offset == 4 * (1 + DT_OCCL_MAX_LIGHTS)
    assert [f for f, _ in Irradiance._fields_] == list(dt.IRRADIANCE_PLANES) == ["direct", "direct_rgb", "indirect_rgb", "sky"]


def _normalized(v):
    """dt_math.h normalized: v / sqrt((x*x + y*y) + z*z) if that is > 0"""
    s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    return v / math.sqrt(s) if s > 0 else v


def test_gather_ray_is_the_ball_points_direction_on_the_normal():
    g = dt.globals_default()
    g.seed = 12345
    p, n = np.array([0.25, -1.5, 3.0]), np.array([0.0, 0.6, 0.8])
    seen = 0
    for pixel, sample, r in [(0, 0, 0), (7, 3, 1), (129, 2, 15), (2 ** 31 + 5, 1023, 4), (64, 0, 9)]:
        start, dir = dt.irradiance_gather_ray(g, 3, pixel, sample, r, p, n)
        again = dt.irradiance_gather_ray(g, 3, pixel, sample, r, p, n)
        assert (start, dir) == again   # deterministic
        v, tries = ball(g.seed, 3, [pixel], [sample], P_GATHER, r)   # the counter: purpose 8, sub = r*16 + a
        assert tries[0] < DT_OCCL_TRIES and v[0].any()
        u = _normalized(v[0])
        want_dir = n + u
        want_start = p + 1e-3 * want_dir
        assert np.array(dir).tobytes() == want_dir.tobytes() and np.array(start).tobytes() == want_start.tobytes()
        # dir - n is the unit vector u up to the rounding of the sum and of normalized: a few ulp of 1
        back = np.array(dir) - n
        assert abs(math.sqrt(float(back @ back)) - 1.0) <= 8 * np.finfo(np.float64).eps
        seen += 1
    assert seen == 5
    # another frame, another seed: other draws
    a = dt.irradiance_gather_ray(g, 3, 7, 3, 1, p, n)
    assert dt.irradiance_gather_ray(g, 4, 7, 3, 1, p, n) != a
    g.seed = 12346
    assert dt.irradiance_gather_ray(g, 3, 7, 3, 1, p, n) != a


def test_gather_ray_void_probes_and_argument_errors():
    g = dt.globals_default()
    p = np.array([1.0, 2.0, 3.0])
    # n = -u: dir is the zero vector, a void probe (dir 0, start p)
    _, d = dt.irradiance_gather_ray(g, 0, 11, 2, 3, p, (0.0, 0.0, 0.0))
    start, dir = dt.irradiance_gather_ray(g, 0, 11, 2, 3, p, tuple(-v for v in d))
    assert dir == (0.0, 0.0, 0.0) and start == tuple(p)
    # a non-finite normal: a void dir
    start, dir = dt.irradiance_gather_ray(g, 0, 11, 2, 3, p, (float("nan"), 0.0, 1.0))
    assert dir == (0.0, 0.0, 0.0) and start == tuple(p)
    s, dd = D3(), D3()
    for r in (-1, DT_OCCL_MAX_AO_RAYS):
        assert dt.lib.dt_irradiance_gather_ray(1, 0, 0, 0, r, D3(*p), D3(0, 1, 0), s, dd) == INVALID
        assert dt.lib.dt_last_error().startswith(b"dt_irradiance_gather_ray: r ")
    assert dt.lib.dt_irradiance_gather_ray(1, 0, 0, 0, 0, None, D3(0, 1, 0), s, dd) == INVALID
    assert dt.lib.dt_last_error() == b"dt_irradiance_gather_ray: null argument"


def test_cosine_exact_cases_and_void_directions():
    n = (0.0, 1.0, 0.0)
    assert dt.irradiance_cosine(n, (0.0, 7.0, 0.0)) == 1.0          # parallel
    assert dt.irradiance_cosine(n, (0.0, -0.25, 0.0)) == 0.0        # opposite
    assert dt.irradiance_cosine(n, (3.0, 0.0, -4.0)) == 0.0         # perpendicular
    assert dt.irradiance_cosine((0.0, 0.0, 2.0), (0.0, 0.0, 1e-3)) == 2.0   # n as given: not normalised
    for void in [(0.0, 0.0, 0.0), (float("nan"), 1.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 1.0, -float("inf"))]:
        assert dt.irradiance_cosine(n, void) == 0.0
    # a general case: dmax(0, dot(n, normalized(dir))) in dt_math.h's order
    nn, d = np.array([0.36, 0.48, 0.8]), np.array([1.5, -0.25, 2.0])
    u = _normalized(d)
    assert dt.irradiance_cosine(nn, d) == max(0.0, (nn[0] * u[0] + nn[1] * u[1]) + nn[2] * u[2]) > 0
    c = ctypes.c_double(5.0)
    assert dt.lib.dt_irradiance_cosine(None, D3(0, 1, 0), ctypes.byref(c)) == INVALID and c.value == 5.0
    assert dt.lib.dt_last_error() == b"dt_irradiance_cosine: null argument"


# ---- the argument checks, before any device work --------------------------------------------------------------

_KEEP = []


def _arr(n, dtype=np.float64):
    a = np.zeros(n, dtype)
    _KEEP.append(a)
    return a


def _planes(*wanted):
    return Irradiance(*[_arr(8 * N).ctypes.data if w else None for w in wanted])


def _params(n_lights=1, gather_rays=2, light=()):
    p = IrradianceParams()
    p.n_lights, p.gather_rays = n_lights, gather_rays
    for j, l in enumerate(light):
        p.light[j] = l
    return p


POINT, NORMAL = _arr(3 * N), _arr(3 * N) + 1.0
_KEEP.append(NORMAL)
OKAY = dict(scene=STAND_IN, g=dt.globals_default(), n=N, point=POINT, normal=NORMAL, n_samples=4, p=_params(),
            out=_planes(1, 1, 1, 1))
W = "dt_points_irradiance: "
ROWS = [
    (dict(scene=None), W + "null scene"),
    (dict(g=None), W + "null globals"),
    (dict(point=None), W + "null point"),
    (dict(normal=None), W + "null normal"),
    (dict(p=None), W + "null params"),
    (dict(out=None), W + "null out"),
    (dict(n=-1), W + "n_points < 0"),
    (dict(n=2 ** 32), W + "n_points >= 2^32 (a point is the RNG counter's pixel)"),
    (dict(n_samples=0), W + "n_samples 0 outside 1..1024"),
    (dict(n_samples=1025), W + "n_samples 1025 outside 1..1024"),
    (dict(p=_params(n_lights=-1)), W + "n_lights -1 outside 0..8"),
    (dict(p=_params(n_lights=9)), W + "n_lights 9 outside 0..8"),
    (dict(p=_params(gather_rays=-1)), W + "gather_rays -1 outside 0..16"),
    (dict(p=_params(gather_rays=17)), W + "gather_rays 17 outside 0..16"),
    (dict(p=_params(n_lights=0), out=_planes(1, 0, 0, 1)), W + "out->direct given with n_lights == 0"),
    (dict(p=_params(n_lights=0), out=_planes(0, 1, 0, 1)), W + "out->direct_rgb given with n_lights == 0"),
    (dict(p=_params(gather_rays=0), out=_planes(1, 1, 1, 0)), W + "out->indirect_rgb given with gather_rays == 0"),
    (dict(p=_params(n_lights=0), out=_planes(0, 0, 1, 1)), W + "out->indirect_rgb given with n_lights == 0"),
    (dict(p=_params(gather_rays=0), out=_planes(1, 1, 0, 1)), W + "out->sky given with gather_rays == 0"),
    (dict(out=Irradiance()), W + "out wants no plane (every pointer is null)"),
    # two faults: the order of the checks
    (dict(scene=None, out=None), W + "null scene"),
    (dict(point=None, n=-1), W + "null point"),
    (dict(n=-1, n_samples=0), W + "n_points < 0"),
    (dict(n_samples=0, p=_params(gather_rays=17)), W + "n_samples 0 outside 1..1024"),
    (dict(p=_params(n_lights=9, gather_rays=17)), W + "n_lights 9 outside 0..8"),
    (dict(p=_params(n_lights=0, gather_rays=0), out=_planes(1, 0, 1, 1)), W + "out->direct given with n_lights == 0"),
    # ... and the errors come before the n_points == 0 shortcut
    (dict(n=0, n_samples=0), W + "n_samples 0 outside 1..1024"),
    (dict(n=0, out=Irradiance()), W + "out wants no plane (every pointer is null)"),
]


@pytest.mark.parametrize("i", range(len(ROWS)))
def test_rejected_before_any_device_work(i):
    change, text = ROWS[i]
    kw = dict(OKAY, **change)
    st = dt.Stats()
    ctypes.memset(ctypes.byref(st), 0x5A, ctypes.sizeof(st))
    ref = lambda x: None if x is None else ctypes.byref(x)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    rc = dt.lib.dt_points_irradiance(kw["scene"], ref(kw["g"]), 0, kw["n"], ptr(kw["point"]), ptr(kw["normal"]),
                                     kw["n_samples"], ref(kw["p"]), ref(kw["out"]), 0, None, ctypes.byref(st))
    assert rc == INVALID, (change, dt.lib.dt_last_error())
    assert dt.lib.dt_last_error() == text.encode(), change
    assert bytes(st) == b"\x5a" * ctypes.sizeof(st), change   # a rejected call leaves the caller's stats alone


def test_the_wrapper_rejects_an_unknown_plane_and_too_many_lights():
    pts = np.zeros((2, 3))
    with pytest.raises(dt.DTError, match="at most 8"):
        dt.points_irradiance(None, dt.globals_default(), pts, pts, lights=tuple(range(9)))
    with pytest.raises(dt.DTError, match="unknown plane 'ao'"):
        dt.points_irradiance(None, dt.globals_default(), pts, pts, lights=(0,), planes=("ao",))


# ---- the prediction on a scene with a closed-form answer -------------------------------------------------------

def test_ref_on_a_floor_under_a_point_light():
    """one rectangle, one point light straight above its centre: no occluder, every gather probe leaves the scene"""
    b = scene_gen._Builder(1.0, (0.0, 0.0, 0.0))
    scene_gen._rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.5, 0.5, 0.5), flags=0)
    b.light(scene_gen.POINT_LIGHT, center=(0, 2, 0), color=(0.5, 0.25, 1.0))
    g = b.globals((0.0, 2.0, 8.0), (0.0, 0.0, 0.0), 0.0, 6.0)
    desc, keep = b.desc()
    p = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, -1.5], [np.nan, 0.0, 0.0]])
    n = np.tile([0.0, 1.0, 0.0], (len(p), 1))
    ref = PointsIrradianceRef(desc, g, 5, p, n, 3, (0,), 2)
    want, counts = ref.planes()
    # the foot point: dir = (0, 2, 0), cosine exactly 1; elsewhere 2 / |(x, 2, z)| in dt_math.h's order
    assert want["direct"][0, 0] == 1.0 and list(want["direct_rgb"][0]) == [0.5, 0.25, 1.0]
    for i in (1, 2):
        d = np.array([0.0, 2.0, 0.0]) - p[i]
        c = (d / math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))[1]
        assert want["direct"][i, 0] == np.float32(((c + c) + c) / 3.0) and 0 < c < 1
    assert (want["sky"][:3] == 1.0).all() and (want["indirect_rgb"] == 0).all()
    # the void point: zeros, no probes
    assert want["direct"][3, 0] == 0 and want["sky"][3] == 0 and (want["direct_rgb"][3] == 0).all()
    assert counts == {"shadow_rays": 3 * 3, "rays": 3 * 3 * 2}
    # prefix cuts cost what they hold, and an unwanted plane costs nothing
    assert ref.planes(n_points=2, n_samples=1, gather_rays=1)[1] == {"shadow_rays": 2, "rays": 2}
    assert ref.planes(want=("sky",))[1] == {"shadow_rays": 0, "rays": 18}
    assert ref.planes(want=("direct",))[1] == {"shadow_rays": 9, "rays": 0}
