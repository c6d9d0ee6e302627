"""The argument checks of the auxiliary entry points (include/dt.h: the four ray queries, the two point-occlusion
calls, dt_render_occlusion, dt_render_features(_path), dt_render_mattes, dt_intersect_primary, dt_camera_rays),
as a table: for every rejecting branch the exact (code, dt_last_error text), and for every entry point inputs with
two faults at once, which pin the order of the checks. The table is the library's answers before the entry
points moved into a unit of their own and took one shared front; it holds unchanged after.

The first half needs no GPU: the scene is a stand-in address, as in tests/test_transmittance_host.py, and every
check in it returns before the scene is dereferenced. What a check reads from the scene (the
RectPrismWithCylinder rule, the light indices, the shape count) and the n == 0 shortcut behind those checks need
a scene, and a scene needs a device (dt_scene_prepare asks for the current one): the second half, marked gpu,
on the smallest builder scenes the GPU tests already use."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd import _lib

OK, INVALID, UNSUPPORTED = 0, -1, -4
N = 5
STAND_IN = ctypes.c_void_p(0x1000)   # a scene that is never dereferenced
_KEEP = []                           # arrays the structs below point into


def _arr(n, dtype=np.float64):
    a = np.zeros(n, dtype)
    _KEEP.append(a)
    return a


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _struct(cls, *wanted):
    """cls with a plane of 64 * N bytes behind every field whose flag is true"""
    return cls(*[_arr(8 * N).ctypes.data if w else None for w in wanted])


def G(**kw):
    g = dt.globals_default()
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def params(**kw):
    p = dt.occlusion_params_default()
    for k, v in kw.items():
        if k == "lights":
            for j, x in enumerate(v):
                p.lights[j] = x
        else:
            setattr(p, k, v)
    return p


def garbage_stats():
    st = dt.Stats()
    ctypes.memset(ctypes.byref(st), 0x5A, ctypes.sizeof(st))
    return st


def stats_zeroed(st):
    return bytes(st) == bytes(ctypes.sizeof(st))


START, DIR, SKIP = _arr(3 * N), _arr(3 * N) + 1.0, _arr(N, np.int32)
_KEEP.append(DIR)

# ---- the entry points: the arguments of a call every check accepts, and the call ----------------------------

RH, MH, RT = _lib.RayHits, _lib.RayMultiHits, _lib.RayTransmittance
Occ, Pan, Feat, Mat = _lib.Occlusion, _lib.OcclusionPanes, _lib.Features, _lib.Mattes


def trace_rays(scene, g, n, start, dir, out, stats=None):
    return dt.lib.dt_trace_rays(scene, _ref(g), n, _p(start), _p(dir), _ref(out), 0, None, _ref(stats))


def trace_rays_multi(scene, g, n, start, dir, k, out, stats=None):
    return dt.lib.dt_trace_rays_multi(scene, _ref(g), n, _p(start), _p(dir), k, _ref(out), 0, None, _ref(stats))


def rays_occluded(scene, g, n, start, dir, occluded, stats=None):
    return dt.lib.dt_rays_occluded(scene, _ref(g), n, _p(start), _p(dir), _p(SKIP), _p(occluded), 0, None, _ref(stats))


def rays_transmittance(scene, g, n, start, dir, k, out, stats=None):
    return dt.lib.dt_rays_transmittance(scene, _ref(g), n, _p(start), _p(dir), _p(SKIP), k, _ref(out), 0, None,
                                        _ref(stats))


def points_occlusion(scene, g, n, point, normal, n_samples, p, out, stats=None):
    return dt.lib.dt_points_occlusion(scene, _ref(g), 0, n, _p(point), _p(normal), n_samples, _ref(p), _ref(out), 0,
                                      None, _ref(stats))


def points_occlusion_glass(scene, g, n, point, normal, n_samples, p, max_panes, out, panes, stats=None):
    return dt.lib.dt_points_occlusion_glass(scene, _ref(g), 0, n, _p(point), _p(normal), n_samples, _ref(p), max_panes,
                                            _ref(out), _ref(panes), 0, None, _ref(stats))


def render_occlusion(scene, g, n_samples, p, out, stats=None):
    return dt.lib.dt_render_occlusion(scene, _ref(g), 0, None, n_samples, _ref(p), _ref(out), 0, None, _ref(stats))


def render_features(scene, g, n_samples, out, stats=None):
    return dt.lib.dt_render_features(scene, _ref(g), 0, None, n_samples, _ref(out), 0, None, _ref(stats))


def render_features_path(scene, g, n_samples, max_bounces, out, bounces, stats=None):
    return dt.lib.dt_render_features_path(scene, _ref(g), 0, None, n_samples, max_bounces, _ref(out), _p(bounces), 0, None,
                                          _ref(stats))


def render_mattes(scene, g, n_samples, gmap, n_shapes, layers, out, stats=None):
    return dt.lib.dt_render_mattes(scene, _ref(g), 0, None, n_samples, _p(gmap), n_shapes, layers, _ref(out), 0, None,
                                   _ref(stats), None)


def intersect_primary(scene, g, first, n, hit_shape, hit_t, ms=None):
    return dt.lib.dt_intersect_primary(scene, _ref(g), 0, first, n, _p(hit_shape), _p(hit_t), 0, None, _ref(ms))


def camera_rays(g, tiles, b, e, start, dir):
    return dt.lib.dt_camera_rays(_ref(g), 0, _ref(tiles), b, e, _p(start), _p(dir), 0, None, None)


def camera_rays_rows(g, tiles, b, e, start=None, dir=None):
    return dt.lib.dt_camera_rays_rows(_ref(g), _ref(tiles), b, e)


GMAP_BAD = _arr(4, np.int32)
GMAP_BAD[2] = -3
GMAP_BAD[3] = -1

ENTRY = {
    "dt_trace_rays": (trace_rays, dict(scene=STAND_IN, g=G(), n=N, start=START, dir=DIR, out=_struct(RH, 1, 1, 0, 0, 0))),
    "dt_trace_rays_multi": (trace_rays_multi, dict(scene=STAND_IN, g=G(), n=N, start=START, dir=DIR, k=2,
                                                   out=_struct(MH, 1, 1, 0, 0, 0, 0))),
    "dt_rays_occluded": (rays_occluded, dict(scene=STAND_IN, g=G(), n=N, start=START, dir=DIR, occluded=_arr(N, np.uint8))),
    "dt_rays_transmittance": (rays_transmittance, dict(scene=STAND_IN, g=G(), n=N, start=START, dir=DIR, k=2,
                                                       out=_struct(RT, 1, 1))),
    "dt_points_occlusion": (points_occlusion, dict(scene=STAND_IN, g=G(), n=N, point=START, normal=DIR, n_samples=4,
                                                   p=params(), out=_struct(Occ, 1, 0))),
    "dt_points_occlusion_glass": (points_occlusion_glass,
                                  dict(scene=STAND_IN, g=G(), n=N, point=START, normal=DIR, n_samples=4, p=params(),
                                       max_panes=1, out=_struct(Occ, 1, 0), panes=None)),
    "dt_render_occlusion": (render_occlusion, dict(scene=STAND_IN, g=G(), n_samples=9, p=params(), out=_struct(Occ, 1, 0))),
    "dt_render_features": (render_features, dict(scene=STAND_IN, g=G(), n_samples=9, out=_struct(Feat, 1, 0, 1, 0, 0))),
    "dt_render_features_path": (render_features_path, dict(scene=STAND_IN, g=G(), n_samples=9, max_bounces=2,
                                                           out=_struct(Feat, 1, 0, 1, 0, 0), bounces=None)),
    "dt_render_mattes": (render_mattes, dict(scene=STAND_IN, g=G(), n_samples=9, gmap=None, n_shapes=4, layers=2,
                                             out=_struct(Mat, 1, 1, 0))),
    "dt_intersect_primary": (intersect_primary, dict(scene=STAND_IN, g=G(), first=0, n=N, hit_shape=_arr(N, np.int32),
                                                     hit_t=_arr(N, np.float32))),
    "dt_camera_rays": (camera_rays, dict(g=G(xRes=4, yRes=2), tiles=None, b=0, e=2, start=_arr(48), dir=_arr(48))),
    "dt_camera_rays_rows": (camera_rays_rows, dict(g=G(xRes=4, yRes=2), tiles=None, b=0, e=2)),
}

NO_PLANE = "out wants no plane (every pointer is null)"
W00 = "window [0,0): need 0 <= begin < end <= spp (9)"
W04 = "window [0,4): with spp < 64 the only window is [0,9)"
BOTH = _struct(Occ, 1, 1)
ONLY_LIGHT = _struct(Occ, 0, 1)


def _ray_front(who, out_name="out", with_planes=True):
    """the rows the four ray queries share: (changes, code, text); the last four hold two faults each"""
    rows = [
        (dict(scene=None), INVALID, who + ": null scene"),
        (dict(g=None), INVALID, who + ": null globals"),
        (dict(start=None), INVALID, who + ": null start"),
        (dict(dir=None), INVALID, who + ": null dir"),
        (dict(**{out_name: None}), INVALID, who + ": null " + out_name),
        (dict(n=-1), INVALID, who + ": n_rays < 0"),
        (dict(scene=None, g=None), INVALID, who + ": null scene"),
        (dict(g=None, n=-1), INVALID, who + ": null globals"),
        (dict(start=None, dir=None), INVALID, who + ": null start"),
        (dict(**{out_name: None, "n": -1}), INVALID, who + ": null " + out_name),
    ]
    if with_planes:
        cls = type(ENTRY[who][1]["out"])
        none = cls()
        rows += [(dict(out=none), INVALID, who + ": " + NO_PLANE),
                 (dict(out=none, n=-1), INVALID, who + ": " + NO_PLANE),
                 (dict(out=none, dir=None), INVALID, who + ": null dir")]
    return rows


def _occl_rows(who):
    """check_occlusion's rows before it looks at the scene, shared by the three occlusion calls"""
    return [
        (dict(p=params(ao_rays=-1)), INVALID, who + ": ao_rays -1 outside 0..16"),
        (dict(p=params(ao_rays=17)), INVALID, who + ": ao_rays 17 outside 0..16"),
        (dict(p=params(n_lights=-1)), INVALID, who + ": n_lights -1 outside 0..8"),
        (dict(p=params(n_lights=9)), INVALID, who + ": n_lights 9 outside 0..8"),
        (dict(p=params(ao_radius=0.0)), INVALID, who + ": ao_radius must be finite and > 0"),
        (dict(p=params(ao_radius=float("nan"))), INVALID, who + ": ao_radius must be finite and > 0"),
        (dict(p=params(ao_radius=float("inf"))), INVALID, who + ": ao_radius must be finite and > 0"),
        (dict(p=params(ao_rays=0, n_lights=1), out=BOTH), INVALID, who + ": out->ao given with ao_rays == 0"),
        (dict(out=BOTH), INVALID, who + ": out->light given with n_lights == 0"),
        (dict(out=Occ()), INVALID, who + ": " + NO_PLANE),
        # two faults
        (dict(p=params(ao_rays=17, n_lights=9)), INVALID, who + ": ao_rays 17 outside 0..16"),
        (dict(p=params(n_lights=9, ao_radius=0.0)), INVALID, who + ": n_lights 9 outside 0..8"),
        (dict(p=params(ao_rays=0), out=BOTH), INVALID, who + ": out->ao given with ao_rays == 0"),
        (dict(p=params(ao_radius=-1.0), out=Occ()), INVALID, who + ": ao_radius must be finite and > 0"),
    ]


def _points_rows(who):
    return [
        (dict(scene=None), INVALID, who + ": null scene"),
        (dict(g=None), INVALID, who + ": null globals"),
        (dict(point=None), INVALID, who + ": null point"),
        (dict(normal=None), INVALID, who + ": null normal"),
        (dict(p=None), INVALID, who + ": null params"),
        (dict(out=None), INVALID, who + ": null out"),
        (dict(n=-1), INVALID, who + ": n_points < 0"),
        (dict(n=2 ** 32), INVALID, who + ": n_points >= 2^32 (a point is the RNG counter's pixel)"),
        (dict(n_samples=0), INVALID, who + ": n_samples 0 outside 1..1024"),
        (dict(n_samples=1025), INVALID, who + ": n_samples 1025 outside 1..1024"),
        # two faults
        (dict(scene=None, out=None), INVALID, who + ": null scene"),
        (dict(point=None, n=-1), INVALID, who + ": null point"),
        (dict(p=None, out=None), INVALID, who + ": null params"),
        (dict(n=-1, n_samples=0), INVALID, who + ": n_points < 0"),
        (dict(n_samples=0, p=params(ao_rays=17)), INVALID, who + ": n_samples 0 outside 1..1024"),
        # ... and the errors come before the n_points == 0 shortcut
        (dict(n=0, n_samples=0), INVALID, who + ": n_samples 0 outside 1..1024"),
        (dict(n=0, out=Occ()), INVALID, who + ": " + NO_PLANE),
    ] + _occl_rows(who)


def _window_rows(who, prefix):
    """dt_window_check's answers for samples [0, n_samples) under the caller's prefix"""
    return [
        (dict(n_samples=0), INVALID, prefix + W00),
        (dict(n_samples=4), INVALID, prefix + W04),
        (dict(n_samples=10), INVALID, prefix + "window [0,10): need 0 <= begin < end <= spp (9)"),
        (dict(g=G(antialias_samples=0)), INVALID, prefix + "invalid globals"),
        (dict(g=G(antialias_samples=4096), n_samples=100), INVALID,
         prefix + "window [0,100): end must be a multiple of 64 or spp (4096)"),
    ]


FP, MT, RO = "dt_render_features_path", "dt_render_mattes", "dt_render_occlusion"
TABLE = {
    "dt_trace_rays": _ray_front("dt_trace_rays"),
    "dt_trace_rays_multi": _ray_front("dt_trace_rays_multi") + [
        (dict(k=0), INVALID, "dt_trace_rays_multi: k = 0 outside 1..8"),
        (dict(k=9), INVALID, "dt_trace_rays_multi: k = 9 outside 1..8"),
        (dict(k=-2), INVALID, "dt_trace_rays_multi: k = -2 outside 1..8"),
        (dict(n=-1, k=0), INVALID, "dt_trace_rays_multi: n_rays < 0"),
        (dict(out=MH(), k=9), INVALID, "dt_trace_rays_multi: " + NO_PLANE),
        (dict(n=0, k=9), INVALID, "dt_trace_rays_multi: k = 9 outside 1..8"),
    ],
    "dt_rays_occluded": _ray_front("dt_rays_occluded", "occluded", with_planes=False),
    "dt_rays_transmittance": _ray_front("dt_rays_transmittance") + [
        (dict(k=-1), INVALID, "dt_rays_transmittance: k = -1 outside 0..8"),
        (dict(k=9), INVALID, "dt_rays_transmittance: k = 9 outside 0..8"),
        (dict(k=0), INVALID, "dt_rays_transmittance: out->pane_shape given with k == 0"),
        (dict(n=-1, k=9), INVALID, "dt_rays_transmittance: n_rays < 0"),
        (dict(out=RT(), k=9), INVALID, "dt_rays_transmittance: " + NO_PLANE),
        (dict(n=0, k=9), INVALID, "dt_rays_transmittance: k = 9 outside 0..8"),
        (dict(n=0, k=0), INVALID, "dt_rays_transmittance: out->pane_shape given with k == 0"),
    ],
    "dt_points_occlusion": _points_rows("dt_points_occlusion"),
    "dt_points_occlusion_glass": _points_rows("dt_points_occlusion_glass") + [
        (dict(max_panes=-1), INVALID, "dt_points_occlusion_glass: max_panes -1 outside 0..8"),
        (dict(max_panes=9), INVALID, "dt_points_occlusion_glass: max_panes 9 outside 0..8"),
        (dict(p=params(ao_rays=0, n_lights=1), out=ONLY_LIGHT, panes=_struct(Pan, 1, 0)), INVALID,
         "dt_points_occlusion_glass: panes->ao_panes given with ao_rays == 0"),
        (dict(panes=_struct(Pan, 0, 1)), INVALID, "dt_points_occlusion_glass: panes->light_panes given with n_lights == 0"),
        (dict(out=Occ(), panes=_struct(Pan, 1, 0)), INVALID, "dt_points_occlusion_glass: " + NO_PLANE),
        # two faults
        (dict(n_samples=0, max_panes=9), INVALID, "dt_points_occlusion_glass: n_samples 0 outside 1..1024"),
        (dict(max_panes=9, p=params(ao_rays=17)), INVALID, "dt_points_occlusion_glass: max_panes 9 outside 0..8"),
        (dict(panes=_struct(Pan, 0, 1), p=params(ao_rays=17)), INVALID,
         "dt_points_occlusion_glass: panes->light_panes given with n_lights == 0"),
        (dict(n=0, max_panes=9), INVALID, "dt_points_occlusion_glass: max_panes 9 outside 0..8"),
    ],
    RO: [
        (dict(scene=None), INVALID, RO + ": null scene"),
        (dict(g=None), INVALID, RO + ": null globals"),
        (dict(p=None), INVALID, RO + ": null params"),
        (dict(out=None), INVALID, RO + ": null out"),
        # two faults
        (dict(scene=None, p=None), INVALID, RO + ": null scene"),
        (dict(p=None, out=None), INVALID, RO + ": null params"),
        (dict(out=None, n_samples=0), INVALID, RO + ": null out"),
        (dict(n_samples=0, p=params(ao_rays=17)), INVALID, RO + ": n_samples: " + W00),
    ] + _window_rows(RO, RO + ": n_samples: ") + _occl_rows(RO),
    "dt_render_features": [
        (dict(scene=None), INVALID, "dt_render_features: null scene"),
        (dict(g=None), INVALID, "dt_render_features: null globals"),
        (dict(out=None), INVALID, "dt_render_features: null planes"),
        (dict(out=Feat()), INVALID, "dt_render_features: no plane wanted (every pointer is null)"),
        # two faults
        (dict(scene=None, g=None), INVALID, "dt_render_features: null scene"),
        (dict(g=None, out=None), INVALID, "dt_render_features: null globals"),
        (dict(out=Feat(), n_samples=0), INVALID, "dt_render_features: no plane wanted (every pointer is null)"),
    ] + _window_rows("dt_render_features", ""),   # (dt_window_check's text as it is)
    FP: [
        (dict(scene=None), INVALID, FP + ": null scene"),
        (dict(g=None), INVALID, FP + ": null globals"),
        (dict(out=None), INVALID, FP + ": null planes"),
        (dict(out=Feat()), INVALID, FP + ": no plane wanted (every pointer is null)"),
        (dict(max_bounces=-1), INVALID, FP + ": max_bounces must be in 0..8, got -1"),
        (dict(max_bounces=9), INVALID, FP + ": max_bounces must be in 0..8, got 9"),
        # two faults
        (dict(scene=None, out=None), INVALID, FP + ": null scene"),
        (dict(out=None, max_bounces=9), INVALID, FP + ": null planes"),
        (dict(n_samples=0, max_bounces=9), INVALID, FP + ": n_samples: " + W00),
    ] + _window_rows(FP, FP + ": n_samples: "),
    MT: [
        (dict(scene=None), INVALID, MT + ": null scene"),
        (dict(g=None), INVALID, MT + ": null globals"),
        (dict(out=None), INVALID, MT + ": null out"),
        (dict(out=Mat()), INVALID, MT + ": " + NO_PLANE),
        (dict(layers=0), INVALID, MT + ": layers 0 outside 1..8"),
        (dict(layers=9), INVALID, MT + ": layers 9 outside 1..8"),
        (dict(n_shapes=-1), INVALID, MT + ": n_shapes -1 is negative"),
        (dict(gmap=GMAP_BAD), INVALID, MT + ": group_of_shape[2] is negative"),
        # two faults
        (dict(scene=None, layers=0), INVALID, MT + ": null scene"),
        (dict(out=Mat(), n_samples=0), INVALID, MT + ": " + NO_PLANE),
        (dict(n_samples=0, layers=0), INVALID, MT + ": n_samples: " + W00),
        (dict(layers=9, n_shapes=-1), INVALID, MT + ": layers 9 outside 1..8"),
        (dict(n_shapes=-1, gmap=GMAP_BAD), INVALID, MT + ": n_shapes -1 is negative"),
    ] + _window_rows(MT, MT + ": n_samples: "),
    "dt_intersect_primary": [
        (dict(scene=None), INVALID, "null argument"),
        (dict(g=None), INVALID, "null argument"),
        (dict(hit_shape=None), INVALID, "null argument"),
        (dict(hit_t=None), INVALID, "null argument"),
        (dict(first=-1), INVALID, "negative ray range"),
        (dict(n=-1), INVALID, "negative ray range"),
        # two faults
        (dict(hit_t=None, n=-1), INVALID, "null argument"),
        (dict(scene=None, first=-1), INVALID, "null argument"),
    ],
    "dt_camera_rays": [
        (dict(start=None), INVALID, "dt_camera_rays: null start"),
        (dict(dir=None), INVALID, "dt_camera_rays: null dir"),
        (dict(g=None), INVALID, "dt_camera_rays: null globals"),
        (dict(b=-1), INVALID, "dt_camera_rays: samples [-1,2): need 0 <= sample_begin < sample_end, at most 1024 samples"),
        (dict(b=2), INVALID, "dt_camera_rays: samples [2,2): need 0 <= sample_begin < sample_end, at most 1024 samples"),
        (dict(e=1025), INVALID, "dt_camera_rays: samples [0,1025): need 0 <= sample_begin < sample_end, at most 1024 samples"),
        (dict(g=G(xRes=0)), INVALID, "dt_camera_rays: globals or tiles: invalid globals"),
        (dict(tiles=_lib.Tiles(x0=3, x1=2, world=1)), INVALID, "dt_camera_rays: globals or tiles: empty pixel window"),
        (dict(tiles=_lib.Tiles(rank=2, world=2)), INVALID, "dt_camera_rays: globals or tiles: rank out of range"),
        # two faults
        (dict(start=None, dir=None), INVALID, "dt_camera_rays: null start"),
        (dict(dir=None, b=2), INVALID, "dt_camera_rays: null dir"),
        (dict(g=None, start=None), INVALID, "dt_camera_rays: null globals"),
        (dict(b=2, g=G(xRes=0)), INVALID,
         "dt_camera_rays: samples [2,2): need 0 <= sample_begin < sample_end, at most 1024 samples"),
    ],
    "dt_camera_rays_rows": [   # the same check under its own name; the answer is -1
        (dict(g=None), -1, "dt_camera_rays_rows: null globals"),
        (dict(e=0), -1, "dt_camera_rays_rows: samples [0,0): need 0 <= sample_begin < sample_end, at most 1024 samples"),
        (dict(g=G(yRes=-1)), -1, "dt_camera_rays_rows: globals or tiles: invalid globals"),
        (dict(e=0, g=G(yRes=-1)), -1,
         "dt_camera_rays_rows: samples [0,0): need 0 <= sample_begin < sample_end, at most 1024 samples"),
        (dict(g=None, e=0), -1, "dt_camera_rays_rows: null globals"),
    ],
}

ROWS = [(name, i) for name in TABLE for i in range(len(TABLE[name]))]


def test_every_entry_point_is_in_the_table_with_two_fault_rows():
    assert set(TABLE) == set(ENTRY)
    for name, rows in TABLE.items():
        assert sum(len(change) >= 2 for change, _, _ in rows) >= 2, name


def test_camera_rays_rows_of_the_accepted_call():
    fn, ok = ENTRY["dt_camera_rays_rows"]
    assert fn(**ok) == 4 * 2 * 2


@pytest.mark.parametrize("name,i", ROWS, ids=["%s-%d" % r for r in ROWS])
def test_rejected_with_the_exact_code_and_text(name, i):
    fn, ok = ENTRY[name]
    change, code, text = TABLE[name][i]
    st = garbage_stats() if "stats" in fn.__code__.co_varnames else None
    kw = dict(ok, **change)
    if st is not None:
        kw["stats"] = st
    assert fn(**kw) == code, (change, dt.lib.dt_last_error())
    assert dt.lib.dt_last_error() == text.encode(), change
    if st is not None:   # a rejected call leaves the caller's stats alone
        assert bytes(st) == b"\x5a" * ctypes.sizeof(st), change


# ---- what needs a scene (and so a device) --------------------------------------------------------------------

@pytest.fixture(scope="module")
def scenes(cuda):
    g = dt.globals_default()
    g.use_model = 0
    g.xRes, g.yRes = 16, 8
    room = dt.Scene(dt.build_scene("final", 240, g), g)
    prism = dt.Scene(dt.build_scene("prismcyl", 30, g), g)
    yield g, room, prism
    room.close()
    prism.close()


def _with_scene(name, scene, g, **change):
    fn, ok = ENTRY[name]
    kw = dict(ok, scene=scene._h, g=g, **change)
    st = None
    if "stats" in fn.__code__.co_varnames:
        st = kw["stats"] = garbage_stats()
    rc = fn(**kw)
    return rc, dt.lib.dt_last_error().decode(), st


QUERIES = ["dt_trace_rays", "dt_trace_rays_multi", "dt_rays_occluded", "dt_rays_transmittance", "dt_points_occlusion",
           "dt_points_occlusion_glass"]
RPC = "scenes with a RectPrismWithCylinder"


@pytest.mark.gpu
@pytest.mark.parametrize("name", QUERIES)
def test_no_rays_is_ok_with_zeroed_stats(scenes, name):
    g, room, prism = scenes
    rc, err, st = _with_scene(name, room, g, n=0)
    assert rc == OK and stats_zeroed(st)
    # ... but the RectPrismWithCylinder rule comes first
    rc, err, st = _with_scene(name, prism, g, n=0)
    assert (rc, err) == (UNSUPPORTED, name + ": " + RPC) and not stats_zeroed(st)


@pytest.mark.gpu
def test_no_rays_of_intersect_primary(scenes):
    g, room, prism = scenes
    ms = ctypes.c_float(7.0)
    fn, ok = ENTRY["dt_intersect_primary"]
    assert fn(**dict(ok, scene=room._h, g=g, n=0, ms=ms)) == OK and ms.value == 0.0
    assert fn(**dict(ok, scene=prism._h, g=g, n=0, ms=ms)) == UNSUPPORTED
    assert dt.lib.dt_last_error() == b"dt_intersect_primary: " + RPC.encode()


@pytest.mark.gpu
def test_the_checks_that_read_the_scene(scenes):
    g, room, prism = scenes
    for name in QUERIES + ["dt_render_occlusion", "dt_render_features", "dt_render_features_path", "dt_render_mattes"]:
        extra = dict(n_shapes=0) if name == "dt_render_mattes" else {}
        rc, err, _ = _with_scene(name, prism, g, **extra)
        if name == "dt_render_mattes":   # the shape count comes before the rule
            assert rc == INVALID and err.startswith(MT + ": n_shapes 0, the scene has "), err
            continue
        assert (rc, err) == (UNSUPPORTED, name + ": " + RPC), name
    # the argument checks come before the rule
    for name, change, text in [("dt_trace_rays_multi", dict(k=9), "dt_trace_rays_multi: k = 9 outside 1..8"),
                               ("dt_rays_transmittance", dict(k=0), "dt_rays_transmittance: out->pane_shape given with k == 0"),
                               ("dt_render_features_path", dict(max_bounces=9), FP + ": max_bounces must be in 0..8, got 9"),
                               ("dt_trace_rays", dict(n=-1), "dt_trace_rays: n_rays < 0")]:
        rc, err, _ = _with_scene(name, prism, g, **change)
        assert (rc, err) == (INVALID, text), name
    # the light indices: after the planes' rules, before the RectPrismWithCylinder rule
    for name in ("dt_points_occlusion", "dt_points_occlusion_glass", "dt_render_occlusion"):
        for scene in (room, prism):
            rc, err, _ = _with_scene(name, scene, g, p=params(n_lights=2, lights=[0, 99]), out=BOTH)
            assert rc == INVALID and err.startswith(name + ": lights[1] = 99, the scene has ") and err.endswith(" lights"), err
            rc, err, _ = _with_scene(name, scene, g, p=params(n_lights=1, lights=[-1]), out=Occ())
            assert (rc, err) == (INVALID, name + ": " + NO_PLANE)
