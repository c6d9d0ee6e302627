"""Transmittance queries, the host half (include/dt.h dt_rays_transmittance, dt_points_occlusion_glass): the
exports, every DT_E_INVALID check (all before any device work; the scene is a stand-in address that is never
dereferenced, as in tests/test_points_occlusion_host.py), the restatement of tests/transmittance_ref.py against
cases worked by hand, and the conditions under which tests/test_gpu_transmittance.py means something: on every
ray set used there the restatement's (panes != 0) is RayQueryRef.occluded, and every class of ray is present at
least 16 times, so that a kernel which never sees a pane cannot pass. No GPU.

DT_E_UNSUPPORTED, the light indices and n == 0 need a scene, and a scene needs a device: the GPU file."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
import transmittance_ref as T
from distraytracer_amd import _lib

INVALID = -1
FLOOR = 16   # rays per class and ray set, at the least


def test_the_exports_exist():
    for name in ("dt_rays_transmittance", "dt_points_occlusion_glass"):
        assert name in _lib.EXPORTS and hasattr(dt.lib, name), name
    assert dt.lib.dt_abi_version() == 8 and _lib.DT_TRANSMIT_MAX_PANES == 8 == T.MAX_PANES
    assert "rays_transmittance" in dt.__all__ and callable(dt.rays_transmittance)


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def test_rays_transmittance_argument_errors_come_before_any_device_work():
    g = dt.globals_default()
    N = 5
    start, dir = np.zeros((N, 3)), np.ones((N, 3))
    panes, shape = np.zeros(N, np.int32), np.zeros(N * 8, np.int32)
    scene = ctypes.c_void_p(0x1000)
    RT = _lib.RayTransmittance
    ok = dict(scene=scene, g=g, n=N, start=start, dir=dir, k=2, out=RT(panes.ctypes.data, shape.ctypes.data))

    def call(scene, g, n, start, dir, k, out):
        st = dt.Stats()
        return dt.lib.dt_rays_transmittance(scene, ctypes.byref(g) if g is not None else None, n, _ptr(start), _ptr(dir),
                                            None, k, ctypes.byref(out) if out is not None else None, 0, None,
                                            ctypes.byref(st))

    cases = [
        (dict(scene=None), b"null scene"),
        (dict(g=None), b"null globals"),
        (dict(start=None), b"null start"),
        (dict(dir=None), b"null dir"),
        (dict(out=None), b"null out"),
        (dict(out=RT(None, None)), b"every pointer is null"),
        (dict(n=-1), b"n_rays < 0"),
        (dict(k=-1), b"k = -1 outside 0..8"),
        (dict(k=9), b"k = 9 outside 0..8"),
        (dict(k=0), b"out->pane_shape given with k == 0"),
        # the errors also come before the n_rays == 0 shortcut
        (dict(n=0, k=9), b"k = 9"),
    ]
    for change, msg in cases:
        assert call(**dict(ok, **change)) == INVALID, msg
        err = dt.lib.dt_last_error()
        assert err.startswith(b"dt_rays_transmittance: ") and msg in err, (msg, err)


def test_points_occlusion_glass_argument_errors_come_before_any_device_work():
    g = dt.globals_default()
    N = 5
    pt, nm = np.zeros((N, 3)), np.tile([0.0, 1.0, 0.0], (N, 1))
    ao, light = np.zeros(N, np.float32), np.zeros(N * 8, np.float32)
    aop, lp = np.zeros(N, np.float32), np.zeros(N * 8, np.float32)
    scene = ctypes.c_void_p(0x1000)
    Occ, Pan = _lib.Occlusion, _lib.OcclusionPanes

    def params(**kw):
        p = dt.occlusion_params_default()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(scene, g, n_points, point, normal, n_samples, p, max_panes, o, pn):
        st = dt.Stats()
        return dt.lib.dt_points_occlusion_glass(scene, ctypes.byref(g) if g is not None else None, 0, n_points,
                                                _ptr(point), _ptr(normal), n_samples,
                                                ctypes.byref(p) if p is not None else None, max_panes,
                                                ctypes.byref(o) if o is not None else None,
                                                ctypes.byref(pn) if pn is not None else None, 0, None, ctypes.byref(st))

    both = Occ(ao.ctypes.data, light.ctypes.data)
    only_ao = Occ(ao.ctypes.data, None)
    ok = dict(scene=scene, g=g, n_points=N, point=pt, normal=nm, n_samples=4, p=params(), max_panes=1, o=only_ao,
              pn=None)
    cases = [
        (dict(scene=None), b"null scene"),
        (dict(g=None), b"null globals"),
        (dict(point=None), b"null point"),
        (dict(normal=None), b"null normal"),
        (dict(p=None), b"null params"),
        (dict(o=None), b"null out"),
        (dict(n_points=-1), b"n_points < 0"),
        (dict(n_points=2 ** 32), b"n_points >= 2^32"),
        (dict(n_samples=0), b"n_samples 0 outside 1..1024"),
        (dict(n_samples=1025), b"n_samples 1025 outside 1..1024"),
        (dict(max_panes=-1), b"max_panes -1 outside 0..8"),
        (dict(max_panes=9), b"max_panes 9 outside 0..8"),
        (dict(p=params(ao_rays=0, n_lights=1), o=Occ(None, light.ctypes.data), pn=Pan(aop.ctypes.data, None)),
         b"panes->ao_panes given with ao_rays == 0"),
        (dict(pn=Pan(None, lp.ctypes.data)), b"panes->light_panes given with n_lights == 0"),
        (dict(p=params(ao_rays=-1)), b"ao_rays"),
        (dict(p=params(ao_rays=17)), b"ao_rays"),
        (dict(p=params(n_lights=-1)), b"n_lights"),
        (dict(p=params(n_lights=9)), b"n_lights"),
        (dict(p=params(ao_radius=0.0)), b"ao_radius"),
        (dict(p=params(ao_radius=float("nan"))), b"ao_radius"),
        (dict(p=params(ao_rays=0, n_lights=1), o=both), b"out->ao given with ao_rays == 0"),
        (dict(o=both), b"out->light given with n_lights == 0"),
        (dict(o=Occ(None, None)), b"every pointer is null"),
        (dict(o=Occ(None, None), pn=Pan(aop.ctypes.data, None)), b"every pointer is null"),
        (dict(n_points=0, max_panes=9), b"max_panes"),
    ]
    for change, msg in cases:
        assert call(**dict(ok, **change)) == INVALID, msg
        err = dt.lib.dt_last_error()
        assert err.startswith(b"dt_points_occlusion_glass: ") and msg in err, (msg, err)


def test_python_wrapper_checks():
    s, d = np.zeros((2, 3)), np.ones((2, 3))
    for k in (-1, 9, 1.0, True):
        with pytest.raises(dt.DTError, match="rays_transmittance: k must be an integer in 0..8"):
            dt.rays_transmittance(None, dt.globals_default(), s, d, k=k)
    with pytest.raises(dt.DTError, match="unknown plane"):
        dt.rays_transmittance(None, dt.globals_default(), s, d, planes=("t",))


def test_three_panes_and_a_wall_by_hand():
    """pane_stack(3): glass rectangles at z = 1, 2, 3 (shapes 0, 1, 2) over x in [-2, 2], y in [0, 4], the wall
    (shape 3) at z = 4 over y in [0, 2], the glass sphere (shape 4) at (4, 2, 3), r = 0.75"""
    desc, g, keep = T.pane_stack(3)
    tr = T.TransmitRef(desc, g)
    assert list(tr.glass) == [True, True, True, False, True]
    nan = float("nan")
    rays = [   # start, dir, skip, panes, pane_shape at k = 2
        ((0, 1, 0), (0, 0, 0.5), -1, 0, (-1, -1)),        # ends before the first pane
        ((0, 1, 0), (0, 0, 1.5), -1, 1, (0, -1)),
        ((0, 1, 0), (0, 0, 2.5), -1, 2, (0, 1)),
        ((0, 1, 0), (0, 0, 3.5), -1, 3, (0, 1)),          # the list holds the two smallest of three
        ((0, 1, 0), (0, 0, 3.5), 0, 2, (1, 2)),           # the first pane skipped
        ((0, 1, 0), (0, 0, 3.5), 3, 3, (0, 1)),           # the wall skipped: it is beyond t_max anyway
        ((0, 1, 0), (0, 0, 5.0), -1, -1, (-1, -1)),       # the wall: blocked, nothing listed
        ((0, 1, 0), (0, 0, 5.0), 3, 3, (0, 1)),           # the wall skipped
        ((0, 3, 0), (0, 0, 5.0), -1, 3, (0, 1)),          # over the wall
        ((0, 1, 5), (0, 0, -5.0), -1, -1, (-1, -1)),      # from behind: the wall first, all the same
        ((0, 1, 3.5), (0, 0, -3.0), -1, 3, (0, 1)),       # from between wall and panes, backwards
        ((4, 2, 0), (0, 0, 3.0), -1, 1, (4, -1)),         # ends at the centre of the glass sphere
        ((4, 2, 0), (0, 0, 6.0), -1, 1, (4, -1)),         # through it: a shape counts once
        ((4, 2, 0), (0, 0, 6.0), 4, 0, (-1, -1)),
        ((4, 2, 0), (0, 0, 2.0), -1, 0, (-1, -1)),        # ends before it
        ((3, 1, 0), (0, 0, 6.0), -1, 0, (-1, -1)),        # beside everything
        ((0, 1, 0), (0, 0, 0), -1, 0, (-1, -1)),          # void: a zero dir
        ((0, nan, 0), (0, 0, 5.0), -1, 0, (-1, -1)),      # void: a NaN
        ((0.1, 1, 0), (0.3, 0.2, 3.5), -1, 3, (0, 1)),    # tilted
    ]
    start = np.array([r[0] for r in rays], np.float64)
    dir = np.array([r[1] for r in rays], np.float64)
    skip = np.array([r[2] for r in rays], np.int32)
    got = tr.transmittance(start, dir, skip, k=2)
    assert got["panes"].tolist() == [r[3] for r in rays]
    assert got["pane_shape"].tolist() == [list(r[4]) for r in rays]
    assert np.array_equal(tr.rq.occluded(start, dir, skip) != 0, got["panes"] != 0)
    # k = 0: no list; k = 8: everything, -1 beyond
    assert tr.transmittance(start, dir, skip, k=0)["pane_shape"].shape == (len(rays), 0)
    assert tr.transmittance(start[3:4], dir[3:4], skip[3:4], k=8)["pane_shape"].tolist() == [[0, 1, 2] + [-1] * 5]


def _gpu_ray_sets():
    """every ray set of tests/test_gpu_transmittance.py on the two synthetic scenes: (scene, what, start, dir, skip)"""
    out = []
    for name in ("stack", "glass"):
        s, d, k = T.ray_set(name)
        out.append((name, "main", s, d, k))
    for n_clear in (0, 1):
        out.append(("stack", "blocked wave, %d clear" % n_clear) + T.blocked_wave_rays(n_clear))
    return out


def test_panes_nonzero_is_occluded_on_every_gpu_ray_set():
    for name, what, s, d, k in _gpu_ray_sets():
        tr = T.scene(name)[3]
        got = tr.transmittance(s, d, k)["panes"]
        assert np.array_equal(got != 0, tr.rq.occluded(s, d, k) != 0), (name, what)


@pytest.mark.parametrize("name", ["stack", "glass"])
def test_every_class_of_ray_is_in_the_main_ray_sets(name):
    tr = T.scene(name)[3]
    s, d, k = T.ray_set(name)
    assert len(s) == 64 * 3 + 7
    cl = T.classes(tr, s, d, k, T.K_CLASS[name])
    counts = {c: int(v.sum()) for c, v in cl.items()}
    print(name, counts)
    assert len(counts) == 9
    for c, v in counts.items():
        assert v >= FLOOR, (name, c, v)
    # and within every full wave: four distinct skip shapes beside -1, an axis-parallel ray beside finite ones
    for w in range(3):
        sk, dd = k[64 * w:64 * w + 64], d[64 * w:64 * w + 64]
        assert len(set(sk.tolist()) - {-1}) >= 4 and (sk == -1).any()
        par = (dd == 0).any(axis=1)
        assert par.any() and not par.all()
    # up to five panes crossed on the stack
    if name == "stack":
        assert T.prediction(name, 8)["panes"].max() == 5


def test_the_blocked_waves():
    tr = T.scene("stack")[3]
    a = tr.transmittance(*T.blocked_wave_rays(0))["panes"]
    b = tr.transmittance(*T.blocked_wave_rays(1))["panes"]
    assert (a == -1).all()
    assert (b == -1).sum() == 63 and b[37] == 5


def test_points_behind_the_pane_light_up_through_it():
    """the floor of shade_glass behind its pane: dark at max_panes = 0, lit at 1, by the restatement"""
    ref, p, n = T.points_case()
    p0, probes0 = ref.planes(0)
    p1, probes1 = ref.planes(1)
    assert probes0 == probes1 > 0
    assert ((p0["light"] == 0) & (p1["light"] > 0)).any()
    assert (p0["ao_panes"] == 0).all() and (p0["light_panes"] == 0).all()
    assert (p1["light_panes"] > 0).any() and (p1["ao_panes"] > 0).any()
    assert ((p1["ao"] > 0) & (p1["ao"] < 1)).any()
    # the void point writes zeros
    for pl in (p0, p1):
        assert pl["ao"][100] == 0 and (pl["light"][100] == 0).all() and (pl["light_panes"][100] == 0).all()
    # with max_panes = 0 the restatement is PointsOcclusionRef's planes
    from points_occlusion_ref import PointsOcclusionRef
    P = T.POINTS
    desc, g, keep, tr = T.scene("glass")
    old = PointsOcclusionRef(desc, g, P["frame"], p[:70], n[:70], 2, P["ao_rays"], P["ao_radius"], P["lights"], rq=tr.rq)
    want, probes = old.planes()
    got, gprobes = ref.planes(0, n_points=70, n_samples=2)
    assert probes == gprobes
    for name in ("ao", "light"):
        assert np.array_equal(want[name].view(np.uint32), got[name].view(np.uint32)), name
