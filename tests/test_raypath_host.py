"""Path ray queries, the host half (include/dt.h dt_trace_rays_path): the export, every argument error (all before
any device work; the scene is a stand-in address that is never dereferenced, as in
tests/test_transmittance_host.py), n_rays == 0, the Python wrappers' own checks, and the restatement of
tests/raypath_ref.py against PathRef, whose per-sample chain it must be: on the unit scene's camera rays the
same samples end on a surface and follow the same number of bounces. Then the premise of
tests/test_gpu_raypath.py, asserted of the prediction: its ray set holds every kind of path it claims. No GPU.

DT_E_UNSUPPORTED needs a scene, and a scene needs a device: the GPU file."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
import raypath_ref as R
from distraytracer_amd import _lib
from features_path_ref import GLASS, STEEL, EPS, PathRef

INVALID = -1


def test_the_export_exists():
    assert "dt_trace_rays_path" in _lib.EXPORTS and hasattr(dt.lib, "dt_trace_rays_path")
    assert dt.lib.dt_abi_version() == 8
    assert _lib.DT_RAY_PATH_MAX_BOUNCES == 8 == dt.GUIDE_MAX_BOUNCES
    assert (_lib.DT_PATH_VOID, _lib.DT_PATH_MISS, _lib.DT_PATH_SURFACE, _lib.DT_PATH_CUT) == (0, 1, 2, 3)
    assert (R.VOID, R.MISS, R.SURFACE, R.CUT) == (dt.DT_PATH_VOID, dt.DT_PATH_MISS, dt.DT_PATH_SURFACE, dt.DT_PATH_CUT)
    for name in ("trace_rays_path", "ray_polyline", "pick"):
        assert name in dt.__all__ and callable(getattr(dt, name))
    assert dt.RAY_PATH_PLANES == R.PLANES == tuple(f for f, _ in _lib.RayPaths._fields_)


def test_struct_layout_matches_c(tmp_path):
    """offsetof/sizeof of dt_ray_paths from gcc on include/dt.h against the ctypes mirror, as tests/test_abi.py"""
    import os
    import subprocess
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dt.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % hdr, "int main(void){",
             'printf("size %zu\\n", sizeof(dt_ray_paths));']
    for f, _ in _lib.RayPaths._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(dt_ray_paths, %s));' % (f, f))
    lines.append('printf("codes %d %d %d %d %d\\n", DT_PATH_VOID, DT_PATH_MISS, DT_PATH_SURFACE, DT_PATH_CUT, '
                 'DT_RAY_PATH_MAX_BOUNCES);')
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(c)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.RayPaths)
    for f, _ in _lib.RayPaths._fields_:
        assert int(got[f]) == getattr(_lib.RayPaths, f).offset, f
    assert got["codes"].split() == ["0", "1", "2", "3", "8"]


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _call(scene, g, n, start, dir, K, out):
    st = dt.Stats()
    return dt.lib.dt_trace_rays_path(scene, ctypes.byref(g) if g is not None else None, n, _ptr(start), _ptr(dir), K,
                                     ctypes.byref(out) if out is not None else None, 0, None, ctypes.byref(st))


def test_argument_errors_come_before_any_device_work():
    g = dt.globals_default()
    N = 5
    start, dir = np.zeros((N, 3)), np.ones((N, 3))
    end = np.zeros(N, np.int32)
    scene = ctypes.c_void_p(0x1000)
    RP = _lib.RayPaths
    ok = dict(scene=scene, g=g, n=N, start=start, dir=dir, K=2, out=RP(end=end.ctypes.data))
    cases = [
        (dict(scene=None), b"null scene"),
        (dict(g=None), b"null globals"),
        (dict(start=None), b"null start"),
        (dict(dir=None), b"null dir"),
        (dict(out=None), b"null out"),
        (dict(out=RP()), b"every pointer is null"),
        (dict(n=-1), b"n_rays < 0"),
        (dict(K=-1), b"max_bounces must be in 0..8, got -1"),
        (dict(K=9), b"max_bounces must be in 0..8, got 9"),
        # the errors also come before the n_rays == 0 shortcut
        (dict(n=0, K=9), b"max_bounces"),
        (dict(n=0, out=RP()), b"every pointer is null"),
    ]
    for change, msg in cases:
        assert _call(**dict(ok, **change)) == INVALID, msg
        err = dt.lib.dt_last_error()
        assert err.startswith(b"dt_trace_rays_path: ") and msg in err, (msg, err)


def test_every_single_plane_is_a_plane():
    """an out with any one plane passes the "no plane" check: with a null scene the next error is reached"""
    g = dt.globals_default()
    buf = np.zeros(64, np.float64)
    for f, _ in _lib.RayPaths._fields_:
        out = _lib.RayPaths(**{f: buf.ctypes.data})
        assert _call(None, g, 1, buf, buf, 0, out) == INVALID
        assert dt.lib.dt_last_error() == b"dt_trace_rays_path: null scene"
        assert _call(ctypes.c_void_p(0x1000), g, -1, buf, buf, 0, out) == INVALID
        assert b"n_rays < 0" in dt.lib.dt_last_error(), f


def test_python_wrapper_checks():
    s, d = np.zeros((2, 3)), np.ones((2, 3))
    for K in (-1, 9, 1.0, True):
        with pytest.raises(dt.DTError, match=r"trace_rays_path: max_bounces must be an integer in 0\.\.8"):
            dt.trace_rays_path(None, dt.globals_default(), s, d, max_bounces=K)
    with pytest.raises(dt.DTError, match="unknown plane"):
        dt.trace_rays_path(None, dt.globals_default(), s, d, planes=("t",))
    with pytest.raises(dt.DTError, match="3 doubles per ray"):
        dt.trace_rays_path(None, dt.globals_default(), s, np.ones((3, 3)))
    g = dt.globals_default()
    with pytest.raises(dt.DTError, match="pick: pixel"):
        dt.pick(None, g, 0, g.xRes, 0)
    with pytest.raises(dt.DTError, match="ray_polyline: paths holds no 'seg_shape'"):
        dt.ray_polyline({"seg_point": np.zeros((1, 1, 3)), "start": np.zeros((1, 3))}, 0)


def test_ray_polyline_by_hand():
    paths = {"start": np.array([[0.0, 0, 0], [9.0, 9, 9]]),
             "seg_shape": np.array([[4, 2, -1], [-1, -1, -1]], np.int32),
             "seg_point": np.array([[[1.0, 0, 0], [1, 1, 0], [0, 0, 0]], [[0.0, 0, 0]] * 3])}
    assert dt.ray_polyline(paths, 0).tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0]]
    assert dt.ray_polyline(paths, 1).tolist() == [[9, 9, 9]]


@pytest.mark.parametrize("K", [0, 1, 2, 8])
def test_the_restatement_is_pathref_chain_on_camera_rays(K):
    """the same `ended` and `followed` as PathRef.trace(...).per_sample(K) on the unit scene's camera rays, and
    the same counters as PathRef.planes counts them"""
    ref, desc, g, keep = R.unit_ref()
    n = 2
    old = _pathref(n)
    s, d = R.camera_rays_ref(g, 0, n)
    planes, cnt, log = ref.trace(s, d, K)
    ended, fol = old.per_sample(K)
    mine_ended = np.isin(planes["end"], (R.SURFACE, R.CUT)).reshape(g.yRes, g.xRes, n)
    assert np.array_equal(mine_ended, ended) and ended.any() and not ended.all()
    assert np.array_equal(R.followed(planes["end"], planes["segments"]).reshape(g.yRes, g.xRes, n), fol)
    assert np.array_equal(planes["shape"] >= 0, mine_ended.reshape(-1))
    want, wcnt = old.planes(n, K)
    assert cnt == wcnt
    assert np.array_equal(planes["shape"].reshape(g.yRes, g.xRes, n)[:, :, 0], want["shape"])
    if K >= 1:
        assert fol.max() >= 1 and cnt["rays"] > len(s)
    if K == 0:
        assert (planes["end"] != R.SURFACE).all() and (planes["segments"] == 1).all()


_PATHREF = {}


def _pathref(n):
    if n not in _PATHREF:
        ref, desc, g, keep = R.unit_ref()
        _PATHREF[n] = PathRef(desc, g).trace(g, 0, n, 8)
    return _PATHREF[n]


def test_the_gpu_ray_set_holds_every_kind_of_path():
    """what tests/test_gpu_raypath.py's case 2 exercises, asserted of the prediction"""
    s, d, names = R.ray_set()
    assert len(s) == 64 * 3 + 17
    for K in (1, 2, 8):
        planes, cnt, log = R.prediction(K)
        assert set(planes["end"].tolist()) == {R.VOID, R.MISS, R.SURFACE, R.CUT}, K
        assert {R.REFLECT, R.REFRACT} <= R.codes_seen(log), K
    planes, cnt, log = R.prediction(8)
    for name in ("nan_start", "zero_dir", "inf"):
        i = names[name]
        assert (planes["end"][i] == R.VOID).all() and (planes["segments"][i] == 0).all(), name
        assert (planes["last_dir"][i] == 0).all() and (planes["seg_shape"][i] == -1).all(), name
    i = names["through_centre"][0]
    assert planes["end"][i] == R.VOID and planes["segments"][i] == 1 and planes["seg_shape"][i, 0] == R.GLASS_SPHERE
    assert planes["shape"][i] == -1 and planes["length"][i] > 0
    i = names["miss"]
    assert (planes["end"][i] == R.MISS).all() and (planes["segments"][i] == 1).all() and (planes["length"][i] == 0).all()
    # rays that start inside the glass sphere: inside = 1 at their first hit, and total internal reflection
    seg0, rule0 = log[0]["seg"], log[0]["rule"]
    ins = np.concatenate([names["inside"], names["inside_out"]])
    assert (seg0["inside"][ins] == 1).all() and (seg0["shape"][ins] == R.GLASS_SPHERE).all()
    tir = ins[rule0["chk"][ins] < 0]
    assert tir.size >= 1 and (rule0["code"][tir] == R.REFLECT).all()
    assert (rule0["code"][names["inside_out"]] == R.REFRACT).all()
    # a grazing hit on the steel sphere: the mirror rule stops at rn <= eps
    gz = names["grazing"]
    graze = gz[seg0["hit"][gz] & (seg0["shape"][gz] == R.STEEL_SPHERE) & (rule0["rn"][gz] <= EPS)]
    assert graze.size >= 1 and (rule0["code"][graze] == R.STOP).all()
    assert (planes["end"][graze] == R.SURFACE).all() and (planes["segments"][graze] == 1).all()
    assert log[0]["material"][names["steel"]][0] == STEEL and log[0]["material"][names["glass"]][0] == GLASS
    # paths of several lengths, and some cut at every K
    assert planes["segments"].max() >= 4
    assert cnt["rays"] > len(s)
