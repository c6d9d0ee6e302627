"""Specular-path feature buffers, the host half (include/dt.h dt_guide_bounce, dt_render_features_path): the
bounce rule's host export against its numpy restatement (tests/features_path_ref.py bounce_rule) bit for bit,
the restatement at max_bounces = 0 against the first-hit prediction of tests/test_gpu_features.py, and the
DT_E_INVALID checks of the new export, which come before any device work. No GPU (DT_E_UNSUPPORTED needs a
scene, and a scene needs a device: tests/test_gpu_features_path.py).

dt_render_features_path checks its arguments in the order scene, globals, out, planes, n_samples, max_bounces
and looks at the scene only after all of them (dt_api.cpp): where a check other than the scene's is meant, the
scene is a stand-in address that is never dereferenced, as in tests/test_features_host.py."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
import scene_gen
from distraytracer_amd._lib import EXPORTS, Features
from features_path_ref import (ALUMINUM, EPS, F_GLOSSY, GLASS, LINOLEUM, REFLECT, REFRACT, STEEL, STOP, WATER, PathRef,
                               bounce_rule)
from oracle import geom as G

INVALID = -1
N_PAIRS = 3000
NONE, OTHER = 0, 6


def _pairs(seed):
    """(in, n, p): N_PAIRS random directions with random fixNorm'ed normals, then the cases randomness does not
    reach: grazing pairs (rn <= eps), normals left on the ray's side (rn <= 0) and normal incidence"""
    rng = np.random.default_rng(seed)
    in_ = rng.normal(size=(N_PAIRS, 3))
    in_ /= np.sqrt((in_ * in_).sum(axis=1))[:, None]
    n = rng.normal(size=(N_PAIRS, 3))
    n /= np.sqrt((n * n).sum(axis=1))[:, None]
    n[(in_ * n).sum(axis=1) > 0] *= -1   # fixNorm
    # grazing: n turned to within 1e-3 of perpendicular to in
    k = N_PAIRS // 10
    side = np.cross(in_[:k], n[:k])
    side /= np.sqrt((side * side).sum(axis=1))[:, None]
    perp = np.cross(side, in_[:k])   # unit, perpendicular to in, on n's side
    c = rng.uniform(1e-5, 2e-3, size=k)[:, None]
    n[:k] = perp * np.sqrt(1 - c * c) - c * in_[:k]
    n[k:2 * k] *= -1                 # the wrong side: the mirror ray leaves into the surface
    axes = np.array([[0, 0, -1.0], [0, 1.0, 0], [-1.0, 0, 0], [0.6, 0, 0.8]])
    in_ = np.concatenate([in_, axes])
    n = np.concatenate([n, -axes])
    p = rng.uniform(-5, 5, size=in_.shape)
    return in_, n, p


def _host(g, material, flags, inside, in_, n, p):
    code = np.zeros(len(in_), np.int64)
    nd, ns = np.zeros((len(in_), 3)), np.zeros((len(in_), 3))
    D3 = ctypes.c_double * 3
    for i in range(len(in_)):
        a, b = D3(), D3()
        code[i] = dt.lib.dt_guide_bounce(ctypes.byref(g), int(material), int(flags), int(inside), D3(*in_[i]), D3(*n[i]),
                                         D3(*p[i]), a, b)
        nd[i], ns[i] = tuple(a), tuple(b)
    return code, nd, ns


_seen = {"codes": set(), "tir": 0, "grazing": 0, "normal_incidence": 0, "wrong_side": 0}

CASES = [(m, fl, ins, ng, rf) for m in (GLASS, STEEL, ALUMINUM, WATER, LINOLEUM) for fl, ng in ((0, 0), (F_GLOSSY, 0), (F_GLOSSY, 1))
         for ins in (0, 1) for rf in (1,)] + [(GLASS, 0, 0, 0, 0), (STEEL, 0, 1, 1, 0), (NONE, 0, 0, 0, 1), (OTHER, 0, 1, 1, 1)]


@pytest.mark.parametrize("material,flags,inside,nogloss,reflect", CASES)
def test_bounce_rule_is_the_numpy_rule(material, flags, inside, nogloss, reflect):
    g = dt.globals_default()
    g.nogloss, g.reflect = nogloss, reflect
    in_, n, p = _pairs(1000 * material + 10 * inside + nogloss)
    N = len(in_)
    want = bounce_rule(g, np.full(N, material), np.full(N, flags), np.full(N, inside), in_, n, p)
    code, nd, ns = _host(g, material, flags, inside, in_, n, p)
    assert np.array_equal(code, want["code"]), np.nonzero(code != want["code"])[0][:5]
    go = code != STOP
    if go.any():
        assert not G.differs(nd[go], want["dir"][go]).any() and not G.differs(ns[go], want["start"][go]).any()
    assert (nd[~go] == 0).all() and (ns[~go] == 0).all()   # STOP writes nothing
    specular = reflect and material in (GLASS, STEEL, ALUMINUM, WATER, LINOLEUM) and not (flags & F_GLOSSY and not nogloss)
    assert bool(want["specular"].all()) == bool(specular) and (specular or not go.any())
    if specular:
        _seen["codes"] |= set(code.tolist())
        mirror = code != REFRACT
        _seen["grazing"] += int((mirror & (want["rn"] > 0) & (want["rn"] <= EPS)).sum())
        _seen["wrong_side"] += int((mirror & want["refl_err"]).sum())
        if material == GLASS:
            if inside == 1:
                _seen["tir"] += int(((want["chk"] < 0) & (code == REFLECT)).sum())
            _seen["normal_incidence"] += int(((code == REFRACT) & ~np.isfinite(nd).all(axis=1)).sum())
            assert (code == REFRACT).any()
            # refraction bends towards the normal going in and away from it going out (Snell): a check of the
            # restatement itself, on the finite rays
            fin = (code == REFRACT) & np.isfinite(nd).all(axis=1)
            assert (np.einsum("ij,ij->i", nd[fin], n[fin]) < 0).all()


def test_the_set_held_every_case():
    """what the parametrised cases met (run alone, it runs them itself)"""
    if not _seen["codes"]:
        for case in CASES:
            test_bounce_rule_is_the_numpy_rule(*case)
    print(_seen)
    assert _seen["codes"] == {STOP, REFLECT, REFRACT}
    assert _seen["tir"] > 0 and _seen["grazing"] > 0 and _seen["normal_incidence"] > 0 and _seen["wrong_side"] > 0


def test_null_arguments_of_the_rule():
    g = dt.globals_default()
    D3 = ctypes.c_double * 3
    v = D3(0, 0, 1)
    args = [ctypes.byref(g), STEEL, 0, 0, v, v, v, v, v]
    for k in (0, 4, 5, 6, 7, 8):
        a = list(args)
        a[k] = None
        assert dt.lib.dt_guide_bounce(*a) == INVALID and b"dt_guide_bounce: null" in dt.lib.dt_last_error()
    assert dt.guide_bounce(g, NONE, 0, 0, (0, 0, -1), (0, 0, 1), (1, 2, 3)) == (STOP, None, None)
    code, nd, ns = dt.guide_bounce(g, STEEL, 0, 0, (0, 0, -1), (0, 0, 1), (1, 2, 3))
    assert code == REFLECT and nd == (0.0, 0.0, 1.0) and ns == (1.0, 2.0, 3.0 + EPS)


def test_zero_bounces_is_the_first_hit_prediction():
    from test_gpu_features import predict
    desc, g, keep = scene_gen.features(*scene_gen.CASES["unit"])
    g.xRes, g.yRes, g.antialias_samples = 24, 16, 9
    want, seen = predict(desc, g, 0, 9)
    got, cnt = PathRef(desc, g).trace(g, 0, 9, 0).planes(9, 0)
    cov = want["coverage"]
    assert ((cov > 0) & (cov < 1)).any() and (want["shape"] == 1).any() and (want["shape"] == 2).any()   # glass, steel
    for k in want:
        assert not G.differs(got[k].reshape(-1), want[k].reshape(-1)).any(), k
    assert (got["bounces"] == 0).all()
    assert cnt["rays"] == 24 * 16 * 9 and cnt["reflect_errors"] == 0
    assert all(cnt[k] == seen[k] for k in ("tex_fetches", "uv_out_of_range", "prism_norm_fallback"))


def _globals(aa, w=40, h=24):
    g = dt.globals_default()
    g.xRes, g.yRes, g.antialias_samples = w, h, aa
    return g


def _planes(n_px):
    keep = [np.zeros(3 * n_px, np.float32), np.zeros(3 * n_px, np.float32), np.zeros(n_px, np.float32),
            np.zeros(n_px, np.float32), np.zeros(n_px, np.int32)]
    return Features(*[a.ctypes.data for a in keep]), keep


def _call(scene, g, n, k, f, bounces=None):
    st = dt.Stats()
    return dt.lib.dt_render_features_path(scene, ctypes.byref(g) if g is not None else None, 0, None, n, k,
                                          ctypes.byref(f) if f is not None else None, bounces, 0, None, ctypes.byref(st))


def _err():
    return dt.lib.dt_last_error()


def test_exports_and_abi_version():
    assert "dt_render_features_path" in EXPORTS and "dt_guide_bounce" in EXPORTS
    assert hasattr(dt.lib, "dt_render_features_path") and hasattr(dt.lib, "dt_guide_bounce")
    assert dt.lib.dt_abi_version() == 8


def test_argument_errors_come_before_any_device_work():
    g = _globals(256)
    f, keep = _planes(40 * 24)
    fake = ctypes.c_void_p(64)
    pre = b"dt_render_features_path: "
    assert _call(None, g, 64, 2, f) == INVALID and _err().startswith(pre + b"null scene")
    assert _call(fake, None, 64, 2, f) == INVALID and _err().startswith(pre + b"null globals")
    assert _call(fake, g, 64, 2, None) == INVALID and _err().startswith(pre + b"null planes")
    assert _call(fake, g, 64, 2, Features()) == INVALID and _err().startswith(pre + b"no plane wanted")
    for k in (-1, 9, 1 << 20):
        assert _call(fake, g, 64, k, f) == INVALID and _err().startswith(pre + b"max_bounces"), _err()
    # the first-hit call's messages keep their own prefix
    st = dt.Stats()
    assert dt.lib.dt_render_features(None, ctypes.byref(g), 0, None, 64, ctypes.byref(f), 0, None, ctypes.byref(st)) == INVALID
    assert _err().startswith(b"dt_render_features: null scene")


@pytest.mark.parametrize("aa,n,rule", [
    (256, 100, "end must be a multiple of 64 or spp"),
    (256, 0, "begin < end"),
    (256, 320, "end <= spp"),
    (16, 8, "the only window is [0,16)"),
])
def test_bad_n_samples_is_refused(aa, n, rule):
    g = _globals(aa)
    f, keep = _planes(40 * 24)
    assert _call(ctypes.c_void_p(64), g, n, 2, f) == INVALID
    assert _err().startswith(b"dt_render_features_path: ") and rule.encode() in _err(), _err()


class _NoScene:
    handle = None


def test_wrapper_plane_names():
    """"bounces" is a plane of the path call only; sizes as the other one-per-pixel planes"""
    g = _globals(256)
    n3 = dt.accum_doubles(g)
    with pytest.raises(dt.DTError, match="unknown plane 'bounces'"):
        dt.render_features(_NoScene, g, 0, out={"bounces": np.zeros(n3 // 3, np.float32)})
    with pytest.raises(dt.DTError, match="bounces holds"):
        dt.render_features(_NoScene, g, 0, out={"bounces": np.zeros(n3, np.float32)}, specular_bounces=2)
    with pytest.raises(dt.DTError, match="dt_render_features_path.*null scene"):
        dt.render_features(_NoScene, g, 0, out={"bounces": np.zeros(n3 // 3, np.float32)}, specular_bounces=2)
    with pytest.raises(dt.DTError, match="max_bounces"):
        dt.render_features(type("S", (), {"handle": ctypes.c_void_p(64)}), g, 0, n_samples=64,
                           out={"depth": np.zeros(n3 // 3, np.float32)}, specular_bounces=9)
