"""Temporal reuse, the host half (include/dt.h dt_camera_get, dt_reproject): the exports and the struct
layouts, the argument checks that come before any work, dt_camera_get against the oracle's primary rays, the
host loop against the numpy restatement of the specification (tests/temporal_ref.py) bit for bit, and the
properties the specification states exactly. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd._lib import EXPORTS, Camera, Features, History, TemporalParams

from denoise_ref import synthetic_planes
from denoise_var_ref import synthetic_variance
from temporal_ref import (CAMERAS, _g, assert_result_bits, assert_same_bits, bits, cameras, frames, params,
                          reproject_ref)

INVALID = -1
INF = float("inf")
NAN = float("nan")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dt.h")
f32 = np.float32


# ---- exports, layouts, argument checks -------------------------------------------------------------

def test_exports_and_abi_version():
    for name in ("dt_camera_get", "dt_temporal_params_default", "dt_reproject"):
        assert name in EXPORTS and hasattr(dt.lib, name)
    assert dt.lib.dt_abi_version() == 8
    p = dt.temporal_params_default()
    assert p.demodulate == 1 and 0 < p.alpha_min <= 1 and p.max_history >= 1
    assert 0 <= p.depth_tol < INF and 0 <= p.normal_tol < INF and 0 <= p.albedo_tol < INF


@pytest.mark.parametrize("cname,mirror,size", [("dt_camera", Camera, 128), ("dt_temporal_params", TemporalParams, 24),
                                               ("dt_history", History, 24)])
def test_struct_layouts_match_c(tmp_path, cname, mirror, size):
    """offsetof/sizeof from gcc on include/dt.h vs the ctypes mirror"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){",
             'printf("size %%zu\\n", sizeof(%s));' % cname]
    for f, _ in mirror._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f))
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(c)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(mirror) == size
    for f, _ in mirror._fields_:
        assert int(got[f]) == getattr(mirror, f).offset, f


class _Call:
    """a valid 4x3 call with variance and history, whose arguments the checks below spoil one at a time"""

    def __init__(self):
        n = 12
        self.cur = dt.camera(_g(4, 3))
        self.prev = dt.camera(_g(4, 3))
        # every plane in a slot of its own of one buffer, 256 elements apart: a pointer moved by less than a
        # plane's length overlaps one plane only
        names3 = ("colour", "variance", "albedo", "normal", "p_albedo", "p_normal", "h_colour", "h_var", "out", "out_var", "o_colour", "o_var")
        names1 = ("depth", "p_depth", "h_len", "o_len")
        self.fbuf = np.full(256 * (len(names3) + len(names1) + 1), 1.0, np.float32)
        self.ibuf = np.zeros(256 * 3, np.int32)
        self.a = {k: self.fbuf[256 * (i + 1):256 * (i + 1) + (3 * n if k in names3 else n)] for i, k in enumerate(names3 + names1)}
        self.a.update({k: self.ibuf[256 * i + 128:256 * i + 128 + n] for i, k in enumerate(("shape", "p_shape"))})
        self.p = params()

    def run(self, null=(), ptr=None, cur=None, prev=None, p=None, no_variance=False, first=False):
        """null: names passed as NULL; ptr: {name: address}"""
        a = self.a

        def at(k):
            if k in null or (no_variance and k in ("variance", "h_var", "o_var", "out_var")):
                return None
            return (ptr or {}).get(k, a[k].ctypes.data)
        f = Features(at("albedo"), at("normal"), at("depth"), None, at("shape"))
        pf = Features(at("p_albedo"), at("p_normal"), at("p_depth"), None, at("p_shape"))
        hi = History(at("h_colour"), at("h_var"), at("h_len"))
        ho = History(at("o_colour"), at("o_var"), at("o_len"))
        ref = lambda o, k: None if k in null or first else ctypes.byref(o)
        return dt.lib.dt_reproject(None if "cur" in null else ctypes.byref(cur or self.cur), at("colour"), at("variance"),
                                   None if "feat" in null else ctypes.byref(f), ref(prev or self.prev, "prev"),
                                   ref(pf, "prev_feat"), ref(hi, "hist_in"),
                                   None if "params" in null else ctypes.byref(p or self.p), at("out"), at("out_var"),
                                   None if "hist_out" in null else ctypes.byref(ho), 0, None, None)


def _refused(rc, message):
    return rc == INVALID and dt.lib.dt_last_error().startswith(b"dt_reproject: ") and message.encode() in dt.lib.dt_last_error()


def test_null_arguments_and_missing_planes_are_refused():
    c = _Call()
    assert c.run() == 0 and c.run(no_variance=True) == 0 and c.run(first=True) == 0
    assert c.run(null=("shape",)) == 0 and c.run(null=("p_shape",)) == 0
    for name in ("cur", "colour", "feat", "params", "out", "hist_out"):
        assert _refused(c.run(null=(name,)), "null " + name), name
    for name, msg in (("albedo", "feat->albedo missing"), ("normal", "feat->normal missing"), ("depth", "feat->depth missing"),
                      ("p_albedo", "prev_feat->albedo missing"), ("p_normal", "prev_feat->normal missing"), ("p_depth", "prev_feat->depth missing"),
                      ("h_colour", "hist_in->colour missing"), ("h_len", "hist_in->len missing"),
                      ("h_var", "hist_in->var missing"), ("o_colour", "hist_out->colour missing"),
                      ("o_len", "hist_out->len missing"), ("o_var", "hist_out->var missing"), ("out_var", "null out_var")):
        assert _refused(c.run(null=(name,)), msg), name
    assert _refused(c.run(null=("variance",)), "hist_in->var given without variance")
    assert _refused(c.run(null=("variance", "h_var")), "hist_out->var given without variance")
    assert _refused(c.run(null=("variance", "h_var", "o_var")), "out_var given without variance")
    # the previous camera, its planes and the history go together
    assert _refused(c.run(null=("prev",)), "null prev")
    assert _refused(c.run(null=("prev_feat",)), "null prev_feat")
    assert _refused(c.run(null=("hist_in",)), "null hist_in")


def test_bad_cameras_and_params_are_refused():
    c = _Call()
    assert _refused(c.run(prev=dt.camera(_g(5, 3))), "prev: a camera of another size than cur")
    assert _refused(c.run(prev=dt.camera(_g(4, 2))), "prev: a camera of another size than cur")
    bad = dt.camera(_g(4, 3))
    bad.xRes = 0
    assert _refused(c.run(cur=bad), "cur: xRes < 1")
    bad = dt.camera(_g(4, 3))
    bad.yRes = -2
    assert _refused(c.run(cur=bad), "cur: yRes < 1")
    assert _refused(c.run(p=params(demodulate=2)), "demodulate must be 0 or 1")
    for v in (0.0, -0.5, 1.5, NAN, INF):
        assert _refused(c.run(p=params(alpha_min=v)), "alpha_min outside (0, 1]"), v
    assert c.run(p=params(alpha_min=1.0)) == 0
    for v in (0.5, 0.0, -1.0, NAN):
        assert _refused(c.run(p=params(max_history=v)), "max_history must be >= 1"), v
    assert c.run(p=params(max_history=1.0)) == 0 and c.run(p=params(max_history=INF)) == 0
    for field in ("depth_tol", "normal_tol", "albedo_tol"):
        for v in (-1e-3, -INF, NAN):
            assert _refused(c.run(p=params(**{field: v})), field + " must be >= 0"), (field, v)
        assert c.run(p=params(**{field: 0.0})) == 0 and c.run(p=params(**{field: INF})) == 0


def test_aliasing_is_refused():
    c = _Call()
    a = c.a
    ins = {"colour": "colour", "variance": "variance", "albedo": "feat->albedo", "normal": "feat->normal",
           "depth": "feat->depth", "shape": "feat->shape", "p_albedo": "prev_feat->albedo", "p_normal": "prev_feat->normal", "p_depth": "prev_feat->depth",
           "p_shape": "prev_feat->shape", "h_colour": "hist_in->colour", "h_var": "hist_in->var", "h_len": "hist_in->len"}
    outs = {"out": "out", "out_var": "out_var", "o_colour": "hist_out->colour", "o_var": "hist_out->var",
            "o_len": "hist_out->len"}
    for o, oname in outs.items():
        for i, iname in ins.items():
            last = a[i].ctypes.data + 4 * (a[i].size - 1)   # one float of overlap is enough
            assert _refused(c.run(ptr={o: last}), "%s aliases %s" % (oname, iname)), (o, i)
    order = list(outs)
    for k, o in enumerate(order):
        for o2 in order[:k]:
            assert _refused(c.run(ptr={o: a[o2].ctypes.data}), "%s aliases %s" % (outs[o], outs[o2])), (o, o2)
    assert c.run() == 0


def test_wrapper_checks_sizes_sides_and_groups():
    w, h = 4, 3
    cur, prevs = cameras(w, h)
    c, f, pf, hist, v = frames(w, h)
    with pytest.raises(dt.DTError, match="colour holds"):
        dt.reproject(cur, c[:-3], f, None, None, None)
    with pytest.raises(dt.DTError, match="go together"):
        dt.reproject(cur, c, f, prevs["pan"], None, None)
    with pytest.raises(dt.DTError, match="history lacks the var plane"):
        dt.reproject(cur, c, f, prevs["pan"], pf, {"colour": hist["colour"], "len": hist["len"]}, variance=v)
    with pytest.raises(dt.DTError, match="feats lacks the depth plane"):
        dt.reproject(cur, c, {"albedo": f["albedo"], "normal": f["normal"]}, None, None, None)
    with pytest.raises(dt.DTError, match="float32"):
        dt.reproject(cur, c.astype(np.float64), f, None, None, None)
    with pytest.raises(dt.DTError, match="alpha_min outside"):
        dt.reproject(cur, c, f, None, None, None, params(alpha_min=0.0))
    out = np.zeros(3 * w * h, np.float32)
    assert dt.reproject(cur, c, f, None, None, None, out=out)[0] is out


# ---- dt_camera_get ---------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(7, 5), (160, 90)])
def test_camera_record_gives_the_oracles_primary_rays_bit_for_bit(w, h):
    """final(240)'s camera with aperture 0: or_primary_ray's ray of pixel (x, y) is (eye + focal_length*dir) - eye
    in f64, dir = (a*X + b*Y) - near_plane*Z with camera_ray's f32 a and b. Recomputed from the record in that
    operation order, the rays agree BIT FOR BIT (the order can be matched, so no tolerance is used); the starts
    are the eye."""
    from oracle import geom as G
    g = dt.globals_default()
    dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.aperture = w, h, 0.0
    cam = dt.camera(g)
    assert (cam.xRes, cam.yRes, cam.near_plane, cam.focal_length) == (w, h, g.near_plane, g.focal_length)
    start, d = G.or_primary_ray(g, 240, 0, 8 * w * h)
    start, d = start[::8].reshape(h, w, 3), d[::8].reshape(h, w, 3)   # sample 0 of pixel y*W + x
    eye, X, Y, Z = (np.array(list(v)) for v in (cam.eye, cam.X, cam.Y, cam.Z))
    y, x = np.mgrid[0:h, 0:w]
    a = f32(cam.l) + (f32(cam.r) - f32(cam.l)) * x.astype(f32) / f32(w)
    b = f32(cam.b) + (f32(cam.t) - f32(cam.b)) * y.astype(f32) / f32(h)
    assert a.dtype == np.float32 and b.dtype == np.float32
    dirv = (a.astype(np.float64)[..., None] * X + b.astype(np.float64)[..., None] * Y) - np.float64(cam.near_plane) * Z
    want = (eye + np.float64(cam.focal_length) * dirv) - eye
    assert (start == eye).all()
    assert (want.view(np.uint64) == d.view(np.uint64)).all(), float(np.abs(want - d).max())


def test_camera_record_refuses_a_degenerate_gaze_and_bad_globals():
    g = _g(8, 5)
    for k in range(3):
        g.lookingAt[k] = g.eye[k] + 2.0 * g.up[k]
    c = Camera()
    assert dt.lib.dt_camera_get(ctypes.byref(g), ctypes.byref(c)) == INVALID
    assert b"Gaze direction can't be equal to up vector" in dt.lib.dt_last_error()
    with pytest.raises(dt.DTError, match="Gaze direction"):
        dt.camera(g)
    assert dt.lib.dt_camera_get(None, ctypes.byref(c)) == INVALID and b"dt_camera_get: null argument" in dt.lib.dt_last_error()
    assert dt.lib.dt_camera_get(ctypes.byref(_g(8, 5)), None) == INVALID
    assert dt.lib.dt_camera_get(ctypes.byref(_g(0, 5)), ctypes.byref(c)) == INVALID
    assert b"dt_camera_get: invalid globals" in dt.lib.dt_last_error()


# ---- host loop = numpy, bit for bit ----------------------------------------------------------------

CASES = [(37, 23, cam, dm, var, sh, {}) for cam in CAMERAS for dm in (0, 1) for var in (False, True) for sh in (False, True)]
CASES += [(130, 70, cam, dm, var, True, {}) for cam in CAMERAS for dm, var in ((1, True), (0, False))]
CASES += [(w, h, cam, 1, var, True, {}) for w, h in ((1, 1), (1, 40)) for cam in CAMERAS for var in (False, True)]
CASES += [(37, 23, cam, 1, True, True, tol) for cam in ("pan", "back")
          for tol in ({"depth_tol": INF}, {"normal_tol": INF}, {"albedo_tol": INF},
                      {"depth_tol": INF, "normal_tol": INF, "albedo_tol": INF})]
CASES += [(37, 23, "pan", 1, True, True, {"alpha_min": 0.5, "max_history": 4.0, "depth_tol": 0.0, "normal_tol": 0.0, "albedo_tol": 0.0})]


@pytest.mark.parametrize("w,h,cam,demod,var,shapes,tol", CASES)
def test_host_equals_numpy_reference_bit_for_bit(w, h, cam, demod, var, shapes, tol):
    cur, prevs = cameras(w, h)
    c, f, pf, hist, v = frames(w, h, var, shapes)
    p = params(demodulate=demod, **tol)
    got = dt.reproject(cur, c, f, prevs[cam], pf, hist, p, variance=v)
    want = reproject_ref(cur, c, f, prevs[cam], pf, hist, p, variance=v)
    assert_result_bits(got, want, "%dx%d %s demodulate %d variance %d shapes %d %s" % (w, h, cam, demod, var, shapes, tol))


def _shares(w, h, cam, **kw):
    cur, prevs = cameras(w, h)
    c, f, pf, hist, v = frames(w, h, shapes=False)   # (the shape ids are a checker: a turn lands on other squares)
    _, ho, _ = dt.reproject(cur, c, f, prevs[cam], pf, hist, params(**kw), variance=v)
    return float(np.mean(ho["len"] > 1))


def test_the_cameras_exercise_what_they_are_meant_to():
    """the share of pixels that found a history, per camera, with the guide tests off: everything that is not
    sky-on-surface for identical and pan; a part for the 30 degree turn; none facing away. The backward step
    loses pixels to the 2 % depth test and gets them back with depth_tol = inf."""
    off = {"depth_tol": INF, "normal_tol": INF, "albedo_tol": INF}
    assert _shares(130, 70, "identical", **off) > 0.6 and _shares(130, 70, "pan", **off) > 0.6
    assert 0.1 < _shares(130, 70, "turn30", **off) < 0.7
    assert _shares(130, 70, "away", **off) == 0.0
    tight, loose = _shares(130, 70, "back", normal_tol=INF, albedo_tol=INF), _shares(130, 70, "back", **off)
    assert 0.02 < tight < loose, (tight, loose)
    cur, prevs = cameras(130, 70)
    c, f, pf, hist, v = frames(130, 70)
    a = dt.reproject(cur, c, f, prevs["pan"], pf, hist, params(), variance=v)[0]
    b = dt.reproject(cur, c, f, prevs["identical"], pf, hist, params(), variance=v)[0]
    assert np.mean(bits(a) != bits(b)) > 0.1, "a sub-pixel pan must change the interpolation"


# ---- exact properties ------------------------------------------------------------------------------

def test_first_frame_is_copied_through():
    w, h = 37, 23
    cur, _ = cameras(w, h)
    c, f, _, _, v = frames(w, h)
    for demod in (0, 1):
        out, ho, ov = dt.reproject(cur, c, f, None, None, None, params(demodulate=demod), variance=v)
        assert_same_bits(out, c, "out is C")
        assert_same_bits(ov, v, "out_var is Vc")
        nan = np.isnan(c.reshape(-1, 3)).any(axis=1)
        assert (ho["len"][~nan] == 1).all() and (ho["len"][nan] == 0).all() and nan.sum() == 1
        d = np.fmax(f["albedo"], f32(0.0625)) if demod else np.ones_like(c)
        assert_same_bits(ho["colour"], c / d, "history colour is E_p")
        with np.errstate(all="ignore"):
            assert_same_bits(ho["var"], v / (d * d), "history variance is Ve_p")


def test_alpha_min_one_keeps_the_current_frame():
    """alpha = fmaxf(1, 1/n) = 1: E_out = E_h + 1*(E_p - E_h), which is E_p up to the rounding of the two
    operations: both operands lie below 8192 = 2^13, so each rounding is at most half an ulp of 2^14, 2^-10,
    and the result is within 2^-9 of E_p"""
    w, h = 37, 23
    cur, prevs = cameras(w, h)
    c, f, pf, hist, _ = frames(w, h, variance=False)
    _, ho, _ = dt.reproject(cur, c, f, prevs["pan"], pf, hist, params(alpha_min=1.0))
    d = np.fmax(f["albedo"], f32(0.0625))
    e_p = c / d
    ok = ~np.isnan(e_p)
    assert np.abs(hist["colour"][~np.isnan(hist["colour"])]).max() < 8192 and np.abs(e_p[ok]).max() < 8192
    assert (np.abs(ho["colour"][ok] - e_p[ok]) <= 2.0 ** -9).all()
    assert (ho["len"] > 1).mean() > 0.3, "histories were found"


def test_nan_colour_pixel_is_copied_and_is_nobodys_history():
    w, h = 37, 23
    cur, prevs = cameras(w, h)
    c, f, pf, hist, v = frames(w, h)
    q = np.flatnonzero(np.isnan(c))[0] // 3
    out, ho, ov = dt.reproject(cur, c, f, prevs["pan"], pf, hist, params(), variance=v)
    assert_same_bits(out[3 * q:3 * q + 3], c[3 * q:3 * q + 3], "the NaN-colour pixel")
    assert_same_bits(ov[3 * q:3 * q + 3], v[3 * q:3 * q + 3], "its variance")
    assert ho["len"][q] == 0
    assert np.isfinite(np.delete(out.reshape(-1, 3), q, axis=0)).all()
    # the next call reads that history: the NaN reaches nobody, the pixel itself included
    c2 = c.copy()
    c2[3 * q:3 * q + 3] = 50.0
    out2, ho2, _ = dt.reproject(cur, c2, f, prevs["pan"], {"albedo": f["albedo"], "normal": f["normal"], "depth": f["depth"]}, ho,
                                params(depth_tol=INF, normal_tol=INF), variance=v)
    assert np.isfinite(out2).all() and np.isfinite(ho2["colour"]).all()
    assert (ho2["len"] > 1).mean() > 0.5


def test_a_nan_in_the_history_is_never_read_into_out():
    w, h = 37, 23
    cur, prevs = cameras(w, h)
    c, f, pf, hist, v = frames(w, h)
    assert np.isnan(hist["colour"]).sum() == 1
    hist["colour"] = hist["colour"].copy()
    hist["colour"][::7] = np.nan   # many more
    for cam in ("identical", "pan"):
        out, ho, _ = dt.reproject(cur, c, f, prevs[cam], pf, hist, params(depth_tol=INF, normal_tol=INF, albedo_tol=INF), variance=v)
        nan_in = np.isnan(c)
        assert not np.isnan(out[~nan_in]).any() and not np.isnan(ho["colour"][~nan_in]).any()


def test_a_shape_mismatch_alone_rejects_a_tap():
    """flat guides, every other test off, identical cameras: a pixel keeps its history unless the shape ids
    differ"""
    w, h = 16, 9
    n = w * h
    cur, prevs = cameras(w, h)
    c = np.full(3 * n, 100.0, np.float32)
    f = {"albedo": np.full(3 * n, 0.5, np.float32), "normal": np.tile(f32([0, 0, 1]), n), "depth": np.full(n, 5, np.float32),
         "shape": np.full(n, 3, np.int32)}
    pf = {"albedo": f["albedo"].copy(), "normal": f["normal"].copy(), "depth": f["depth"].copy(), "shape": np.full(n, 3, np.int32)}
    hist = {"colour": np.full(3 * n, 150.0, np.float32), "len": np.full(n, 4, np.float32)}
    p = params(depth_tol=INF, normal_tol=INF)
    _, ho, _ = dt.reproject(cur, c, f, prevs["identical"], pf, hist, p)
    assert (ho["len"] == 5).all()
    f["shape"] = f["shape"].copy()
    f["shape"][20:40] = 9
    _, ho, _ = dt.reproject(cur, c, f, prevs["identical"], pf, hist, p)
    assert (ho["len"][20:40] == 1).all() and (np.delete(ho["len"], np.s_[20:40]) == 5).all()
    del pf["shape"]   # one plane alone: no test
    _, ho, _ = dt.reproject(cur, c, f, prevs["identical"], pf, hist, p)
    assert (ho["len"] == 5).all()


def test_an_albedo_mismatch_alone_rejects_a_tap():
    """flat guides, identical cameras, the other tests off: with the previous frame's albedo 0.1 away in one
    channel (> 0.0625) every pixel starts over; 0.05 away (< 0.0625), or with albedo_tol = inf, every pixel
    keeps its history"""
    w, h = 16, 9
    n = w * h
    cur, prevs = cameras(w, h)
    c = np.full(3 * n, 100.0, np.float32)
    f = {"albedo": np.full(3 * n, 0.5, np.float32), "normal": np.tile(f32([0, 0, 1]), n), "depth": np.full(n, 5, np.float32)}
    hist = {"colour": np.full(3 * n, 150.0, np.float32), "len": np.full(n, 4, np.float32)}
    for delta, tol, want in ((0.1, 0.0625, 1), (0.05, 0.0625, 5), (0.1, INF, 5)):
        pf = {k: v.copy() for k, v in f.items()}
        pf["albedo"][1::3] += np.float32(delta)
        _, ho, _ = dt.reproject(cur, c, f, prevs["identical"], pf, hist, params(depth_tol=INF, normal_tol=INF, albedo_tol=tol))
        assert (ho["len"] == want).all(), (delta, tol)


def test_sky_reprojects_onto_sky_only():
    """the top half is sky (Z = 0) in both frames, the pan moves nothing across the horizon row except by
    interpolation: a sky pixel takes history only from sky taps, a surface pixel never from them, so the two
    constant history colours never mix"""
    w, h = 32, 20
    n = w * h
    cur, prevs = cameras(w, h)
    sky = (np.arange(n) // w) < h // 2
    z = np.where(sky, 0, 6).astype(np.float32)
    c = np.full(3 * n, 100.0, np.float32)
    f = {"albedo": np.full(3 * n, 0.5, np.float32), "normal": np.zeros(3 * n, np.float32), "depth": z}
    pf = {"albedo": f["albedo"].copy(), "normal": f["normal"].copy(), "depth": z.copy()}
    hist = {"colour": np.repeat(np.where(sky, f32(1000.0), f32(10.0)), 3).astype(np.float32), "len": np.full(n, 8, np.float32)}
    p = params(demodulate=0, normal_tol=INF, alpha_min=0.05)   # the depth test (2 %) is what keeps a surface off the sky
    for cam in ("identical", "pan"):
        _, ho, _ = dt.reproject(cur, c, f, prevs[cam], pf, hist, p)
        found = ho["len"] > 1
        assert found.mean() > 0.8
        e = ho["colour"].reshape(-1, 3)[:, 0]
        # E_out = E_h + (E_p - E_h)/9 with E_h exactly 1000 (sky) or 10 (surface), E_p = 100
        assert np.allclose(e[found & sky], 900.0, rtol=1e-5) and np.allclose(e[found & ~sky], 20.0, rtol=1e-5)
    # a surface in front of the previous frame's sky: nothing to take
    pf["depth"] = np.zeros(n, np.float32)
    _, ho, _ = dt.reproject(cur, c, f, prevs["identical"], pf, hist, p)
    assert (ho["len"][~sky] == 1).all() and (ho["len"][sky] > 1).all()


def test_nothing_is_written_outside_the_outputs():
    w, h, guard = 37, 23, 64
    n = w * h
    cur, prevs = cameras(w, h)
    c, f, pf, hist, v = frames(w, h)
    bufs = {k: np.full(size + 2 * guard, -12345.0, np.float32)
            for k, size in (("out", 3 * n), ("out_var", 3 * n), ("colour", 3 * n), ("var", 3 * n), ("len", n))}
    inner = {k: b[guard:-guard] for k, b in bufs.items()}
    got = dt.reproject(cur, c, f, prevs["pan"], pf, hist, params(), variance=v, out=inner["out"], out_var=inner["out_var"],
                       out_history={k: inner[k] for k in ("colour", "var", "len")})
    for k, b in bufs.items():
        assert (b[:guard] == -12345.0).all() and (b[-guard:] == -12345.0).all(), k
    assert_result_bits(got, reproject_ref(cur, c, f, prevs["pan"], pf, hist, params(), variance=v), "inside guard bands")


# ---- variance bookkeeping --------------------------------------------------------------------------

def test_three_pushes_of_a_constant_frame_give_v_v2_v3():
    """identical cameras, constant colour, Vc = v everywhere: out_var is v, then ((1/2)^2)*v + ((1/2)^2)*v = v/2,
    then ((1 - a)^2)*(v/2) + (a*a)*v with a = 1.0f/3.0f, which is v/3. The expected bits are the numpy
    restatement's. Against the stated values: a push is about a dozen rounded operations on the way from Vc to
    out_var (demodulation, the interpolation sum and its division, the blend, remodulation), each at most half
    an ulp, and the second push's error passes through the third: 8 ulp bounds it."""
    w, h = 16, 9
    n = w * h
    g = _g(w, h)
    vval = f32(7.3)
    c = np.full(3 * n, 100.0, np.float32)
    f = {"albedo": np.full(3 * n, 0.5, np.float32), "normal": np.tile(f32([0, 0, 1]), n), "depth": np.full(n, 5, np.float32)}
    v = np.full(3 * n, vval, np.float32)
    acc = dt.TemporalAccumulator(params())
    cam = dt.camera(g)
    rp, rf, rh = None, None, None
    for k in range(3):
        out, ov = acc.push(g, c, f, variance=v)
        ro, rh, rv = reproject_ref(cam, c, f, rp, rf, rh, params(), variance=v)
        rp, rf = cam, f
        assert_same_bits(ov, rv, "push %d: out_var vs numpy" % (k + 1))
        assert_same_bits(out, ro, "push %d: out vs numpy" % (k + 1))
        assert (acc.history_length() == k + 1).all()
        want = float(vval) / (k + 1)
        assert (np.abs(ov.astype(np.float64) - want) <= 8 * float(np.spacing(f32(want)))).all(), (k, ov[0], want)
        assert (np.abs(out - 100.0) <= 1e-4).all()
    assert_same_bits(acc.push(g, c, f, variance=v)[1][:3] * 0 + 1, np.ones(3, np.float32), "a fourth push runs")


def test_accumulator_restarts_and_resets():
    g = _g(16, 9)
    c, f = synthetic_planes(16, 9)
    acc = dt.TemporalAccumulator()
    assert acc.history_length() is None
    first = acc.push(g, c, f)
    assert_same_bits(first, c, "first push")
    acc.push(g, c, f)
    assert acc.history_length().max() == 2
    acc.reset()
    assert acc.history_length() is None
    assert_same_bits(acc.push(g, c, f), c, "first push after reset")
    c2, f2 = synthetic_planes(20, 9)
    assert_same_bits(acc.push(_g(20, 9), c2, f2), c2, "another resolution starts a new sequence")
