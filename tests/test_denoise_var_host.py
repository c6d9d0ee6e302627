"""Variance-guided preview denoising, the host half (include/dt.h dt_variance, dt_denoise_var): the exports
and the struct layout, the argument checks that come before any work, the host loops against the numpy
restatements of the specification (tests/denoise_var_ref.py) bit for bit, and the filter's properties.
No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd._lib import EXPORTS, DenoiseParams, DenoiseVarParams, Features

from denoise_ref import synthetic_planes
from denoise_var_ref import denoise_var_ref_params, synthetic_variance, variance_ref

INVALID = -1
INF = float("inf")
NAN = float("nan")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dt.h")


def params(levels=5, demodulate=1, sn=0.5, sz=0.1, sa=0.25, sv=3.0, vf=2.0):
    return DenoiseVarParams(levels, demodulate, sn, sz, sa, sv, vf, 0.0)


def _g(w, h):
    g = dt.globals_default()
    g.xRes, g.yRes = w, h
    return g


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, "%s: %d of %d floats differ, first at %d: %r vs %r" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def test_exports_and_abi_version():
    for name in ("dt_variance", "dt_denoise_var_params_default", "dt_denoise_var_workspace_floats", "dt_denoise_var"):
        assert name in EXPORTS and hasattr(dt.lib, name)
    assert dt.lib.dt_abi_version() == 8
    p = dt.denoise_var_params_default()
    assert (p.levels, p.demodulate) == (5, 1)
    assert all(0 < s < INF for s in (p.sigma_normal, p.sigma_depth, p.sigma_albedo, p.sigma_variance, p.variance_floor))


def test_params_layout_matches_c(tmp_path):
    """offsetof/sizeof of dt_denoise_var_params from gcc on include/dt.h vs the ctypes mirror"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){",
             'printf("size %zu\\n", sizeof(dt_denoise_var_params));']
    for f, _ in DenoiseVarParams._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(dt_denoise_var_params, %s));' % (f, f))
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(c)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(DenoiseVarParams) == 32
    for f, _ in DenoiseVarParams._fields_:
        assert int(got[f]) == getattr(DenoiseVarParams, f).offset, f


def _buffers(w, h):
    n = w * h
    return {"colour": np.full(3 * n, 100, np.float32), "variance": np.full(3 * n, 4, np.float32),
            "albedo": np.full(3 * n, 0.5, np.float32), "normal": np.zeros(3 * n, np.float32),
            "depth": np.ones(n, np.float32), "out": np.zeros(3 * n, np.float32),
            "work": np.zeros(16 * n + 4, np.float32)}


def _call(w, h, keep, p, colour=True, variance=True, feat=True, out=True, work=True, drop=None, out_ptr=None):
    f = Features()
    for name in ("albedo", "normal", "depth"):
        if name != drop:
            setattr(f, name, keep[name].ctypes.data)
    return dt.lib.dt_denoise_var(w, h, keep["colour"].ctypes.data if colour else None,
                                 keep["variance"].ctypes.data if variance else None,
                                 ctypes.byref(f) if feat else None, ctypes.byref(p) if p is not None else None,
                                 out_ptr if out_ptr is not None else (keep["out"].ctypes.data if out else None),
                                 keep["work"].ctypes.data if work else None, 0, None, None)


def _refused(rc, message):
    return rc == INVALID and message.encode() in dt.lib.dt_last_error()


def test_null_arguments_and_missing_planes_are_refused():
    keep, p = _buffers(4, 3), params()
    assert _call(4, 3, keep, p) == 0
    assert _refused(_call(4, 3, keep, p, colour=False), "dt_denoise_var: null colour")
    assert _refused(_call(4, 3, keep, p, variance=False), "dt_denoise_var: null variance")
    assert _refused(_call(4, 3, keep, p, feat=False), "dt_denoise_var: null feat")
    assert _refused(_call(4, 3, keep, None), "dt_denoise_var: null params")
    assert _refused(_call(4, 3, keep, p, out=False), "dt_denoise_var: null out")
    assert _refused(_call(4, 3, keep, p, work=False), "dt_denoise_var: null work")
    for plane in ("albedo", "normal", "depth"):
        assert _refused(_call(4, 3, keep, p, drop=plane), "dt_denoise_var: feat->%s missing" % plane)


def test_bad_sizes_and_params_are_refused():
    keep = _buffers(4, 3)
    assert _refused(_call(0, 3, keep, params()), "dt_denoise_var: xRes < 1")
    assert _refused(_call(4, -1, keep, params()), "dt_denoise_var: yRes < 1")
    for levels in (0, 7):
        assert _refused(_call(4, 3, keep, params(levels=levels)), "dt_denoise_var: levels outside 1..6")
    assert _refused(_call(4, 3, keep, params(demodulate=2)), "dt_denoise_var: demodulate must be 0 or 1")
    for field, name in (("sn", "sigma_normal"), ("sz", "sigma_depth"), ("sa", "sigma_albedo"), ("sv", "sigma_variance")):
        for bad in (0.0, -1.0, NAN, -INF):
            assert _refused(_call(4, 3, keep, params(**{field: bad})), "dt_denoise_var: %s must be > 0" % name), (name, bad)
        assert _call(4, 3, keep, params(**{field: INF})) == 0
    for bad in (0.0, -1.0, INF, NAN):
        assert _refused(_call(4, 3, keep, params(vf=bad)), "dt_denoise_var: variance_floor must be finite and > 0"), bad
    assert dt.lib.dt_denoise_var_workspace_floats(0, 3, None) < 0 and b"dt_denoise_var: xRes < 1" in dt.lib.dt_last_error()
    assert dt.lib.dt_denoise_var_workspace_floats(4, 0, None) < 0 and b"dt_denoise_var: yRes < 1" in dt.lib.dt_last_error()
    p7 = params(levels=7)
    assert dt.lib.dt_denoise_var_workspace_floats(4, 3, ctypes.byref(p7)) < 0
    assert dt.lib.dt_denoise_var_workspace_floats(4, 3, None) == len(keep["work"])


def test_aliasing_is_refused():
    keep, p = _buffers(4, 3), params()
    assert _refused(_call(4, 3, keep, p, out_ptr=keep["colour"].ctypes.data), "out aliases colour")
    assert _refused(_call(4, 3, keep, p, out_ptr=keep["colour"].ctypes.data + 4 * 35), "out aliases colour")
    assert _refused(_call(4, 3, keep, p, out_ptr=keep["variance"].ctypes.data + 4 * 35), "out aliases variance")
    assert _refused(_call(4, 3, keep, p, out_ptr=keep["work"].ctypes.data), "out aliases work")
    assert _refused(_call(4, 3, keep, p, out_ptr=keep["work"].ctypes.data + 4 * (16 * 12 + 3)), "out aliases work")


def test_variance_nulls_and_bad_globals_are_refused():
    g = _g(4, 3)
    a, a2 = np.zeros(36), np.zeros(36)
    c, v = np.zeros(12, np.uint32), np.zeros(36, np.float32)
    ptrs = [a.ctypes.data, a2.ctypes.data, c.ctypes.data, v.ctypes.data]
    assert dt.lib.dt_variance(ctypes.byref(g), None, *ptrs, 0, None) == 0
    for k in range(4):
        args = list(ptrs)
        args[k] = None
        assert _refused(dt.lib.dt_variance(ctypes.byref(g), None, *args, 0, None), "dt_variance: null argument"), k
    assert _refused(dt.lib.dt_variance(None, None, *ptrs, 0, None), "dt_variance: null argument")
    assert _refused(dt.lib.dt_variance(ctypes.byref(_g(0, 3)), None, *ptrs, 0, None), "dt_variance: invalid globals or tiles")
    bad_tile = dt.tiles(rank=3, world=2)
    assert _refused(dt.lib.dt_variance(ctypes.byref(g), ctypes.byref(bad_tile), *ptrs, 0, None),
                    "dt_variance: invalid globals or tiles")


def _seeded_sums(w, h, seed=5):
    """sums of n seeded sample colours per pixel, accumulated left to right as the sampler does: counts 0, 1,
    2, 64 and mixed; pixel 4 holds 64 identical samples (d is 0 up to rounding, either sign); pixel 5 a NaN sum"""
    rng = np.random.default_rng(seed)
    n_px = w * h
    count = rng.choice(np.array([0, 1, 2, 64, 128, 192, 7], np.uint32), n_px)
    count[:6] = [0, 1, 2, 64, 64, 64]
    s1, s2 = np.zeros((n_px, 3)), np.zeros((n_px, 3))
    for q in range(n_px):
        c = rng.uniform(0.0, 1.5, (int(count[q]), 3)) * rng.uniform(0.01, 1.0)
        if q == 4:
            c[:] = [0.1, 0.7, 1.0 / 3.0]
        for row in c:
            s1[q] += row
            s2[q] += row * row
    s1[5, 1] = np.nan
    return s1.reshape(-1), s2.reshape(-1), count


def test_variance_host_equals_numpy_reference_bit_for_bit():
    w, h = 16, 9
    s1, s2, count = _seeded_sums(w, h)
    got = dt.variance(_g(w, h), s1, s2, count)
    want = variance_ref(s1, s2, count)
    assert_same_bits(got, want, "dt_variance host vs numpy")
    v = got.reshape(-1, 3)
    assert (v[:2] == 0).all(), "counts 0 and 1 give no estimate"
    assert (v[2] > 0).all() and (v[3] > 0).all()
    assert (v[4] >= 0).all() and (v[4] < 1e-9).all(), "64 identical samples"
    assert v[5, 1] == 0 and v[5, 0] > 0, "a NaN sum gives 0, its neighbours in the pixel are untouched"
    assert np.isfinite(got).all() and (got >= 0).all()
    # int32 counts are read as uint32; a given out is returned
    out = np.empty(3 * w * h, np.float32)
    assert dt.variance(_g(w, h), s1, s2, count.astype(np.int32), out=out) is out
    assert_same_bits(out, want, "dt_variance with int32 counts")


def test_wrapper_checks_sizes_dtypes_and_sides():
    g = _g(4, 3)
    c, f = synthetic_planes(4, 3)
    v = synthetic_variance(4, 3)
    with pytest.raises(dt.DTError, match="variance holds"):
        dt.denoise(g, c, f, variance=v[:-3])
    with pytest.raises(dt.DTError, match="float32"):
        dt.denoise(g, c, f, variance=v.astype(np.float64))
    with pytest.raises(dt.DTError, match="must be a DenoiseVarParams"):
        dt.denoise(g, c, f, DenoiseParams(5, 1, 0.5, 0.1, 48.0, 0.25), variance=v)
    with pytest.raises(dt.DTError, match="needs a variance plane"):
        dt.denoise(g, c, f, params())
    with pytest.raises(dt.DTError, match="levels outside 1..6"):
        dt.denoise(g, c, f, params(levels=9), variance=v)
    with pytest.raises(dt.DTError, match="expected a contiguous float64"):
        dt.variance(g, np.zeros(36, np.float32), np.zeros(36), np.zeros(12, np.uint32))
    with pytest.raises(dt.DTError, match="need 12 elements"):
        dt.variance(g, np.zeros(36), np.zeros(36), np.zeros(11, np.uint32))
    out = np.zeros(36, np.float32)
    assert dt.denoise(g, c, f, params(), out=out, variance=v) is out


CASES = [(37, 23, lv, dm, {}) for lv in range(1, 7) for dm in (0, 1)]
CASES += [(130, 70, lv, dm, {}) for lv, dm in ((6, 1), (3, 0))]
CASES += [(37, 23, 5, 1, {k: INF}) for k in ("sn", "sz", "sa", "sv")]
CASES += [(37, 23, 3, 1, {"sn": INF, "sz": INF, "sa": INF}), (37, 23, 4, 1, {"sv": 0.75, "vf": 0.03125})]
CASES += [(1, 1, lv, dm, {}) for lv in (1, 6) for dm in (0, 1)] + [(1, 40, lv, dm, {}) for lv in (1, 4, 6) for dm in (0, 1)]


@pytest.mark.parametrize("w,h,levels,demod,sig", CASES)
def test_host_equals_numpy_reference_bit_for_bit(w, h, levels, demod, sig):
    """37x23: at steps 16 and 32 most taps fall outside the image (the border skip); 130x70: every step has
    taps inside; 1x1 and 1x40: none or one column of taps, and of the 3x3 prefilter, is ever inside"""
    c, f = synthetic_planes(w, h)
    v = synthetic_variance(w, h)
    p = params(levels=levels, demodulate=demod, **sig)
    got = dt.denoise(_g(w, h), c, f, p, variance=v)
    want = denoise_var_ref_params(w, h, c, v, f, p)
    assert_same_bits(got, want, "%dx%d levels %d demodulate %d %s" % (w, h, levels, demod, sig))
    if min(w, h) > 1 and not sig:
        assert np.mean(bits(got) != bits(c)) > 0.5, "the filter left most of the image as it was"


def test_variance_changes_the_result():
    """the plane is read: scaling it moves the output"""
    w, h = 37, 23
    c, f = synthetic_planes(w, h)
    v = synthetic_variance(w, h)
    a = dt.denoise(_g(w, h), c, f, params(), variance=v)
    b = dt.denoise(_g(w, h), c, f, params(), variance=v * np.float32(16))
    assert np.mean(bits(a) != bits(b)) > 0.25


def test_infinite_sigma_variance_is_dt_denoise_without_its_colour_term():
    """cv = 1/(inf * (vbar + vf)) = 0, so xc = 0 and R(xc) = 1, as with isc = 1/(inf*inf) = 0 in dt_denoise"""
    w, h = 37, 23
    c, f = synthetic_planes(w, h)
    v = synthetic_variance(w, h)
    for demod in (0, 1):
        got = dt.denoise(_g(w, h), c, f, params(levels=4, demodulate=demod, sv=INF), variance=v)
        want = dt.denoise(_g(w, h), c, f, DenoiseParams(4, demod, 0.5, 0.1, INF, 0.25))
        assert_same_bits(got, want, "sigma_variance=inf vs dt_denoise sigma_colour=inf, demodulate %d" % demod)


def _two_halves(n=40):
    """n x n, flat guides, two constant halves 40 apart in every channel: dist2 across the edge = 3*40^2 = 4800"""
    left = (np.arange(n * n) % n) < n // 2
    C = np.where(left[:, None], np.float32(80), np.float32(120)) * np.ones((1, 3), np.float32)
    f = {"albedo": np.full(3 * n * n, 0.5, np.float32), "normal": np.tile(np.float32([0, 1, 0]), n * n),
         "depth": np.full(n * n, 5, np.float32)}
    return np.ascontiguousarray(C.reshape(-1), np.float32), f, left


@pytest.mark.parametrize("levels", [1, 3])
def test_low_variance_keeps_an_edge_exactly(levels):
    """variance plane 1.0 everywhere (V = 3 over the three channels), sigma_variance 4, floor 1:
    sv2 * (vbar + vf) = 16 * 4 = 64, xc = 4800 / 64 = 75 >= 1: the weight across the edge is exactly 0, each
    half is a weighted mean of its own constant, and V only shrinks from level to level, so the edge holds at
    every level. Every pixel at least 2 * 2^(levels-1) from the border (the reach of the widest tap) stays
    within 1e-3 of its input: the rounding of S / Wt over 25 equal values of at most 120."""
    n = 40
    C, f, _ = _two_halves(n)
    out = dt.denoise(_g(n, n), C, f, params(levels=levels, demodulate=0, sv=4.0, vf=1.0),
                     variance=np.full(3 * n * n, 1.0, np.float32))
    m = 2 * 2 ** (levels - 1)
    inner = np.zeros((n, n), bool)
    inner[m:n - m, m:n - m] = True
    diff = np.abs(out - C).reshape(n, n, 3)[inner]
    assert diff.max() <= 1e-3, (levels, float(diff.max()))


def test_high_variance_blurs_the_same_edge():
    """variance plane 10000 everywhere (V = 30000): sv2 * (vbar + vf) = 16 * 30001, xc = 4800 / 480016 = 0.01,
    R(xc) = 0.98: the pixels touching the edge take two of their five tap columns from the other half,
    K-weights 0.25 + 0.0625 = 0.3125 of the row's 1.0: a move of about 0.3125 * 0.98 * 40 = 12 towards it;
    the test asks for more than 4"""
    n = 40
    C, f, left = _two_halves(n)
    out = dt.denoise(_g(n, n), C, f, params(levels=1, demodulate=0, sv=4.0, vf=1.0),
                     variance=np.full(3 * n * n, 10000.0, np.float32))
    o, c = out.reshape(n, n, 3), C.reshape(n, n, 3)
    move_left = o[:, n // 2 - 1] - c[:, n // 2 - 1]     # the left half's last column rises
    move_right = c[:, n // 2] - o[:, n // 2]            # the right half's first column falls
    assert move_left.min() > 4 and move_right.min() > 4, (float(move_left.min()), float(move_right.min()))
    assert move_left.max() < 20 and move_right.max() < 20
    assert np.abs(o[:, :n // 2 - 2] - c[:, :n // 2 - 2]).max() <= 1e-3, "one level reaches two pixels"


def test_nan_pixels_pass_through_and_do_not_spread():
    w, h = 37, 23
    c, f = synthetic_planes(w, h)
    v = synthetic_variance(w, h)
    q = np.flatnonzero(np.isnan(c))[0] // 3
    for demod in (0, 1):
        out = dt.denoise(_g(w, h), c, f, params(demodulate=demod), variance=v)
        assert_same_bits(out[3 * q:3 * q + 3], c[3 * q:3 * q + 3], "the NaN-colour pixel")
        rest = np.delete(out.reshape(-1, 3), q, axis=0)
        assert np.isfinite(rest).all(), "a NaN spread to a neighbour"


def test_out_is_untouched_outside_its_floats():
    w, h, guard = 37, 23, 64
    c, f = synthetic_planes(w, h)
    v = synthetic_variance(w, h)
    buf = np.full(3 * w * h + 2 * guard, -12345.0, np.float32)
    out = buf[guard:-guard]
    dt.denoise(_g(w, h), c, f, params(), out=out, variance=v)
    assert (buf[:guard] == -12345.0).all() and (buf[-guard:] == -12345.0).all()
    assert_same_bits(out, denoise_var_ref_params(w, h, c, v, f, params()), "out inside a guard band")
