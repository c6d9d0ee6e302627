"""Preview denoising, the host half (include/dt.h dt_denoise): the exports and the struct layout, the
argument checks that come before any work, the host loop against the numpy restatement of the
specification (tests/denoise_ref.py) bit for bit, and the filter's properties. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd._lib import EXPORTS, DenoiseParams, Features

from denoise_ref import denoise_ref_params, synthetic_planes

INVALID = -1
INF = float("inf")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dt.h")


def params(levels=5, demodulate=1, sn=0.5, sz=0.1, sc=48.0, sa=0.25):
    return DenoiseParams(levels, demodulate, sn, sz, sc, sa)


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
    for name in ("dt_denoise_params_default", "dt_denoise_workspace_floats", "dt_denoise"):
        assert name in EXPORTS and hasattr(dt.lib, name)
    assert dt.lib.dt_abi_version() == 8
    p = dt.denoise_params_default()
    assert (p.levels, p.demodulate) == (5, 1)
    assert all(0 < s < INF for s in (p.sigma_normal, p.sigma_depth, p.sigma_colour, p.sigma_albedo))


def test_params_layout_matches_c(tmp_path):
    """offsetof/sizeof of dt_denoise_params from gcc on include/dt.h vs the ctypes mirror"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){",
             'printf("size %zu\\n", sizeof(dt_denoise_params));']
    for f, _ in DenoiseParams._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(dt_denoise_params, %s));' % (f, f))
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(c)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(DenoiseParams) == 24
    for f, _ in DenoiseParams._fields_:
        assert int(got[f]) == getattr(DenoiseParams, f).offset, f


def _buffers(w, h):
    n = w * h
    keep = {"colour": np.full(3 * n, 100, np.float32), "albedo": np.full(3 * n, 0.5, np.float32),
            "normal": np.zeros(3 * n, np.float32), "depth": np.ones(n, np.float32),
            "out": np.zeros(3 * n, np.float32), "work": np.zeros(16 * n + 4, np.float32)}
    return keep


def _call(w, h, keep, p, colour=True, feat=True, out=True, work=True, drop=None, out_ptr=None):
    f = Features()
    for name in ("albedo", "normal", "depth"):
        if name != drop:
            setattr(f, name, keep[name].ctypes.data)
    return dt.lib.dt_denoise(w, h, keep["colour"].ctypes.data if colour else None, ctypes.byref(f) if feat else None,
                             ctypes.byref(p) if p is not None else None,
                             out_ptr if out_ptr is not None else (keep["out"].ctypes.data if out else None),
                             keep["work"].ctypes.data if work else None, 0, None, None)


def _refused(rc, message):
    return rc == INVALID and message.encode() in dt.lib.dt_last_error()


def test_null_arguments_and_missing_planes_are_refused():
    keep, p = _buffers(4, 3), params()
    assert _call(4, 3, keep, p) == 0
    assert _refused(_call(4, 3, keep, p, colour=False), "dt_denoise: null colour")
    assert _refused(_call(4, 3, keep, p, feat=False), "dt_denoise: null feat")
    assert _refused(_call(4, 3, keep, None), "dt_denoise: null params")
    assert _refused(_call(4, 3, keep, p, out=False), "dt_denoise: null out")
    assert _refused(_call(4, 3, keep, p, work=False), "dt_denoise: null work")
    for plane in ("albedo", "normal", "depth"):
        assert _refused(_call(4, 3, keep, p, drop=plane), "dt_denoise: feat->%s missing" % plane)


def test_bad_sizes_and_params_are_refused():
    keep = _buffers(4, 3)
    assert _refused(_call(0, 3, keep, params()), "xRes < 1")
    assert _refused(_call(4, -1, keep, params()), "yRes < 1")
    for levels in (0, 7, -1):
        assert _refused(_call(4, 3, keep, params(levels=levels)), "levels outside 1..6")
    assert _refused(_call(4, 3, keep, params(demodulate=2)), "demodulate must be 0 or 1")
    for field, name in (("sn", "sigma_normal"), ("sz", "sigma_depth"), ("sc", "sigma_colour"), ("sa", "sigma_albedo")):
        for bad in (0.0, -1.0, float("nan"), -INF):
            assert _refused(_call(4, 3, keep, params(**{field: bad})), "%s must be > 0" % name), (name, bad)
        assert _call(4, 3, keep, params(**{field: INF})) == 0
    assert dt.lib.dt_denoise_workspace_floats(0, 3, None) < 0 and b"xRes < 1" in dt.lib.dt_last_error()
    assert dt.lib.dt_denoise_workspace_floats(4, 0, None) < 0 and b"yRes < 1" in dt.lib.dt_last_error()
    p7 = params(levels=7)
    assert dt.lib.dt_denoise_workspace_floats(4, 3, ctypes.byref(p7)) < 0
    assert dt.lib.dt_denoise_workspace_floats(4, 3, None) == len(keep["work"])


def test_aliasing_is_refused():
    keep, p = _buffers(4, 3), params()
    assert _refused(_call(4, 3, keep, p, out_ptr=keep["colour"].ctypes.data), "out aliases colour")
    assert _refused(_call(4, 3, keep, p, out_ptr=keep["colour"].ctypes.data + 4 * 35), "out aliases colour")
    assert _refused(_call(4, 3, keep, p, out_ptr=keep["work"].ctypes.data), "out aliases work")
    assert _refused(_call(4, 3, keep, p, out_ptr=keep["work"].ctypes.data + 4 * (16 * 12 + 3)), "out aliases work")


def test_wrapper_checks_sizes_dtypes_and_sides():
    g = _g(4, 3)
    c, f = synthetic_planes(4, 3)
    with pytest.raises(dt.DTError, match="depth plane is missing"):
        dt.denoise(g, c, {"albedo": f["albedo"], "normal": f["normal"]})
    with pytest.raises(dt.DTError, match="plane normal holds"):
        dt.denoise(g, c, dict(f, normal=f["normal"][:-3]))
    with pytest.raises(dt.DTError, match="colour holds"):
        dt.denoise(g, c[:-3], f)
    with pytest.raises(dt.DTError, match="float32"):
        dt.denoise(g, c.astype(np.float64), f)
    with pytest.raises(dt.DTError, match="out must hold"):
        dt.denoise(g, c, f, out=np.zeros(5, np.float32))
    with pytest.raises(dt.DTError, match="levels outside 1..6"):
        dt.denoise(g, c, f, params(levels=9))
    out = np.zeros(36, np.float32)
    assert dt.denoise(g, c, dict(f, coverage=None, shape=None), params(), out=out) is out


CASES = [(37, 23, lv, dm, {}) for lv in range(1, 7) for dm in (0, 1)]
CASES += [(37, 23, 5, 1, {k: INF}) for k in ("sn", "sz", "sc", "sa")]
CASES += [(37, 23, 3, 1, {"sn": INF, "sz": INF, "sc": INF, "sa": INF})]
CASES += [(1, 1, lv, dm, {}) for lv in (1, 6) for dm in (0, 1)] + [(1, 40, lv, dm, {}) for lv in (1, 4, 6) for dm in (0, 1)]
CASES += [(40, 1, 6, 1, {})]


@pytest.mark.parametrize("w,h,levels,demod,sig", CASES)
def test_host_equals_numpy_reference_bit_for_bit(w, h, levels, demod, sig):
    """37x23: at steps 16 and 32 most taps fall outside the image (the border skip); 1x1 and 1x40: none
    or one column of taps is ever inside"""
    c, f = synthetic_planes(w, h)
    p = params(levels=levels, demodulate=demod, **sig)
    got = dt.denoise(_g(w, h), c, f, p)
    want = denoise_ref_params(w, h, c, f, p)
    assert_same_bits(got, want, "%dx%d levels %d demodulate %d %s" % (w, h, levels, demod, sig))
    if min(w, h) > 1 and not sig:
        assert np.mean(bits(got) != bits(c)) > 0.5, "the filter left most of the image as it was"


def test_nan_pixels_pass_through_and_do_not_spread():
    w, h = 37, 23
    c, f = synthetic_planes(w, h)
    nan_c = np.flatnonzero(np.isnan(c))
    assert nan_c.size == 1
    q = nan_c[0] // 3
    for demod in (0, 1):
        out = dt.denoise(_g(w, h), c, f, params(demodulate=demod))
        assert_same_bits(out[3 * q:3 * q + 3], c[3 * q:3 * q + 3], "the NaN-colour pixel")
        rest = np.delete(out.reshape(-1, 3), q, axis=0)
        assert np.isfinite(rest).all(), "a NaN spread to a neighbour"
        # the NaN-normal pixel (the last one) has weight 0 for every tap, its own included: with
        # demodulate=0 it keeps its colour
        if demod == 0:
            assert_same_bits(out[-3:], c[-3:], "the NaN-normal pixel")


def test_output_stays_within_its_side_of_a_normal_edge():
    """A two-plane step image, demodulate=0: the two halves have normals whose squared distance (2) over
    sigma_normal^2 (0.25) is 8 > 1, so the weight across the edge is exactly 0 and every output channel is
    a chain of convex combinations of its own side's inputs. Rounding: per level S is 25 products and 24
    adds of non-negative terms, Wt 24 adds, then one division: S/Wt = mean * (1 + t), |t| <= g = 50u/(1-50u),
    u = 2^-24 (Higham, Accuracy and Stability, lemma 3.1); L levels compound to (1 + g)^L."""
    w, h, levels = 33, 21, 5
    rng = np.random.default_rng(3)
    n = w * h
    left = (np.arange(n) % w) < 16
    N = np.where(left[:, None], np.float32([0, 1, 0]), np.float32([1, 0, 0])).astype(np.float32)
    C = np.where(left[:, None], rng.uniform(10, 50, (n, 3)), rng.uniform(150, 250, (n, 3))).astype(np.float32)
    f = {"albedo": np.full(3 * n, 0.5, np.float32), "normal": N.reshape(-1), "depth": np.full(n, 5, np.float32)}
    out = dt.denoise(_g(w, h), C.reshape(-1), f, params(levels=levels, demodulate=0, sc=INF)).reshape(n, 3)
    u = 2.0 ** -24
    grow = (1 + 50 * u / (1 - 50 * u)) ** levels
    for side in (left, ~left):
        for k in range(3):
            lo, hi = float(C[side, k].min()), float(C[side, k].max())
            assert out[side, k].min() >= lo / grow and out[side, k].max() <= hi * grow, (k, lo, hi)
    # and it did smooth: each side's spread shrank
    assert out[left].std() < 0.5 * C[left].std() and out[~left].std() < 0.5 * C[~left].std()


def test_out_is_untouched_outside_its_floats():
    w, h, guard = 37, 23, 64
    c, f = synthetic_planes(w, h)
    buf = np.full(3 * w * h + 2 * guard, -12345.0, np.float32)
    out = buf[guard:-guard]
    dt.denoise(_g(w, h), c, f, params(), out=out)
    assert (buf[:guard] == -12345.0).all() and (buf[-guard:] == -12345.0).all()
    assert_same_bits(out, denoise_ref_params(w, h, c, f, params()), "out inside a guard band")
