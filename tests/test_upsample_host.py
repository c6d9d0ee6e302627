"""Guided upsampling of previews, the host half (include/dt.h dt_upsample): the exports and the struct
layout, the argument checks that come before any work, the host loop against the numpy restatement of the
specification (tests/upsample_ref.py) bit for bit, and the filter's properties. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd._lib import EXPORTS, Features, UpsampleParams

from denoise_ref import synthetic_planes
from upsample_ref import replicate, upsample_ref_params

INVALID = -1
INF = float("inf")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dt.h")

# full resolution and factor: 6x4 (every 3x3 window of the 3x2 low-resolution image is clipped), 74x46,
# 111x69 with the factor whose fx is not exactly representable, 148x92
SHAPES = [(6, 4, 2), (74, 46, 2), (111, 69, 3), (148, 92, 4)]


def params(factor=2, **kw):
    p = dt.upsample_params_default()
    p.factor = factor
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# default, no demodulation, every term off, and a tight set that rejects every tap on part of the image
PARAMS = {"default": {}, "nodemod": {"demodulate": 0},
          "guides-off": {"sigma_normal": INF, "sigma_depth": INF, "sigma_albedo": INF},
          "tight": {"sigma_normal": 0.05, "sigma_depth": 0.01}}


def _g(w, h):
    g = dt.globals_default()
    g.xRes, g.yRes = w, h
    return g


def planes(W, H, s):
    """independent synthetic planes at the two resolutions (the inputs are arbitrary)"""
    c_lo, f_lo = synthetic_planes(W // s, H // s, seed=7)
    _, f_hi = synthetic_planes(W, H, seed=11)
    return c_lo, f_lo, f_hi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, "%s: %d of %d floats differ, first at %d: %r vs %r" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def test_exports_and_abi_version():
    for name in ("dt_upsample_params_default", "dt_upsample"):
        assert name in EXPORTS and hasattr(dt.lib, name)
    assert dt.lib.dt_abi_version() == 8
    p = dt.upsample_params_default()
    assert (p.factor, p.demodulate) == (2, 1)
    assert all(0 < s < INF for s in (p.sigma_normal, p.sigma_depth, p.sigma_albedo))


def test_params_layout_matches_c(tmp_path):
    """offsetof/sizeof of dt_upsample_params from gcc on include/dt.h vs the ctypes mirror"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){",
             'printf("size %zu\\n", sizeof(dt_upsample_params));']
    for f, _ in UpsampleParams._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(dt_upsample_params, %s));' % (f, f))
    lines.append("return 0;}")
    c = tmp_path / "layout.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(c)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(UpsampleParams) == 24
    for f, _ in UpsampleParams._fields_:
        assert int(got[f]) == getattr(UpsampleParams, f).offset, f


@pytest.mark.parametrize("W,H,s", SHAPES)
@pytest.mark.parametrize("which", list(PARAMS))
def test_host_equals_numpy_reference_bit_for_bit(W, H, s, which):
    c_lo, f_lo, f_hi = planes(W, H, s)
    p = params(s, **PARAMS[which])
    info = {}
    want = upsample_ref_params(W, H, c_lo, f_lo, f_hi, p, info)
    got = dt.upsample(_g(W, H), c_lo, f_lo, f_hi, p)
    assert_same_bits(got, want, "%dx%d factor %d %s" % (W, H, s, which))
    if which == "tight":
        assert info["fallback"].any() and not info["fallback"].all(), "the tight set must take both paths"


def _nan_case(W, H, s, block):
    c_lo, f_lo, f_hi = planes(W, H, s)
    c_lo = np.where(np.isnan(c_lo), np.float32(50.0), c_lo)   # (synthetic_planes' own NaN pixel out of the way)
    c = c_lo.reshape(H // s, W // s, 3)
    r, x = (H // s) // 2, (W // s) // 2
    if block:
        c[r:r + 2, x:x + 2, 2] = np.nan
    else:
        c[r, x, 0] = np.nan
    return c.reshape(-1), f_lo, f_hi


@pytest.mark.parametrize("block,which", [(False, "default"), (False, "guides-off"), (True, "tight")])
def test_nan_pixels_do_not_spread(block, which):
    """one bad low-resolution pixel, and a 2x2 block of them under the tight set: a NaN reaches the output
    only where every tap was rejected and the nearest pixel is bad, and there it is the pixel's own colour"""
    W, H, s = 74, 46, 2
    c_lo, f_lo, f_hi = _nan_case(W, H, s, block)
    p = params(s, **PARAMS[which])
    info = {}
    want = upsample_ref_params(W, H, c_lo, f_lo, f_hi, p, info)
    got = dt.upsample(_g(W, H), c_lo, f_lo, f_hi, p)
    assert_same_bits(got, want, "NaN case %s" % which)
    nan_px = np.isnan(got).reshape(H, W, 3).any(axis=2)
    assert (nan_px == info["copied"]).all(), "a NaN outside the copied-through pixels"
    if block:
        assert info["copied"].any(), "the case must reach Wt == 0 on a bad nearest pixel"
        R, X = np.argwhere(info["copied"])[0]
        q = (R // s) * (W // s) + X // s
        assert_same_bits(got[3 * (R * W + X):3 * (R * W + X) + 3], c_lo[3 * q:3 * q + 3], "the copied pixel")
    if which == "guides-off":
        assert not nan_px.any()   # the spatial term alone always finds a good neighbour


def test_exact_recovery_of_a_one_pixel_checker():
    """What the feature is for: a one-pixel albedo checker under flat lighting. The low-resolution render
    sees albedo 0.5 and colour 50 everywhere, so E' = 100 at every tap, S/Wt is 100 within a few ulp and
    the full-resolution albedo puts the checker back: 20 / 80. Pixel replication gives 50: off by 30."""
    W, H, s = 24, 12, 2
    n_hi, n_lo = W * H, (W // s) * (H // s)
    R, X = np.mgrid[0:H, 0:W]
    a = np.where((R + X) % 2 == 0, np.float32(0.2), np.float32(0.8)).astype(np.float32)
    A_hi = np.repeat(a.reshape(-1), 3)
    up = np.tile(np.float32([0, 0, 1]), n_hi)
    f_hi = {"albedo": A_hi, "normal": up, "depth": np.full(n_hi, 5, np.float32)}
    f_lo = {"albedo": np.full(3 * n_lo, 0.5, np.float32), "normal": np.tile(np.float32([0, 0, 1]), n_lo),
            "depth": np.full(n_lo, 5, np.float32)}
    c_lo = np.full(3 * n_lo, 50, np.float32)
    out = dt.upsample(_g(W, H), c_lo, f_lo, f_hi)
    want = np.float32(100) * A_hi
    assert np.abs(out - want).max() <= 1e-3
    assert np.abs(replicate(W, H, s, c_lo) - want).min() >= 29.9


@pytest.mark.parametrize("s", [2, 3, 4])
def test_row_and_column_mapping(s):
    """The low-resolution colour encodes its own (row, column); with every guide term off and no
    demodulation an output pixel is a convex combination of the taps around (R div s, X div s), so its
    channels lie within those taps' rows and columns. A flipped-row mapping fails this. Rounding: S is 9
    products and 8 adds of non-negative terms, Wt 8 adds, one division: a factor (1 + g), g = 19u/(1-19u),
    u = 2^-24 (Higham, Accuracy and Stability, lemma 3.1)."""
    W, H = 24, 36
    w, h = W // s, H // s
    r, x = np.mgrid[0:h, 0:w]
    c_lo = np.stack([r + 1, x + 1, np.zeros_like(r)], axis=2).astype(np.float32).reshape(-1)
    n_hi, n_lo = W * H, w * h
    f_lo = {"albedo": np.zeros(3 * n_lo, np.float32), "normal": np.zeros(3 * n_lo, np.float32), "depth": np.zeros(n_lo, np.float32)}
    f_hi = {"albedo": np.ones(3 * n_hi, np.float32), "normal": np.ones(3 * n_hi, np.float32), "depth": np.ones(n_hi, np.float32)}
    p = params(s, demodulate=0, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)
    out = dt.upsample(_g(W, H), c_lo, f_lo, f_hi, p).reshape(H, W, 3)
    u = 2.0 ** -24
    grow = 1 + 19 * u / (1 - 19 * u)
    R, X = np.mgrid[0:H, 0:W]
    rc, xc = R // s, X // s
    for k, (c, n) in enumerate(((rc, h), (xc, w))):
        lo, hi = np.maximum(c - 1, 0) + 1, np.minimum(c + 1, n - 1) + 1
        assert (out[..., k] >= lo / grow).all() and (out[..., k] <= hi * grow).all(), k
    # and it interpolates: away from the border the row code grows along R by 1/s per pixel on average
    assert abs((out[H - s - 1, W // 2, 0] - out[s, W // 2, 0]) - (H - 2 * s - 1) / s) < 1.0


def _buffers(W, H, s):
    """the planes as slices of one array, each followed by a gap longer than out: an out that starts on a
    plane overlaps that plane and no other"""
    n_hi, n_lo = W * H, (W // s) * (H // s)
    sizes = [("colour_lo", 3 * n_lo, 100), ("lo.albedo", 3 * n_lo, 0.5), ("lo.normal", 3 * n_lo, 0), ("lo.depth", n_lo, 1),
             ("hi.albedo", 3 * n_hi, 0.5), ("hi.normal", 3 * n_hi, 0), ("hi.depth", n_hi, 1), ("out", 3 * n_hi, 0)]
    gap = 3 * n_hi + 16
    arena = np.zeros(sum(n + gap for _, n, _ in sizes) + gap, np.float32)
    keep, at = {"arena": arena, "lo": {}, "hi": {}}, gap
    for name, n, v in sizes:
        a = arena[at:at + n]
        a[:] = v
        at += n + gap
        if "." in name:
            keep[name[:2]][name[3:]] = a
        else:
            keep[name] = a
    return keep


def _call(W, H, keep, p, null=None, drop=None, out_ptr=None):
    fl, fh = Features(), Features()
    for f, side in ((fl, "lo"), (fh, "hi")):
        for name in ("albedo", "normal", "depth"):
            if (side, name) != drop:
                setattr(f, name, keep[side][name].ctypes.data)
    return dt.lib.dt_upsample(W, H, None if null == "colour_lo" else keep["colour_lo"].ctypes.data,
                              None if null == "feat_lo" else ctypes.byref(fl),
                              None if null == "feat_hi" else ctypes.byref(fh),
                              None if null == "params" else ctypes.byref(p),
                              out_ptr if out_ptr is not None else (None if null == "out" else keep["out"].ctypes.data),
                              0, None, None)


def _refused(rc, name):
    msg = dt.lib.dt_last_error()
    return rc == INVALID and msg.startswith(b"dt_upsample: ") and name.encode() in msg


def test_null_arguments_and_missing_planes_are_refused():
    keep, p = _buffers(8, 4, 2), params(2)
    assert _call(8, 4, keep, p) == 0
    for name in ("colour_lo", "feat_lo", "feat_hi", "params", "out"):
        assert _refused(_call(8, 4, keep, p, null=name), name), name
    for side in ("lo", "hi"):
        for plane in ("albedo", "normal", "depth"):
            assert _refused(_call(8, 4, keep, p, drop=(side, plane)), "feat_%s->%s" % (side, plane))


def test_bad_sizes_and_params_are_refused():
    keep = _buffers(12, 12, 2)
    assert _refused(_call(0, 12, keep, params(2)), "xRes")
    assert _refused(_call(12, -2, keep, params(2)), "yRes")
    for factor in (0, 1, 5, -2):
        assert _refused(_call(12, 12, keep, params(factor)), "factor"), factor
    assert _refused(_call(11, 12, keep, params(2)), "xRes")
    assert _refused(_call(12, 11, keep, params(2)), "yRes")
    assert _refused(_call(12, 10, keep, params(3)), "yRes")
    assert _refused(_call(12, 12, keep, params(2, demodulate=2)), "demodulate")
    for name in ("sigma_normal", "sigma_depth", "sigma_albedo"):
        for bad in (0.0, -1.0, float("nan"), -INF):
            assert _refused(_call(12, 12, keep, params(2, **{name: bad})), name), (name, bad)
        assert _call(12, 12, keep, params(2, **{name: INF})) == 0
    for factor in (2, 3, 4):
        assert _call(12, 12, keep, params(factor)) == 0   # (buffers sized for factor 2 hold the smaller ones)
    assert dt.lib.dt_abi_version() == 8


def test_aliasing_is_refused():
    keep, p = _buffers(8, 4, 2), params(2)
    assert _refused(_call(8, 4, keep, p, out_ptr=keep["colour_lo"].ctypes.data), "colour_lo")
    # out starting in front of an input and running into it
    assert _refused(_call(8, 4, keep, p, out_ptr=keep["colour_lo"].ctypes.data - 4 * 90), "colour_lo")
    for side in ("lo", "hi"):
        for plane in ("albedo", "normal", "depth"):
            assert _refused(_call(8, 4, keep, p, out_ptr=keep[side][plane].ctypes.data), "feat_%s->%s" % (side, plane))


def test_wrapper_checks_sizes_and_sides():
    g = _g(8, 4)
    c_lo, f_lo, f_hi = planes(8, 4, 2)
    with pytest.raises(dt.DTError, match="depth plane of feats_lo is missing"):
        dt.upsample(g, c_lo, {"albedo": f_lo["albedo"], "normal": f_lo["normal"]}, f_hi)
    with pytest.raises(dt.DTError, match="plane normal of feats_hi holds"):
        dt.upsample(g, c_lo, f_lo, dict(f_hi, normal=f_hi["normal"][:-3]))
    with pytest.raises(dt.DTError, match="colour_lo holds"):
        dt.upsample(g, c_lo[:-3], f_lo, f_hi)
    with pytest.raises(dt.DTError, match="float32"):
        dt.upsample(g, c_lo.astype(np.float64), f_lo, f_hi)
    with pytest.raises(dt.DTError, match="out must hold"):
        dt.upsample(g, c_lo, f_lo, f_hi, out=np.zeros(5, np.float32))
    with pytest.raises(dt.DTError, match="factor outside 2..4"):
        dt.upsample(g, c_lo, f_lo, f_hi, params(5))
    with pytest.raises(dt.DTError, match="not a multiple of factor 3"):
        dt.upsample(g, c_lo, f_lo, f_hi, params(3))
    with pytest.raises(dt.DTError, match="sigma_depth must be > 0"):
        dt.upsample(g, c_lo, f_lo, f_hi, params(2, sigma_depth=0.0))
    out = np.zeros(96, np.float32)
    assert dt.upsample(g, c_lo, dict(f_lo, coverage=None), f_hi, params(2), out=out) is out


def test_out_is_untouched_outside_its_floats():
    W, H, s, guard = 74, 46, 2, 64
    c_lo, f_lo, f_hi = planes(W, H, s)
    buf = np.full(3 * W * H + 2 * guard, -12345.0, np.float32)
    out = buf[guard:-guard]
    dt.upsample(_g(W, H), c_lo, f_lo, f_hi, params(s), out=out)
    assert (buf[:guard] == -12345.0).all() and (buf[-guard:] == -12345.0).all()
    assert_same_bits(out, upsample_ref_params(W, H, c_lo, f_lo, f_hi, params(s)), "out inside a guard band")


def test_low_res_globals():
    g = _g(1920, 1080)
    g.seed = 77
    for s in (2, 3, 4):
        lo = dt.low_res_globals(g, s)
        assert (lo.xRes, lo.yRes) == (1920 // s, 1080 // s)
        assert (lo.seed, lo.aspect, lo.antialias_samples, lo.fov) == (77, g.aspect, g.antialias_samples, g.fov)
        lo.xRes, lo.yRes = g.xRes, g.yRes
        assert bytes(lo) == bytes(g), "only xRes and yRes differ"
    assert (g.xRes, g.yRes) == (1920, 1080), "g itself is unchanged"
    with pytest.raises(dt.DTError, match="not a multiple"):
        dt.low_res_globals(g, 7)
    with pytest.raises(dt.DTError, match="not a multiple"):
        dt.low_res_globals(_g(96, 55), 2)
