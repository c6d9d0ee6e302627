"""First-hit feature buffers, the host half (include/dt.h dt_render_features): the export, the
argument checks that come before any device work, and the Python wrapper's checks of the planes. No GPU.

dt_render_features checks its arguments in the order scene, globals, out, planes, n_samples and looks
at the scene only after all of them (dt_api.cpp): where a check other than the scene's is meant, the
scene is a stand-in address that is never dereferenced, as in tests/test_progressive_host.py."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd._lib import EXPORTS, Features

INVALID = -1


def _globals(aa, w=40, h=24):
    g = dt.globals_default()
    g.xRes, g.yRes, g.antialias_samples = w, h, aa
    return g


def _planes(n_px):
    keep = [np.zeros(3 * n_px, np.float32), np.zeros(3 * n_px, np.float32), np.zeros(n_px, np.float32),
            np.zeros(n_px, np.float32), np.zeros(n_px, np.int32)]
    f = Features(*[a.ctypes.data for a in keep])
    return f, keep


def _call(scene, g, n, f):
    st = dt.Stats()
    return dt.lib.dt_render_features(scene, ctypes.byref(g) if g is not None else None, 0, None, n,
                                     ctypes.byref(f) if f is not None else None, 0, None, ctypes.byref(st))


def test_export_and_abi_version():
    assert "dt_render_features" in EXPORTS
    assert hasattr(dt.lib, "dt_render_features")
    assert dt.lib.dt_abi_version() == 8
    assert ctypes.sizeof(Features) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_null_arguments_are_refused_before_any_device_work():
    g = _globals(256)
    f, keep = _planes(40 * 24)
    fake = ctypes.c_void_p(64)
    assert _call(None, g, 64, f) == INVALID and b"null scene" in dt.lib.dt_last_error()
    assert _call(fake, None, 64, f) == INVALID and b"null globals" in dt.lib.dt_last_error()
    assert _call(fake, g, 64, None) == INVALID and b"null planes" in dt.lib.dt_last_error()
    assert _call(fake, g, 64, Features()) == INVALID and b"no plane wanted" in dt.lib.dt_last_error()


@pytest.mark.parametrize("aa,n,rule", [
    (256, 100, "end must be a multiple of 64 or spp"),
    (256, 32, "end must be a multiple of 64 or spp"),
    (256, 0, "begin < end"),
    (256, -64, "begin < end"),
    (256, 320, "end <= spp"),
    (121, 100, "end must be a multiple of 64 or spp"),
    (16, 8, "the only window is [0,16)"),
    (16, 64, "end <= spp"),
])
def test_bad_n_samples_is_refused(aa, n, rule):
    g = _globals(aa)
    f, keep = _planes(40 * 24)
    assert _call(ctypes.c_void_p(64), g, n, f) == INVALID
    assert rule.encode() in dt.lib.dt_last_error(), dt.lib.dt_last_error()


class _NoScene:
    handle = None


def test_wrapper_rejects_wrong_planes():
    """sizes from accum_doubles(g, tile), float32 planes and an int32 shape plane, one side"""
    g = _globals(256)
    n3 = dt.accum_doubles(g)
    with pytest.raises(dt.DTError, match="albedo holds"):
        dt.render_features(_NoScene, g, 0, out={"albedo": np.zeros(n3 - 3, np.float32)})
    with pytest.raises(dt.DTError, match="depth holds"):
        dt.render_features(_NoScene, g, 0, out={"depth": np.zeros(n3, np.float32)})
    with pytest.raises(dt.DTError, match="float32"):
        dt.render_features(_NoScene, g, 0, out={"normal": np.zeros(n3, np.float64)})
    with pytest.raises(dt.DTError, match="int32"):
        dt.render_features(_NoScene, g, 0, out={"shape": np.zeros(n3 // 3, np.float32)})
    with pytest.raises(dt.DTError, match="unknown plane"):
        dt.render_features(_NoScene, g, 0, out={"colour": np.zeros(n3, np.float32)})
    tile = dt.tiles(tile_w=8, tile_h=8, rank=1, world=3, layout=dt.DT_OUT_SLAB)
    with pytest.raises(dt.DTError, match="coverage holds"):
        dt.render_features(_NoScene, g, 0, tile=tile, out={"coverage": np.zeros(n3 // 3, np.float32)})
    # rightly sized planes reach the library, which refuses the null scene
    with pytest.raises(dt.DTError, match="null scene"):
        dt.render_features(_NoScene, g, 0, out={"coverage": np.zeros(n3 // 3, np.float32),
                                                "shape": np.zeros(n3 // 3, np.int32)})
    with pytest.raises(dt.DTError, match="null scene"):
        dt.render_features(_NoScene, g, 0, n_samples=64, tile=tile,
                           out={"albedo": np.zeros(dt.accum_doubles(g, tile), np.float32)})


def test_feature_images_are_the_cli_formulas():
    g = _globals(1, 2, 1)
    feats = {"albedo": np.array([0.5, 1.0, 2.0, 0.0, 0.25, 0.0], np.float32),
             "normal": np.array([-0.5, 0.5, 0.0, 0.0, 0.0, -0.25], np.float32),
             "depth": np.array([4.0, 1.0], np.float32), "coverage": np.array([1.0, 0.25], np.float32)}
    img = dt.feature_images(g, feats)
    assert img["albedo"].tolist() == [127.5, 255.0, 255.0, 0.0, 63.75, 0.0]
    assert img["normal"].tolist() == [63.75, 191.25, 127.5, 31.875, 31.875, 0.0]
    assert img["depth"].tolist() == [255.0] * 3 + [63.75] * 3
    assert img["coverage"].tolist() == [255.0] * 3 + [63.75] * 3
    assert all(v.dtype == np.float32 for v in img.values())
