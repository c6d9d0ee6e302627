"""Progressive rendering, the host half (include/dt.h: dt_accum_doubles, dt_window_check, dt_resolve on
host arrays, and the argument checks of dt_render_window that come before any device work). No GPU.

A window is the samples [begin, end) of every owned pixel, in whole 64-sample chunks (the unit one
wave traces); the accumulator has one double per float of the output, in its layout; dt_resolve is
the division and store of dt_render's epilogue (render_final_project.cpp:1213-1217: `/ sampled_n`,
then `clamp(c) * 255`, the clamp on the value converted to float)."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt


def _globals(aa, w=40, h=24):
    g = dt.globals_default()
    g.xRes, g.yRes, g.antialias_samples = w, h, aa
    return g


def test_accum_doubles_matches_the_output_layout():
    g = _globals(256, 40, 24)
    assert dt.accum_doubles(g) == 3 * 40 * 24
    assert dt.accum_doubles(g, dt.tiles()) == 3 * 40 * 24
    # an image-layout share still addresses the whole ppmOut image
    assert dt.accum_doubles(g, dt.tiles(tile_w=8, tile_h=8, rank=1, world=2)) == 3 * 40 * 24
    for rank in (0, 1, 2):
        tile = dt.tiles(tile_w=8, tile_h=8, rank=rank, world=3, layout=dt.DT_OUT_SLAB)
        assert dt.accum_doubles(g, tile) == dt.slab_floats(g, tile) > 0
    g.xRes = 0
    assert dt.lib.dt_accum_doubles(ctypes.byref(g), None) < 0


@pytest.mark.parametrize("aa,begin,end", [(256, 0, 64), (256, 64, 128), (256, 192, 256), (256, 0, 256),
                                          (100, 64, 100), (100, 0, 100), (16, 0, 16), (1, 0, 1)])
def test_window_check_accepts(aa, begin, end):
    g = _globals(aa)
    assert dt.lib.dt_window_check(ctypes.byref(g), begin, end) == 0
    dt.window_check(g, begin, end)


@pytest.mark.parametrize("aa,begin,end,rule", [
    (256, 32, 64, "begin must be a multiple of 64"),
    (256, 0, 32, "end must be a multiple of 64 or spp"),
    (256, 64, 64, "begin < end"),
    (256, -64, 64, "0 <= begin"),
    (256, 192, 320, "end <= spp"),
    (100, 0, 128, "end <= spp"),
    (16, 0, 8, "the only window is [0,16)"),
])
def test_window_check_rejects(aa, begin, end, rule):
    g = _globals(aa)
    assert dt.lib.dt_window_check(ctypes.byref(g), begin, end) == -1   # DT_E_INVALID
    assert rule.encode() in dt.lib.dt_last_error(), dt.lib.dt_last_error()
    with pytest.raises(dt.DTError):
        dt.window_check(g, begin, end)


def test_window_check_uses_sampled_n():
    """spp = int(sqrt(antialias_samples))^2 (cpp:1046,1061): 10 samples are 9, 70 are 64."""
    assert dt.lib.dt_window_check(ctypes.byref(_globals(10)), 0, 9) == 0
    assert dt.lib.dt_window_check(ctypes.byref(_globals(10)), 0, 10) == -1
    assert dt.lib.dt_window_check(ctypes.byref(_globals(70)), 0, 64) == 0
    assert dt.lib.dt_window_check(ctypes.byref(_globals(70)), 0, 70) == -1


def test_render_window_argument_checks_touch_no_device():
    """A null scene, a null accumulator and a bad window: DT_E_INVALID each, before any device work
    and before the scene is looked at (this machine has no device to build one on: the stand-in
    scene and accumulator addresses are never dereferenced, the checks come first)."""
    g = _globals(256)
    st = dt.Stats()
    fake = ctypes.c_void_p(64)
    rc = dt.lib.dt_render_window(None, ctypes.byref(g), 0, None, 0, 64, fake, None, ctypes.byref(st))
    assert rc == -1 and b"null scene" in dt.lib.dt_last_error()
    rc = dt.lib.dt_render_window_async(None, ctypes.byref(g), 0, None, 0, 64, fake, None)
    assert rc == -1 and b"null scene" in dt.lib.dt_last_error()
    rc = dt.lib.dt_render_window(fake, ctypes.byref(g), 0, None, 0, 64, None, None, ctypes.byref(st))
    assert rc == -1 and b"null argument" in dt.lib.dt_last_error()
    rc = dt.lib.dt_render_window(fake, ctypes.byref(g), 0, None, 32, 64, fake, None, ctypes.byref(st))
    assert rc == -1 and b"multiple of 64" in dt.lib.dt_last_error()
    rc = dt.lib.dt_render_window_async(fake, ctypes.byref(g), 0, None, 0, 32, fake, None)
    assert rc == -1 and b"multiple of 64 or spp" in dt.lib.dt_last_error()


@pytest.mark.parametrize("n", [1, 64, 100])
def test_host_resolve_is_divide_clamp_scale(n):
    """dt_resolve on host arrays against numpy's f64 divide, f32 convert, clip, f32 multiply, bit for
    bit: values below 0, above n (clamped to 255), in between, a NaN pixel, and the NaN count."""
    g = _globals(256, 4, 3)
    rng = np.random.default_rng(7 + n)
    a = rng.uniform(0.0, float(n), size=3 * 4 * 3)
    a[0], a[1], a[2] = -3.5, -0.25, -float(n)            # below 0 -> 0
    a[3], a[4], a[5] = n + 0.5, 1e30, float(n)           # above n -> 255 ; exactly n -> 255
    a[6] = n * (1.0 / 3.0)
    a[7] = 5e-324                                        # a denormal sum
    a[9] = np.nan                                        # pixel 3: one NaN channel
    a[12], a[13] = np.nan, np.nan                        # pixel 4: two
    a[16] = np.inf                                       # pixel 5: +inf -> 255
    out = np.full(a.size, -1.0, dtype=np.float32)
    nan = dt.resolve(g, a, n, out)
    with np.errstate(invalid="ignore"):
        want = np.clip(np.float32(a / n), np.float32(0), np.float32(1)) * np.float32(255)
    assert want.dtype == np.float32
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert nan == 2
    assert out[0] == 0 and out[2] == 0 and out[3] == 255 and out[5] == 255 and out[16] == 255
    assert np.isnan(out[9]) and np.isnan(out[12]) and not np.isnan(out[10])


def test_host_resolve_slab_layout_and_errors():
    g = _globals(256, 40, 24)
    tile = dt.tiles(tile_w=8, tile_h=8, rank=1, world=3, layout=dt.DT_OUT_SLAB)
    n = dt.accum_doubles(g, tile)
    a = np.linspace(0.0, 64.0, n)
    out = np.zeros(n, dtype=np.float32)
    assert dt.resolve(g, a, 64, out, tile) == 0
    assert np.array_equal(out, np.clip(np.float32(a / 64), 0, 1) * np.float32(255))
    with pytest.raises(dt.DTError, match="n_samples"):
        dt.resolve(g, a, 0, out, tile)
    with pytest.raises(dt.DTError):
        dt.resolve(g, a[:-3], 64, out, tile)   # shorter than the layout
    with pytest.raises(dt.DTError):
        dt.resolve(g, a.astype(np.float32), 64, out, tile)
