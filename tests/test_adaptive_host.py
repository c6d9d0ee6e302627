"""Adaptive sampling, the host half (include/dt.h: dt_adapt_converged, dt_resolve_adaptive on host
arrays, and the argument checks of dt_render_window_adaptive that come before any device work). No GPU.

The convergence rule, with n = (double)count and thr2 = (tol / 255)^2, per channel:
    d = S2 - (S1 * S1) / n;  v = d / (n * (n - 1));  converged iff v <= thr2 for all three,
and only when count >= min_samples and count >= 64. numpy's f64 runs the same IEEE operations in
the same order as the library (built without contraction), so the agreement asked for is exact."""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt


def _rule(s1, s2, count, tol, min_samples):
    """the rule in numpy f64, operation for operation"""
    if count < 64 or count < min_samples:
        return False
    thr2 = (np.float64(tol) / np.float64(255.0)) * (np.float64(tol) / np.float64(255.0))
    n = np.float64(count)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            d = np.float64(s2[c]) - (np.float64(s1[c]) * np.float64(s1[c])) / n
            v = d / (n * (n - np.float64(1.0)))
            if not (v <= thr2):
                return False
    return True


def _globals(aa, w=40, h=24):
    g = dt.globals_default()
    g.xRes, g.yRes, g.antialias_samples = w, h, aa
    return g


def test_converged_matches_numpy_on_random_sums():
    """4000 random (s1, s2, count): sums of `count` colours in [0,1] with a spread drawn per case, so
    that both answers occur for the tolerances tried; the library and numpy agree on every one."""
    rng = np.random.default_rng(20261019)
    n_true = n_false = 0
    for i in range(4000):
        count = int(rng.choice([64, 100, 128, 192, 256, 1000]))
        spread = 10.0 ** rng.uniform(-4, -0.5)
        cols = np.clip(rng.uniform(0.2, 0.8, size=3) + spread * rng.standard_normal((count, 3)), 0, 1)
        s1 = np.zeros(3)
        s2 = np.zeros(3)
        for c in cols:
            s1 = s1 + c
            s2 = s2 + c * c
        tol = float(rng.choice([0.05, 0.25, 1.0, 4.0]))
        ms = int(rng.choice([0, 64, 128]))
        want = _rule(s1, s2, count, tol, ms)
        assert dt.adapt_converged(s1, s2, count, tol, ms) == want, (i, s1, s2, count, tol, ms)
        n_true += want
        n_false += not want
    assert n_true > 400 and n_false > 400, (n_true, n_false)


def test_converged_edge_cases():
    one = np.array([32.0, 64.0, 16.0])           # 64 samples of (0.5, 1.0, 0.25): zero variance
    sq = np.array([16.0, 64.0, 4.0])
    assert dt.adapt_converged(one, sq, 64, 0.5) is True
    assert dt.adapt_converged(one, sq, 64, 0.0) is True        # tol = 0: v = 0 <= 0
    # d slightly negative from rounding: counts as converged, at tol 0 too
    s1 = np.array([0.1 * 64, 0.1 * 64, 0.1 * 64])
    s2 = np.array([np.nextafter(s1[0] * s1[0] / 64, -np.inf)] * 3)
    assert s2[0] - (s1[0] * s1[0]) / 64 < 0
    assert _rule(s1, s2, 64, 0.0, 0) and dt.adapt_converged(s1, s2, 64, 0.0, 0) is True
    # tol = 0 with any variance: not converged
    assert dt.adapt_converged(one, sq + np.array([0, 0, 1e-9]), 64, 0.0) is False
    # a NaN channel never converges, whatever the tolerance
    for k in range(3):
        bad = one.copy()
        bad[k] = np.nan
        assert dt.adapt_converged(bad, sq, 64, 1e6) is False
        bad2 = sq.copy()
        bad2[k] = np.nan
        assert dt.adapt_converged(one, bad2, 64, 1e6) is False
    # count < min_samples, count < 64 (min_samples below 64 does not lower the floor)
    two = one * 2, sq * 2
    assert dt.adapt_converged(two[0], two[1], 128, 0.5, 128) is True
    assert dt.adapt_converged(two[0], two[1], 128, 0.5, 129) is False
    assert dt.adapt_converged(two[0], two[1], 128, 0.5, 256) is False
    assert dt.adapt_converged(one / 64 * 63, sq / 64 * 63, 63, 1e6, 0) is False
    assert dt.adapt_converged(one, sq, 64, 1e6, 0) is True
    assert dt.adapt_converged(one, sq, 0, 1e6, 0) is False and dt.adapt_converged(one, sq, 1, 1e6, 0) is False
    # a bad tolerance is an error
    for tol in (-1.0, float("nan"), float("inf")):
        with pytest.raises(dt.DTError, match="tol"):
            dt.adapt_converged(one, sq, 64, tol)


def test_host_resolve_adaptive_is_per_pixel_divide_clamp_scale():
    """dt_resolve_adaptive on host arrays against numpy, bit for bit: mixed counts including 0, values
    below 0 and above the count, a NaN pixel, a NaN in a pixel without samples (0: not counted)."""
    g = _globals(256, 5, 4)
    rng = np.random.default_rng(11)
    count = rng.choice([0, 64, 100, 128, 192, 256], size=20).astype(np.uint32)
    count[0], count[1], count[2], count[3], count[4] = 64, 0, 256, 128, 0
    a = rng.uniform(0.0, 1.0, size=60) * np.repeat(np.maximum(count, 1), 3)
    a[0], a[1], a[2] = -3.5, 64.0, 64.5
    a[3], a[4], a[5] = 7.0, np.nan, -2.0            # pixel 1: no samples
    a[6] = np.nan                                   # pixel 2: a NaN channel
    a[9] = 128 * (1.0 / 3.0)
    out = np.full(60, -1.0, dtype=np.float32)
    nan = dt.resolve_adaptive(g, a, count, out)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(np.repeat(count, 3) > 0, a / np.repeat(count, 3).astype(np.float64), 0.0)
        want = np.clip(np.float32(mean), np.float32(0), np.float32(1)) * np.float32(255)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert nan == 1
    assert out[0] == 0 and out[1] == 255 and out[2] == 255 and np.all(out[3:6] == 0) and np.isnan(out[6])
    assert np.all(out[12:15] == 0)
    with pytest.raises(dt.DTError):
        dt.resolve_adaptive(g, a, count[:-1], out)
    with pytest.raises(dt.DTError):
        dt.resolve_adaptive(g, a, count.astype(np.float32), out)


def test_render_window_adaptive_argument_checks_touch_no_device():
    """A null scene, each null buffer, a bad tol and a bad window: DT_E_INVALID each, dt_last_error
    naming the cause, before any device work (the stand-in addresses are never dereferenced)."""
    g = _globals(256)
    st = dt.Stats()
    fake = ctypes.c_void_p(64)
    f = dt.lib.dt_render_window_adaptive
    fa = dt.lib.dt_render_window_adaptive_async
    gp = ctypes.byref(g)

    def sync(scene, begin, end, acc, acc2, cnt, tol, ms=64):
        return f(scene, gp, 0, None, begin, end, acc, acc2, cnt, tol, ms, None, ctypes.byref(st))

    assert sync(None, 0, 64, fake, fake, fake, 0.5) == -1 and b"null scene" in dt.lib.dt_last_error()
    assert fa(None, gp, 0, None, 0, 64, fake, fake, fake, 0.5, 64, None) == -1
    assert b"null scene" in dt.lib.dt_last_error()
    assert f(fake, None, 0, None, 0, 64, fake, fake, fake, 0.5, 64, None, ctypes.byref(st)) == -1
    assert b"null argument" in dt.lib.dt_last_error()
    assert sync(fake, 0, 64, None, fake, fake, 0.5) == -1 and b"null accumulator" in dt.lib.dt_last_error()
    assert sync(fake, 0, 64, fake, None, fake, 0.5) == -1 and b"null accum2" in dt.lib.dt_last_error()
    assert sync(fake, 0, 64, fake, fake, None, 0.5) == -1 and b"null count" in dt.lib.dt_last_error()
    for tol in (-0.5, float("nan"), float("inf"), float("-inf")):
        assert sync(fake, 0, 64, fake, fake, fake, tol) == -1 and b"tol" in dt.lib.dt_last_error(), tol
        assert fa(fake, gp, 0, None, 0, 64, fake, fake, fake, tol, 64, None) == -1
    assert sync(fake, 32, 64, fake, fake, fake, 0.5) == -1 and b"multiple of 64" in dt.lib.dt_last_error()
    assert sync(fake, 0, 32, fake, fake, fake, 0.5) == -1 and b"multiple of 64 or spp" in dt.lib.dt_last_error()
    assert sync(fake, 192, 320, fake, fake, fake, 0.5) == -1 and b"end <= spp" in dt.lib.dt_last_error()
    g16 = _globals(16)
    assert f(fake, ctypes.byref(g16), 0, None, 0, 8, fake, fake, fake, 0.5, 64, None, ctypes.byref(st)) == -1
    assert b"the only window is [0,16)" in dt.lib.dt_last_error()
    assert dt.lib.dt_adapt_select_ms(None, None) == -1
