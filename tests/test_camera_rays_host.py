"""Camera rays as arrays and their way back to pixels, the host half (include/dt.h dt_camera_rays_rows,
dt_camera_rays, dt_rays_resolve). No GPU.

1. The exports, the ABI version.
2. Every argument error returns DT_E_INVALID and a message that starts with the function's name and names the
   argument, before any device work (this machine has no device: a call that got past its checks would return
   DT_E_NO_DEVICE instead).
3. dt_camera_rays_rows against accum_doubles(g, tile) // 3 * ns for whole-image and tile-share globals in both
   layouts.
4. dt_rays_resolve on host arrays against the numpy restatement (tests/camera_rays_ref.py), bit for bit: width 1
   and 3, both modes, with and without shape, n_samples 1 and 9, a pixel with H = 0; a tile share in both
   layouts writes its own pixels only.
5. The host loop alone (csrc/dt_rays_resolve.h) in a stand-alone program under ASan and UBSan
   (tests/rays_resolve_host_check.cpp): arrays of the exact sizes, so a read or write past a row is reported."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import distraytracer_amd as dt
from distraytracer_amd import _lib
from oracle import geom as G

import camera_rays_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def _g(W, H):
    g = dt.globals_default()
    g.xRes, g.yRes = W, H
    return g


def _err():
    return dt.lib.dt_last_error().decode()


def test_exports_and_version():
    for name in ("dt_camera_rays_rows", "dt_camera_rays", "dt_rays_resolve"):
        assert name in _lib.EXPORTS and hasattr(dt.lib, name)
    assert dt.lib.dt_abi_version() == 8
    assert _lib.DT_CAMERA_RAYS_MAX_SAMPLES == 1024
    assert (_lib.DT_RESOLVE_MEAN, _lib.DT_RESOLVE_HIT_MEAN) == (0, 1) == (dt.RESOLVE_MODES["mean"], dt.RESOLVE_MODES["hit_mean"])
    for name in ("camera_rays", "rays_resolve", "peel_layers"):
        assert name in dt.__all__


def test_camera_rays_argument_errors_before_any_device_work():
    g = _g(8, 4)
    a = np.zeros((8 * 4, 1, 3))
    p = ctypes.c_void_p(a.ctypes.data)
    for args, word in [((None, 0, None, 0, 1, p, p), "null globals"), ((g, 0, None, 0, 1, None, p), "null start"),
                       ((g, 0, None, 0, 1, p, None), "null dir"), ((g, 0, None, -1, 1, p, p), "samples [-1,1)"),
                       ((g, 0, None, 3, 3, p, p), "samples [3,3)"), ((g, 0, None, 5, 2, p, p), "samples [5,2)"),
                       ((g, 0, None, 0, 1025, p, p), "at most 1024")]:
        gg = args[0]
        rc = dt.lib.dt_camera_rays(ctypes.byref(gg) if gg is not None else None, *args[1:], 0, None, None)
        assert rc == INVALID and _err().startswith("dt_camera_rays: ") and word in _err(), (word, rc, _err())
    bad = _g(0, 4)
    rc = dt.lib.dt_camera_rays(ctypes.byref(bad), 0, None, 0, 1, p, p, 0, None, None)
    assert rc == INVALID and _err().startswith("dt_camera_rays: globals or tiles"), _err()
    t = dt.tiles(rank=3, world=2)
    rc = dt.lib.dt_camera_rays(ctypes.byref(g), 0, ctypes.byref(t), 0, 1, p, p, 0, None, None)
    assert rc == INVALID and "rank out of range" in _err(), _err()
    assert dt.lib.dt_camera_rays_rows(None, None, 0, 1) == -1
    assert dt.lib.dt_camera_rays_rows(ctypes.byref(g), None, 2, 2) == -1
    assert dt.lib.dt_camera_rays_rows(ctypes.byref(g), None, 0, 1025) == -1
    # a legal range that spp and the 64-sample chunks would refuse elsewhere
    assert dt.lib.dt_camera_rays_rows(ctypes.byref(g), None, 70, 1094) == 8 * 4 * 1024
    with pytest.raises(dt.DTError, match="samples must be a pair"):
        dt.camera_rays(g, samples=3, host=True)
    with pytest.raises(dt.DTError, match="3 doubles for each of the 32 rows"):
        dt.camera_rays(g, out=(np.zeros((31, 3)), np.zeros((31, 3))))


def test_rays_resolve_argument_errors():
    g = _g(8, 4)
    v = np.zeros((32, 2, 3))
    o = np.zeros((32, 3), np.float32)
    pv, po = ctypes.c_void_p(v.ctypes.data), ctypes.c_void_p(o.ctypes.data)
    for args, word in [((None, None, 2, 3, pv, None, 0, po, None), "null globals"),
                       ((g, None, 2, 3, None, None, 0, po, None), "null values"),
                       ((g, None, 2, 3, pv, None, 0, None, None), "null out"),
                       ((g, None, 0, 3, pv, None, 0, po, None), "n_samples 0"),
                       ((g, None, 1025, 3, pv, None, 0, po, None), "n_samples 1025"),
                       ((g, None, 2, 0, pv, None, 0, po, None), "width 0"), ((g, None, 2, 4, pv, None, 0, po, None), "width 4"),
                       ((g, None, 2, 3, pv, None, 2, po, None), "mode 2")]:
        gg = args[0]
        for side in (0, 1):   # the checks come before the side is looked at
            rc = dt.lib.dt_rays_resolve(ctypes.byref(gg) if gg is not None else None, *args[1:], side, None)
            assert rc == INVALID and _err().startswith("dt_rays_resolve: ") and word in _err(), (word, rc, _err())
    with pytest.raises(dt.DTError, match="not 1..3 for each of 32 slots x 2 samples"):
        dt.rays_resolve(g, np.zeros((32, 2, 4)), 2)
    with pytest.raises(dt.DTError, match="mode must be one of"):
        dt.rays_resolve(g, v, 2, mode="median")
    with pytest.raises(dt.DTError, match="shape holds 10 elements"):
        dt.rays_resolve(g, v, 2, shape=np.zeros(10, np.int32))
    with pytest.raises(dt.DTError, match="float64"):
        dt.rays_resolve(g, v.astype(np.float32), 2)


SHARES = [None, dt.tiles(tile_w=32, tile_h=32, rank=1, world=2), dt.tiles(tile_w=32, tile_h=32, rank=1, world=2, layout=dt.DT_OUT_SLAB),
          dt.tiles(x0=3, y0=2, x1=60, y1=30, tile_w=16, tile_h=8, rank=2, world=3, layout=dt.DT_OUT_SLAB)]


@pytest.mark.parametrize("share", range(len(SHARES)))
def test_rows_follow_accum_doubles(share):
    tile = SHARES[share]
    g = _g(70, 37)
    for b, e in [(0, 1), (5, 13), (64, 66), (0, 1024)]:
        want = dt.accum_doubles(g, tile) // 3 * (e - b)
        assert dt.lib.dt_camera_rays_rows(ctypes.byref(g), ctypes.byref(tile) if tile else None, b, e) == want > 0
        assert dt.camera_rays_rows(g, (b, e), tile) == want
    x, y, own = R.slot_pixels(g, tile)
    assert len(own) == dt.accum_doubles(g, tile) // 3
    if tile is None:
        assert own.all()
    else:
        assert own.any() and not own.all()


def _rows(rng, slots, n, width):
    """random f64 rows of mixed magnitude and sign, so that the order of the additions shows in the last bits"""
    v = rng.standard_normal((slots, n, width)) * np.exp(rng.uniform(-12, 12, (slots, n, width)))
    shape = rng.integers(0, 40, (slots, n)).astype(np.int32)
    shape[rng.random((slots, n)) < 0.35] = -1
    shape[1] = -1          # a pixel with H = 0
    shape[2, : n // 2] = -1    # a run of misses
    shape[3] = 7           # a pixel where every row counts
    if n >= 3:             # a pixel whose sum shows its order after the cast too: left to right 0, reversed 1
        v[4] = 0
        v[4, 0], v[4, 1], v[4, 2] = 1.0, 1e17, -1e17
        shape[4] = 7
    return v, shape


@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("width", [1, 3])
def test_host_resolve_equals_the_restatement(n, width):
    g = _g(13, 7)
    slots = 13 * 7
    rng = np.random.default_rng(100 * n + width)
    v, shape = _rows(rng, slots, n, width)
    seen_h0 = False
    for mode in ("mean", "hit_mean"):
        for sh in (None, shape):
            got, cov = dt.rays_resolve(g, v, n, shape=sh, mode=mode, coverage=True)
            want, wcov = R.resolve_ref(v, n, width, shape=sh, mode=mode)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (slots, width)
            assert not G.differs(got.reshape(-1), want.reshape(-1)).any(), (mode, sh is None)
            assert not G.differs(cov, wcov).any()
            if sh is not None:
                assert cov[1] == 0 and cov[3] == 1
                if mode == "hit_mean":
                    assert (got[1] == 0).all()
                    seen_h0 = True
            else:
                assert (cov == 1).all()
            # without the coverage plane: the same plane
            assert not G.differs(dt.rays_resolve(g, v, n, shape=sh, mode=mode).reshape(-1), want.reshape(-1)).any()
    assert seen_h0
    # the order of the additions is observable on these rows: (1 + 1e17) - 1e17 is 0, the reversed sum 1
    if n > 1:
        rev, _ = R.resolve_ref(v[:, ::-1], n, width)
        fwd = dt.rays_resolve(g, v, n)
        assert (fwd[4] == 0).all() and (rev[4] == np.float32(1.0 / n)).all()


@pytest.mark.parametrize("share", [1, 2, 3])
def test_host_resolve_writes_owned_pixels_only(share):
    tile = SHARES[share]
    g = _g(70, 37)
    n, width = 3, 3
    x, y, own = R.slot_pixels(g, tile)
    slots = len(own)
    rng = np.random.default_rng(share)
    v, shape = _rows(rng, slots, n, width)
    out = np.full((slots, width), -7.5, np.float32)
    cov = np.full(slots, -7.5, np.float32)
    want, wcov = R.resolve_ref(v, n, width, shape=shape, mode="hit_mean", owned=own, out=out, coverage=cov)
    dt.rays_resolve(g, v, n, shape=shape, mode="hit_mean", tile=tile, coverage=True, out=(out, cov))
    assert not G.differs(out.reshape(-1), want.reshape(-1)).any()
    assert not G.differs(cov, wcov).any()
    assert (out[~own] == -7.5).all() and (cov[~own] == -7.5).all() and (cov[own] >= 0).all()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_host_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rays_resolve_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", "-I", os.path.join(ROOT, "distraytracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "rays_resolve_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
