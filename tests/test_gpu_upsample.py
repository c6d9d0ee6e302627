"""Guided upsampling of previews on the device (include/dt.h dt_upsample; dt_upsample.hip): the kernel
against the host loop and the numpy restatement of the specification (tests/upsample_ref.py), bit for bit,
on synthetic planes and on the planes of a real preview; the quality gate (the upsampled half-resolution
frame is closer to the full-resolution frame than its pixel replication); renderImage and the CLI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
from distraytracer_amd._lib import Features

from parity_check import _log, log_equal
from test_upsample_host import PARAMS, SHAPES, _g, _nan_case, params, planes
from upsample_ref import replicate, upsample_ref_params

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTRENDER = os.path.join(os.path.dirname(HERE), "distraytracer_amd", "dtrender")
NAMES = ("albedo", "normal", "depth")


def _dev(*a):
    return [{k: torch.from_numpy(v).cuda() for k, v in x.items()} if isinstance(x, dict) else torch.from_numpy(x).cuda()
            for x in a]


def _np(feats):
    return {k: v.cpu().numpy() for k, v in feats.items()}


def _guarded(g, c_lo, f_lo, f_hi, p):
    """dt.upsample on the device into an out with a guard band of 256 floats on each side"""
    n, guard = 3 * g.xRes * g.yRes, 256
    buf = torch.full((n + 2 * guard,), -12345.0, dtype=torch.float32, device="cuda")
    dc, dl, dh = _dev(c_lo, f_lo, f_hi)
    dt.upsample(g, dc, dl, dh, p, out=buf[guard:guard + n])
    got = buf.cpu().numpy()
    assert (got[:guard] == -12345.0).all() and (got[-guard:] == -12345.0).all(), "written outside out"
    return got[guard:-guard]


# the host test's shapes; 260x140: five work-groups in x, 35 in y, 260 no multiple of 64; and the lane boundary
# of the (64, 4) block: a width of exactly 64 (no idle lane) and the next the factor allows (a second block
# with s live lanes), with a height that leaves rows of the last block idle where the factor allows one
@pytest.mark.parametrize("W,H,s", SHAPES + [(260, 140, 2), (64, 6, 2), (66, 6, 2), (64, 12, 4), (68, 12, 4)])
@pytest.mark.parametrize("which", list(PARAMS))
def test_device_equals_host_equals_numpy(cuda, W, H, s, which):
    c_lo, f_lo, f_hi = planes(W, H, s)
    p = params(s, **PARAMS[which])
    want = upsample_ref_params(W, H, c_lo, f_lo, f_hi, p)
    host = dt.upsample(_g(W, H), c_lo, f_lo, f_hi, p)
    got = _guarded(_g(W, H), c_lo, f_lo, f_hi, p)
    log_equal("upsample %dx%d x%d %s host vs numpy" % (W, H, s, which), host.view(np.uint32), want.view(np.uint32))
    log_equal("upsample %dx%d x%d %s device vs numpy" % (W, H, s, which), got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("block,which", [(False, "default"), (False, "guides-off"), (True, "tight")])
def test_nan_pixels_on_the_device(cuda, block, which):
    W, H, s = 74, 46, 2
    c_lo, f_lo, f_hi = _nan_case(W, H, s, block)
    p = params(s, **PARAMS[which])
    info = {}
    want = upsample_ref_params(W, H, c_lo, f_lo, f_hi, p, info)
    got = _guarded(_g(W, H), c_lo, f_lo, f_hi, p)
    log_equal("upsample NaN case %s device vs numpy" % which, got.view(np.uint32), want.view(np.uint32))
    assert (np.isnan(got).reshape(H, W, 3).any(axis=2) == info["copied"]).all()
    if block:
        assert info["copied"].any(), "the case must reach Wt == 0 on a bad nearest pixel"


def test_timed_call_twice_gives_identical_bits(cuda):
    """kernel_ms requested (HIP events, synchronous): a finite positive time, the same bits both times"""
    W, H, s = 260, 140, 2
    c_lo, f_lo, f_hi = planes(W, H, s)
    p = params(s)
    dc, dl, dh = _dev(c_lo, f_lo, f_hi)
    fl, fh = Features(), Features()
    for k in NAMES:
        setattr(fl, k, dl[k].data_ptr())
        setattr(fh, k, dh[k].data_ptr())
    out = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    res = []
    for _ in range(2):
        ms = ctypes.c_float(-1.0)
        dt.check(dt.lib.dt_upsample(W, H, dc.data_ptr(), ctypes.byref(fl), ctypes.byref(fh), ctypes.byref(p),
                                    out.data_ptr(), 1, None, ctypes.byref(ms)), "dt_upsample")
        assert np.isfinite(ms.value) and ms.value > 0
        res.append(out.cpu().numpy().copy())
    log_equal("upsample timed call twice", res[0].view(np.uint32), res[1].view(np.uint32))
    log_equal("upsample timed call vs numpy", res[0].view(np.uint32),
              upsample_ref_params(W, H, c_lo, f_lo, f_hi, p).view(np.uint32))


def _final(w, h):
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = w, h, 64, 3
    return built, g


@pytest.fixture(scope="module")
def real(cuda):
    """final(240), depth 3, 64 spp: the frame and its guides at 96x54 and at 48x27, computed once"""
    built, g = _final(96, 54)
    out = {}
    for gg in (g, dt.low_res_globals(g, 2)):
        scene = dt.Scene(built, gg)
        img = torch.zeros(3 * gg.xRes * gg.yRes, dtype=torch.float32, device="cuda")
        dt.render(scene, gg, 240, img)
        out[gg.xRes] = (img, dt.render_features(scene, gg, 240, planes=NAMES))
        scene.close()
    return g, out[96], out[48]


def test_real_planes_and_quality_gate(real):
    """The device result on real planes equals the numpy restatement bit for bit, and the reason the
    feature exists: the upsampled 48x27 frame is closer to the 96x54 frame than its pixel replication
    (mean squared error over the 0..255 floats, default parameters). The gate was checked with the CPU
    oracle's render and feature restatement and the host loop before the first device run: 124.29 against
    1195.58."""
    g, (hi, f_hi), (lo, f_lo) = real
    got = dt.upsample(g, lo, f_lo, f_hi).cpu().numpy()
    want = upsample_ref_params(96, 54, lo.cpu().numpy(), _np(f_lo), _np(f_hi), dt.upsample_params_default())
    log_equal("upsample final(240) 48x27 -> 96x54 device vs numpy", got.view(np.uint32), want.view(np.uint32))
    full = hi.cpu().numpy().astype(np.float64)
    rep = replicate(96, 54, 2, lo.cpu().numpy()).astype(np.float64)
    ok = ~(np.isnan(full) | np.isnan(rep) | np.isnan(got))
    mse_up = float(np.mean((got.astype(np.float64)[ok] - full[ok]) ** 2))
    mse_rep = float(np.mean((rep[ok] - full[ok]) ** 2))
    line = "upsample quality final(240) 48x27 -> 96x54, 64 spp: mse upsampled=%.4f replicated=%.4f" % (mse_up, mse_rep)
    print(line)
    _log(line)
    assert mse_up < mse_rep, line


def test_render_image_upsample(real, tmp_path):
    """renderImage(..., upsample=2) writes the composed calls' frame at the full resolution; without
    upsample the file is a plain renderImage's, byte for byte"""
    g, (hi, f_hi), (lo, f_lo) = real
    built, g2 = _final(96, 54)
    up, plain, mine = str(tmp_path / "up.ppm"), str(tmp_path / "plain.ppm"), str(tmp_path / "mine.ppm")
    img, st = dt.renderImage(up, 240, "final", g2, upsample=2)
    assert (g2.xRes, g2.yRes) == (96, 54) and img.size == 3 * 96 * 54
    assert st.pixels == 48 * 27
    want = dt.upsample(g, lo, f_lo, f_hi).cpu().numpy()
    log_equal("renderImage(upsample=2) vs the composed calls", img.view(np.uint32), want.view(np.uint32))
    dt.write_ppm(mine, g, want)
    data = open(up, "rb").read()
    assert data.startswith(b"P6\n96 54\n255\n") and data == open(mine, "rb").read()
    _, g3 = _final(96, 54)
    img_plain, _ = dt.renderImage(plain, 240, "final", g3)
    log_equal("renderImage without upsample vs dt_render", img_plain.view(np.uint32), hi.cpu().numpy().view(np.uint32))
    dt.write_ppm(mine, g, hi.cpu().numpy())
    assert open(plain, "rb").read() == open(mine, "rb").read()
    # denoise=True denoises the low-resolution frame first
    img_dn, _ = dt.renderImage(None, 240, "final", _final(96, 54)[1], upsample=2, denoise=True)
    clean = dt.denoise(dt.low_res_globals(g, 2), lo, f_lo)
    log_equal("renderImage(upsample=2, denoise=True) vs the composed calls", img_dn.view(np.uint32),
              dt.upsample(g, clean, f_lo, f_hi).cpu().numpy().view(np.uint32))
    with pytest.raises(dt.DTError, match="not with progressive"):
        dt.renderImage(None, 240, "final", _final(96, 54)[1], upsample=2, adaptive=1.0)


def test_dtrender_upsample(real, tmp_path):
    """`dtrender final 30 --upsample 2` (frame 240): <stem>.upsampled.ppm at the full resolution, equal to the
    Python path's; the frame's bytes are those of a run without the flag"""
    g, (hi, f_hi), (lo, f_lo) = real
    plain, with_u = str(tmp_path / "plain.ppm"), str(tmp_path / "frame.ppm")
    common = ["final", "30", "--res", "96x54", "--spp", "64", "--depth", "3"]
    subprocess.run([DTRENDER] + common + ["--out", plain], check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run([DTRENDER] + common + ["--out", with_u, "--upsample", "2"], check=True, timeout=120,
                   stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_u, "rb").read()
    data = open(str(tmp_path / "frame.upsampled.ppm"), "rb").read()
    assert data.startswith(b"P6\n96 54\n255\n") and len(data) == len(b"P6\n96 54\n255\n") + 3 * 96 * 54
    mine = str(tmp_path / "mine.ppm")
    dt.write_ppm(mine, g, dt.upsample(g, lo, f_lo, f_hi).cpu().numpy())
    assert data == open(mine, "rb").read()
    bad = subprocess.run([DTRENDER] + common + ["--out", with_u, "--upsample", "5"], timeout=120,
                         stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert bad.returncode == 2 and b"--upsample" in bad.stderr
