"""Preview denoising on the device (include/dt.h dt_denoise; dt_denoise.hip): the kernels against the host
loop and the numpy restatement of the specification (tests/denoise_ref.py), bit for bit, on synthetic
planes and on the planes of a real preview; the quality gate (the denoised 64-sample preview is closer
to the 1024-sample frame than the raw one); the CLI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
from distraytracer_amd._lib import DenoiseParams, Features

from denoise_ref import denoise_ref_params, synthetic_planes
from parity_check import _log, log_equal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTRENDER = os.path.join(os.path.dirname(HERE), "distraytracer_amd", "dtrender")
INF = float("inf")


def params(levels=5, demodulate=1, sn=0.5, sz=0.1, sc=48.0, sa=0.25):
    return DenoiseParams(levels, demodulate, sn, sz, sc, sa)


def _g(w, h):
    g = dt.globals_default()
    g.xRes, g.yRes = w, h
    return g


def _dev(c, f):
    return torch.from_numpy(c).cuda(), {k: torch.from_numpy(v).cuda() for k, v in f.items()}


def _final(w, h, aa, depth=3):
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = w, h, aa, depth
    return built, g


def _np(feats):
    return {k: v.cpu().numpy() for k, v in feats.items()}


@pytest.fixture(scope="module")
def synthetic():
    """the shared planes: 37x23 (one workgroup column, steps 16 and 32 mostly outside) and 130x70 (three
    workgroups in x, eighteen in y, halos crossing them at every step; 130 is no multiple of 64); the lane
    boundary of the (64, 4) block, widths 63 (one dead lane), 64 (none) and 65 (a second block with one live
    lane, its dead lanes clamped to W-1) with heights 3 (an idle row) and 5 (a second block row); and 1x1 and
    1x40, where the taps have no or one column inside"""
    return {(w, h): synthetic_planes(w, h) for (w, h) in SHAPES}


SHAPES = [(37, 23), (130, 70)] + [(w, h) for w in (63, 64, 65) for h in (3, 5)] + [(1, 1), (1, 40)]


# levels 6: every tap column of step 32 falls outside for part of a 63..65 row, every tap row of step >= 4
# outside a height of 3 or 5; levels 1: the last level is the only one; levels 2: one ping-pong swap before it
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("p", [params(levels=6), params(levels=6, demodulate=0), params(levels=1),
                               params(levels=1, demodulate=0), params(levels=2), params(levels=2, demodulate=0),
                               params(levels=5, sc=INF), params(levels=4, sn=INF, sz=INF, sa=INF)],
                         ids=["l6", "l6-nodemod", "l1", "l1-nodemod", "l2", "l2-nodemod", "l5-colour-off", "l4-guides-off"])
def test_device_equals_host_equals_numpy(cuda, synthetic, w, h, p):
    c, f = synthetic[(w, h)]
    want = denoise_ref_params(w, h, c, f, p)
    host = dt.denoise(_g(w, h), c, f, p)
    dc, df = _dev(c, f)
    # a guard band around out: nothing outside its 3*W*H floats is written
    guard = 256
    buf = torch.full((3 * w * h + 2 * guard,), -12345.0, dtype=torch.float32, device="cuda")
    out = buf[guard:guard + 3 * w * h]
    dt.denoise(_g(w, h), dc, df, p, out=out)
    got = buf.cpu().numpy()
    assert (got[:guard] == -12345.0).all() and (got[-guard:] == -12345.0).all()
    log_equal("denoise %dx%d host vs numpy" % (w, h), host.view(np.uint32), want.view(np.uint32))
    log_equal("denoise %dx%d device vs numpy" % (w, h), got[guard:-guard].view(np.uint32), want.view(np.uint32))


def test_timed_call_twice_gives_identical_bits(cuda, synthetic):
    """kernel_ms requested (HIP events, synchronous); the second call reuses out and work as the first left
    them: no workspace state survives a call"""
    w, h = 130, 70
    c, f = synthetic[(w, h)]
    p = params(levels=6)
    dc, df = _dev(c, f)
    feat = Features()
    for k in ("albedo", "normal", "depth"):
        setattr(feat, k, df[k].data_ptr())
    n_work = dt.lib.dt_denoise_workspace_floats(w, h, ctypes.byref(p))
    work = torch.full((n_work,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.zeros(3 * w * h, dtype=torch.float32, device="cuda")
    res = []
    for _ in range(2):
        ms = ctypes.c_float(-1.0)
        dt.check(dt.lib.dt_denoise(w, h, dc.data_ptr(), ctypes.byref(feat), ctypes.byref(p), out.data_ptr(),
                                   work.data_ptr(), 1, None, ctypes.byref(ms)), "dt_denoise")
        assert ms.value > 0
        res.append(out.cpu().numpy().copy())
    log_equal("denoise timed call twice", res[0].view(np.uint32), res[1].view(np.uint32))
    log_equal("denoise timed call vs numpy", res[0].view(np.uint32), denoise_ref_params(w, h, c, f, p).view(np.uint32))


def test_progressive_denoised_on_real_planes_and_disturbs_nothing(cuda):
    built, g = _final(96, 54, 256)
    scene = dt.Scene(built, g)
    one_shot = torch.zeros(3 * 96 * 54, dtype=torch.float32, device="cuda")
    dt.render(scene, g, 240, one_shot)
    prog = dt.Progressive(scene, g, 240)
    prog.step()
    clean = prog.denoised().cpu().numpy()
    img, feats = prog.image().cpu().numpy(), _np(prog.features())
    want = denoise_ref_params(96, 54, img, feats, dt.denoise_params_default())
    log_equal("Progressive.denoised vs numpy on image() and features()", clean.view(np.uint32), want.view(np.uint32))
    assert np.mean(clean != img) > 0.5, "the default filter left most of the preview as it was"
    prog.run()
    log_equal("image() after denoised() and run() vs dt_render", prog.image().cpu().numpy().view(np.uint32),
              one_shot.cpu().numpy().view(np.uint32))
    scene.close()


def test_quality_gate_denoised_preview_is_closer_to_the_converged_frame(cuda):
    """final(240) at 160x90, 1024 spp: RMSE over the 0..255 floats against the full frame of the raw
    64-sample preview and of the denoised one (default parameters); the gate is ratio < 1. The measured
    value and the choice of the default sigmas: BASELINE.md."""
    built, g = _final(160, 90, 1024, depth=10)
    scene = dt.Scene(built, g)
    prog = dt.Progressive(scene, g, 240)
    prog.step()
    raw = prog.image().cpu().numpy().astype(np.float64)
    clean = prog.denoised().cpu().numpy().astype(np.float64)
    prog.run()
    full = prog.image().cpu().numpy().astype(np.float64)
    scene.close()
    ok = ~(np.isnan(raw) | np.isnan(clean) | np.isnan(full))
    rmse_raw = float(np.sqrt(np.mean((raw[ok] - full[ok]) ** 2)))
    rmse_clean = float(np.sqrt(np.mean((clean[ok] - full[ok]) ** 2)))
    ratio = rmse_clean / rmse_raw
    line = "denoise quality final(240) 160x90 64 of 1024 spp: rmse raw=%.4f denoised=%.4f ratio=%.4f" % (
        rmse_raw, rmse_clean, ratio)
    print(line)
    _log(line)
    assert ratio < 1.0, line


def test_adaptive_progressive_denoised(cuda):
    built, g = _final(96, 54, 256)
    scene = dt.Scene(built, g)
    prog = dt.AdaptiveProgressive(scene, g, 240, tol=2.0)
    prog.step()
    prog.step()
    clean = prog.denoised().cpu().numpy()
    img, feats = prog.image().cpu().numpy(), _np(prog.features())
    want = denoise_ref_params(96, 54, img, feats, dt.denoise_params_default())
    log_equal("AdaptiveProgressive.denoised vs numpy", clean.view(np.uint32), want.view(np.uint32))
    scene.close()


def test_tile_share_is_refused(cuda):
    built, g = _final(96, 54, 64)
    scene = dt.Scene(built, g)
    prog = dt.Progressive(scene, g, 240, tile=dt.tiles(rank=0, world=2))
    prog.step()
    with pytest.raises(dt.DTError, match="whole frame"):
        prog.denoised()
    scene.close()


@pytest.mark.parametrize("ext", ["ppm", "png"])
def test_dtrender_denoise(cuda, tmp_path, ext):
    """`dtrender spheres --denoise`: the frame's bytes are those of a run without the flag, and
    <stem>.denoised.<ext> is the Python path's result through the same writer"""
    plain, with_d = str(tmp_path / ("plain." + ext)), str(tmp_path / ("frame." + ext))
    subprocess.run([DTRENDER, "spheres", "--out", plain], check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run([DTRENDER, "spheres", "--out", with_d, "--denoise"], check=True, timeout=120,
                   stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_d, "rb").read()
    assert dt.denoised_filename(with_d) == str(tmp_path / ("frame.denoised." + ext))
    # the CLI's globals for `spheres`
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("spheres", 0, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = 256, 256, 1, 1
    scene = dt.Scene(built, g)
    img = torch.zeros(3 * 256 * 256, dtype=torch.float32, device="cuda")
    dt.render(scene, g, 0, img)
    feats = dt.render_features(scene, g, 0, planes=("albedo", "normal", "depth"))
    clean = dt.denoise(g, img, feats)
    scene.close()
    mine = str(tmp_path / ("mine." + ext))
    (dt.write_png if ext == "png" else dt.write_ppm)(mine, g, clean.cpu().numpy())
    assert open(mine, "rb").read() == open(dt.denoised_filename(with_d), "rb").read()
    # --denoise-levels reaches the filter: one level gives another file
    subprocess.run([DTRENDER, "spheres", "--out", with_d, "--denoise", "--denoise-levels", "1"], check=True,
                   timeout=120, stdout=subprocess.DEVNULL)
    p1 = dt.denoise_params_default()
    p1.levels = 1
    clean1 = dt.denoise(g, img, feats, p1)
    (dt.write_png if ext == "png" else dt.write_ppm)(mine, g, clean1.cpu().numpy())
    assert open(mine, "rb").read() == open(dt.denoised_filename(with_d), "rb").read()
