"""Variance-guided preview denoising on the device (include/dt.h dt_variance, dt_denoise_var;
dt_denoise_var.hip): the kernels against the host loops and the numpy restatements of the specification
(tests/denoise_var_ref.py), bit for bit, on synthetic planes and on the sums of a real adaptive frame; the
variance plane of slab shares; the quality gate; the CLI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
from distraytracer_amd._lib import DenoiseVarParams, Features

from denoise_ref import synthetic_planes
from denoise_var_ref import denoise_var_ref_params, synthetic_variance, variance_ref
from parity_check import _log, log_equal

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTRENDER = os.path.join(os.path.dirname(HERE), "distraytracer_amd", "dtrender")
INF = float("inf")


def params(levels=5, demodulate=1, sn=0.5, sz=0.1, sa=0.25, sv=3.0, vf=2.0):
    return DenoiseVarParams(levels, demodulate, sn, sz, sa, sv, vf, 0.0)


def _g(w, h):
    g = dt.globals_default()
    g.xRes, g.yRes = w, h
    return g


def _dev(c, v, f):
    return torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda(), {k: torch.from_numpy(a).cuda() for k, a in f.items()}


def _final(w, h, aa, depth=3):
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = w, h, aa, depth
    return built, g


def _np(feats):
    return {k: v.cpu().numpy() for k, v in feats.items()}


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def synthetic():
    """the shared planes: 37x23 (one workgroup column, steps 16 and 32 mostly outside), 130x70 (three
    workgroups in x, eighteen in y, halos crossing them at every step; 130 is no multiple of 64); the lane
    boundary of the (64, 4) block, widths 63 (one dead lane), 64 (none) and 65 (a second block with one live
    lane, its dead lanes clamped to W-1) with heights 3 (an idle row) and 5 (a second block row); and 1x1 and
    1x40, where the prefilter and the taps have no or one column inside"""
    return {(w, h): synthetic_planes(w, h) + (synthetic_variance(w, h),) for (w, h) in SHAPES + [(1, 1), (1, 40)]}


SHAPES = [(37, 23), (130, 70)] + [(w, h) for w in (63, 64, 65) for h in (3, 5)]


def _device_vs_host_vs_numpy(synthetic, w, h, p):
    c, f, v = synthetic[(w, h)]
    want = denoise_var_ref_params(w, h, c, v, f, p)
    host = dt.denoise(_g(w, h), c, f, p, variance=v)
    dc, dv, df = _dev(c, v, f)
    # a guard band around out: nothing outside its 3*W*H floats is written
    guard = 256
    buf = torch.full((3 * w * h + 2 * guard,), -12345.0, dtype=torch.float32, device="cuda")
    out = buf[guard:guard + 3 * w * h]
    dt.denoise(_g(w, h), dc, df, p, out=out, variance=dv)
    got = buf.cpu().numpy()
    assert (got[:guard] == -12345.0).all() and (got[-guard:] == -12345.0).all()
    log_equal("denoise_var %dx%d host vs numpy" % (w, h), u32(host), u32(want))
    log_equal("denoise_var %dx%d device vs numpy" % (w, h), u32(got[guard:-guard]), u32(want))


# levels 6: every tap column of step 32 falls outside for part of a 63..65 row, every tap row of step >= 4
# outside a height of 3 or 5; levels 1: the last level is the only one; levels 2: one ping-pong swap before it
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("p", [params(levels=6), params(levels=6, demodulate=0), params(levels=1),
                               params(levels=1, demodulate=0), params(levels=2), params(levels=2, demodulate=0),
                               params(levels=5, sv=INF), params(levels=4, sn=INF, sz=INF, sa=INF)],
                         ids=["l6", "l6-nodemod", "l1", "l1-nodemod", "l2", "l2-nodemod", "l5-variance-off", "l4-guides-off"])
def test_device_equals_host_equals_numpy(cuda, synthetic, w, h, p):
    _device_vs_host_vs_numpy(synthetic, w, h, p)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 40)])
def test_device_equals_host_equals_numpy_thin(cuda, synthetic, w, h):
    _device_vs_host_vs_numpy(synthetic, w, h, params(levels=6))


def test_timed_call_twice_gives_identical_bits(cuda, synthetic):
    """kernel_ms requested (HIP events, synchronous) on a NaN-filled workspace; the second call reuses out and
    work as the first left them: no workspace state survives a call"""
    w, h = 130, 70
    c, f, v = synthetic[(w, h)]
    p = params(levels=6)
    dc, dv, df = _dev(c, v, f)
    feat = Features()
    for k in ("albedo", "normal", "depth"):
        setattr(feat, k, df[k].data_ptr())
    n_work = dt.lib.dt_denoise_var_workspace_floats(w, h, ctypes.byref(p))
    work = torch.full((n_work,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.zeros(3 * w * h, dtype=torch.float32, device="cuda")
    res = []
    for _ in range(2):
        ms = ctypes.c_float(-1.0)
        dt.check(dt.lib.dt_denoise_var(w, h, dc.data_ptr(), dv.data_ptr(), ctypes.byref(feat), ctypes.byref(p),
                                       out.data_ptr(), work.data_ptr(), 1, None, ctypes.byref(ms)), "dt_denoise_var")
        assert ms.value > 0
        res.append(out.cpu().numpy().copy())
    log_equal("denoise_var timed call twice", u32(res[0]), u32(res[1]))
    log_equal("denoise_var timed call vs numpy", u32(res[0]), u32(denoise_var_ref_params(w, h, c, v, f, p)))


@pytest.fixture(scope="module")
def adaptive_frame(cuda):
    """final(240) at 96x54, 256 spp, tol 2.0 after two windows: some pixels stopped at 64 samples, the rest
    have 128, so the counts differ"""
    built, g = _final(96, 54, 256)
    scene = dt.Scene(built, g)
    prog = dt.AdaptiveProgressive(scene, g, 240, tol=2.0)
    prog.step()
    prog.step()
    yield built, g, scene, prog
    scene.close()


def test_variance_device_equals_host_on_real_sums(adaptive_frame):
    built, g, scene, prog = adaptive_frame
    cnt = prog.count.cpu().numpy()
    assert 0 < int((cnt == 64).sum()) < cnt.size, "the tolerance stopped no pixel, or every pixel"
    dev = prog.variance().cpu().numpy()
    s1, s2 = prog.accum.cpu().numpy(), prog.accum2.cpu().numpy()
    host = dt.variance(g, s1, s2, cnt)
    log_equal("dt_variance device vs host", u32(dev), u32(host))
    log_equal("dt_variance host vs numpy", u32(host), u32(variance_ref(s1, s2, cnt)))
    assert np.isfinite(dev).all() and (dev >= 0).all() and (dev > 0).any()


def test_variance_of_three_slab_shares_unpacks_to_the_whole_frame(adaptive_frame):
    """the frame as three ranks in DT_OUT_SLAB, rendered one after another: a pixel's samples, and so its
    sums and its stopping, do not depend on the split; dt_unpack_slabs gathers variance planes as colours"""
    built, g, scene, prog = adaptive_frame
    whole = prog.variance().cpu().numpy()
    base = dt.tiles(rank=0, world=3, layout=dt.DT_OUT_SLAB)
    per = dt.slab_floats_max(g, base)
    slabs = torch.zeros(3 * per, dtype=torch.float32, device="cuda")
    for r in range(3):
        t = dt.tiles(rank=r, world=3, layout=dt.DT_OUT_SLAB)
        share = dt.AdaptiveProgressive(scene, g, 240, tol=2.0, tile=t)
        share.step()
        share.step()
        n = dt.accum_doubles(g, t)
        assert 0 < n <= per
        share.variance(out=slabs[r * per:r * per + share.accum.numel()])
    image = torch.full((3 * g.xRes * g.yRes,), -1.0, dtype=torch.float32, device="cuda")
    dt.unpack_slabs(g, base, 3, slabs, image)
    torch.cuda.synchronize()
    log_equal("three ranks' variance slabs unpacked vs the whole frame's plane", u32(image.cpu().numpy()), u32(whole))


def test_adaptive_progressive_denoised_by_variance(adaptive_frame):
    built, g, scene, prog = adaptive_frame
    clean = prog.denoised(variance=True).cpu().numpy()
    img, var, feats = prog.image().cpu().numpy(), prog.variance().cpu().numpy(), _np(prog.features())
    want = denoise_var_ref_params(96, 54, img, var, feats, dt.denoise_var_params_default())
    log_equal("AdaptiveProgressive.denoised(variance=True) vs numpy", u32(clean), u32(want))
    assert np.mean(clean != img) > 0.5, "the default filter left most of the preview as it was"
    plain = prog.denoised().cpu().numpy()
    assert np.mean(clean != plain) > 0.25, "the variance-guided result is dt_denoise's"
    p3 = dt.denoise_var_params_default()
    p3.levels = 3
    log_equal("denoised(params, variance=True) vs numpy", u32(prog.denoised(p3, variance=True).cpu().numpy()),
              u32(denoise_var_ref_params(96, 54, img, var, feats, p3)))


def test_min_samples_spp_never_stops_and_ends_on_dt_render(cuda):
    """with min_samples = spp no pixel stops: the denoised preview disturbs nothing and run() ends on
    dt_render's bits; Progressive has no sums of squares and refuses variance=True"""
    built, g = _final(96, 54, 256)
    scene = dt.Scene(built, g)
    one_shot = torch.zeros(3 * 96 * 54, dtype=torch.float32, device="cuda")
    dt.render(scene, g, 240, one_shot)
    prog = dt.AdaptiveProgressive(scene, g, 240, tol=2.0, min_samples=256)
    prog.step()
    clean = prog.denoised(variance=True).cpu().numpy()
    assert np.isfinite(clean).all()
    prog.run()
    assert int(prog.count.min().item()) == 256
    log_equal("image() after denoised(variance=True) and run() vs dt_render", u32(prog.image().cpu().numpy()),
              u32(one_shot.cpu().numpy()))
    plain = dt.Progressive(scene, g, 240)
    plain.step()
    with pytest.raises(dt.DTError, match="AdaptiveProgressive.*min_samples >= spp"):
        plain.denoised(variance=True)
    scene.close()


def test_render_image_by_variance_needs_adaptive(cuda, tmp_path):
    with pytest.raises(dt.DTError, match="needs adaptive"):
        dt.renderImage(str(tmp_path / "a.ppm"), 0, "spheres", denoise="variance")
    with pytest.raises(dt.DTError, match="needs adaptive"):
        dt.renderImage(str(tmp_path / "a.ppm"), 0, "spheres", denoise=dt.denoise_var_params_default())


def test_quality_gate_variance_guided_preview_is_closer_to_the_converged_frame(cuda):
    """final(240) at 160x90, 1024 spp, depth 10, the frame of test_gpu_denoise.py's gate: AdaptiveProgressive
    with tol 0 and min_samples 1024 never stops a pixel, so its 64-sample preview is that gate's preview.
    RMSE over the 0..255 floats against the full frame of the raw preview, of dt_denoise with defaults and
    of dt_denoise_var with defaults; the gate is ratio_var < 1. The measured values and the choice of the
    defaults: BASELINE.md."""
    built, g = _final(160, 90, 1024, depth=10)
    scene = dt.Scene(built, g)
    prog = dt.AdaptiveProgressive(scene, g, 240, tol=0.0, min_samples=1024)
    prog.step()
    raw = prog.image().cpu().numpy().astype(np.float64)
    plain = prog.denoised().cpu().numpy().astype(np.float64)
    guided = prog.denoised(variance=True).cpu().numpy().astype(np.float64)
    prog.run()
    assert int(prog.count.min().item()) == 1024
    full = prog.image().cpu().numpy().astype(np.float64)
    scene.close()
    ok = ~(np.isnan(raw) | np.isnan(plain) | np.isnan(guided) | np.isnan(full))
    rmse = [float(np.sqrt(np.mean((v[ok] - full[ok]) ** 2))) for v in (raw, plain, guided)]
    ratio_plain, ratio_var = rmse[1] / rmse[0], rmse[2] / rmse[0]
    line = ("denoise_var quality final(240) 160x90 64 of 1024 spp: rmse raw=%.4f dt_denoise=%.4f dt_denoise_var=%.4f "
            "ratio_plain=%.4f ratio_var=%.4f" % (rmse[0], rmse[1], rmse[2], ratio_plain, ratio_var))
    print(line)
    _log(line)
    assert ratio_var < 1.0, line


@pytest.mark.parametrize("ext", ["ppm", "png"])
def test_dtrender_denoise_variance(cuda, tmp_path, ext):
    """`dtrender spheres --adaptive 0.5 --denoise-variance`: the frame's bytes are those of a run without the
    flag, <stem>.denoised.<ext> is the Python path's result through the same writer, and without --adaptive
    the flag is a usage error"""
    plain, with_d = str(tmp_path / ("plain." + ext)), str(tmp_path / ("frame." + ext))
    subprocess.run([DTRENDER, "spheres", "--out", plain, "--adaptive", "0.5"], check=True, timeout=120,
                   stdout=subprocess.DEVNULL)
    subprocess.run([DTRENDER, "spheres", "--out", with_d, "--adaptive", "0.5", "--denoise-variance"], check=True,
                   timeout=120, stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_d, "rb").read()
    # the CLI's globals for `spheres`
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("spheres", 0, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = 256, 256, 1, 1
    scene = dt.Scene(built, g)
    prog = dt.AdaptiveProgressive(scene, g, 0, tol=0.5)
    prog.run()
    mine = str(tmp_path / ("mine." + ext))
    write = dt.write_png if ext == "png" else dt.write_ppm
    write(mine, g, prog.denoised(variance=True).cpu().numpy())
    assert open(mine, "rb").read() == open(dt.denoised_filename(with_d), "rb").read()
    # --denoise-levels reaches the filter: one level gives another file
    subprocess.run([DTRENDER, "spheres", "--out", with_d, "--adaptive", "0.5", "--denoise-variance",
                    "--denoise-levels", "1"], check=True, timeout=120, stdout=subprocess.DEVNULL)
    p1 = dt.denoise_var_params_default()
    p1.levels = 1
    write(mine, g, prog.denoised(p1, variance=True).cpu().numpy())
    assert open(mine, "rb").read() == open(dt.denoised_filename(with_d), "rb").read()
    scene.close()
    # without --adaptive: a usage error before any rendering, no file
    none = str(tmp_path / ("none." + ext))
    r = subprocess.run([DTRENDER, "spheres", "--out", none, "--denoise-variance"], timeout=120,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"--adaptive" in r.stderr
    assert not os.path.exists(none) and not os.path.exists(dt.denoised_filename(none))
