"""Temporal reuse on the device (include/dt.h dt_reproject; dt_temporal.hip): the kernel against the host
loop and the numpy restatement of the specification (tests/temporal_ref.py), bit for bit, on the synthetic
planes and cameras of the host tests; TemporalAccumulator on the planes of a real frame; and the two quality
gates, a standing and a moving camera."""
import ctypes

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
from distraytracer_amd._lib import Features, History

from parity_check import _log, log_equal
from temporal_ref import CAMERAS, bits, cameras, frames, params, reproject_ref

pytestmark = pytest.mark.gpu

INF = float("inf")
GUARD = 256


def _dev(a):
    return None if a is None else ({k: _dev(v) for k, v in a.items()} if isinstance(a, dict) else torch.from_numpy(a).cuda())


def _guarded(n):
    buf = torch.full((n + 2 * GUARD,), -12345.0, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _device_vs_host_vs_numpy(w, h, cam, p, variance, shapes):
    """one case on all three sides; every output of the device call sits in a guard band"""
    cur, prevs = cameras(w, h)
    c, f, pf, hist, v = frames(w, h, variance, shapes)
    want = reproject_ref(cur, c, f, prevs[cam], pf, hist, p, variance=v)
    host = dt.reproject(cur, c, f, prevs[cam], pf, hist, p, variance=v)
    n = w * h
    bufs = {k: _guarded(size) for k, size in (("out", 3 * n), ("out_var", 3 * n), ("colour", 3 * n), ("var", 3 * n), ("len", n))}
    oh = {k: bufs[k][1] for k in (("colour", "var", "len") if variance else ("colour", "len"))}
    got = dt.reproject(cur, _dev(c), _dev(f), prevs[cam], _dev(pf), _dev(hist), p, variance=_dev(v), out=bufs["out"][1],
                       out_history=oh, out_var=bufs["out_var"][1] if variance else None)
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        b = buf.cpu().numpy()
        assert (b[:GUARD] == -12345.0).all() and (b[-GUARD:] == -12345.0).all(), k
        if not variance and k in ("out_var", "var"):
            assert (b == -12345.0).all(), k
    label = "reproject %dx%d %s demodulate %d variance %d shapes %d" % (w, h, cam, p.demodulate, variance, shapes)
    pairs = [("out", got[0], host[0], want[0])] + [("history " + k, got[1][k], host[1][k], want[1][k]) for k in want[1]]
    if variance:
        pairs.append(("out_var", got[2], host[2], want[2]))
    for name, dv, hv, nv in pairs:
        log_equal("%s %s host vs numpy" % (label, name), bits(hv), bits(nv))
        log_equal("%s %s device vs numpy" % (label, name), bits(dv.cpu().numpy()), bits(nv))


@pytest.mark.parametrize("w,h", [(37, 23), (130, 70), (64, 7), (65, 7)])
@pytest.mark.parametrize("cam", CAMERAS)
@pytest.mark.parametrize("demod,variance,shapes", [(1, True, True), (0, False, False)], ids=["demod-var-shapes", "plain"])
def test_device_equals_host_equals_numpy(cuda, w, h, cam, demod, variance, shapes):
    """37x23: one workgroup column, a part of a wave idle; 130x70: three workgroups in x (130 is no multiple of
    64) and eighteen in y, taps crossing them; 64x7 and 65x7: the lane boundary of the (64, 4) block (no idle
    lane; a second block with one live lane) and a second block row with an idle row"""
    _device_vs_host_vs_numpy(w, h, cam, params(demodulate=demod), variance, shapes)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 40)])
@pytest.mark.parametrize("cam", CAMERAS)
def test_device_equals_host_equals_numpy_thin(cuda, w, h, cam):
    _device_vs_host_vs_numpy(w, h, cam, params(), True, True)


@pytest.mark.parametrize("tol", [{"depth_tol": INF}, {"normal_tol": INF}, {"albedo_tol": INF},
                                 {"depth_tol": INF, "normal_tol": INF, "albedo_tol": INF},
                                 {"alpha_min": 0.5, "max_history": 4.0, "depth_tol": 0.0, "normal_tol": 0.0, "albedo_tol": 0.0}],
                         ids=["depth-off", "normal-off", "albedo-off", "all-off", "tight"])
def test_device_equals_host_equals_numpy_tolerances(cuda, tol):
    _device_vs_host_vs_numpy(130, 70, "pan", params(**tol), True, True)
    _device_vs_host_vs_numpy(130, 70, "back", params(**tol), True, True)


def test_first_frame_on_the_device(cuda):
    w, h = 130, 70
    cur, _ = cameras(w, h)
    c, f, _, _, v = frames(w, h)
    out, ho, ov = dt.reproject(cur, _dev(c), _dev(f), None, None, None, params(), variance=_dev(v))
    want = reproject_ref(cur, c, f, None, None, None, params(), variance=v)
    log_equal("reproject first frame out is C", bits(out.cpu().numpy()), bits(c))
    log_equal("reproject first frame out_var is Vc", bits(ov.cpu().numpy()), bits(v))
    for k in want[1]:
        log_equal("reproject first frame history " + k, bits(ho[k].cpu().numpy()), bits(want[1][k]))


def test_timed_call_twice_gives_identical_bits(cuda):
    """kernel_ms requested (HIP events, synchronous), the raw entry point, outputs NaN-filled before the first
    call and left as they are before the second"""
    w, h = 130, 70
    n = w * h
    cur, prevs = cameras(w, h)
    c, f, pf, hist, v = frames(w, h)
    d = {k: _dev(a) for k, a in (("c", c), ("f", f), ("pf", pf), ("h", hist), ("v", v))}
    feat = Features(d["f"]["albedo"].data_ptr(), d["f"]["normal"].data_ptr(), d["f"]["depth"].data_ptr(), None,
                    d["f"]["shape"].data_ptr())
    pfeat = Features(d["pf"]["albedo"].data_ptr(), d["pf"]["normal"].data_ptr(), d["pf"]["depth"].data_ptr(), None, d["pf"]["shape"].data_ptr())
    hin = History(d["h"]["colour"].data_ptr(), d["h"]["var"].data_ptr(), d["h"]["len"].data_ptr())
    o = {k: torch.full((size,), float("nan"), dtype=torch.float32, device="cuda")
         for k, size in (("out", 3 * n), ("out_var", 3 * n), ("colour", 3 * n), ("var", 3 * n), ("len", n))}
    hout = History(o["colour"].data_ptr(), o["var"].data_ptr(), o["len"].data_ptr())
    p = params()
    res = []
    for _ in range(2):
        ms = ctypes.c_float(-1.0)
        dt.check(dt.lib.dt_reproject(ctypes.byref(cur), d["c"].data_ptr(), d["v"].data_ptr(), ctypes.byref(feat),
                                     ctypes.byref(prevs["pan"]), ctypes.byref(pfeat), ctypes.byref(hin), ctypes.byref(p),
                                     o["out"].data_ptr(), o["out_var"].data_ptr(), ctypes.byref(hout), 1, None,
                                     ctypes.byref(ms)), "dt_reproject")
        assert ms.value > 0
        res.append(np.concatenate([o[k].cpu().numpy() for k in ("out", "out_var", "colour", "var", "len")]))
    want = reproject_ref(cur, c, f, prevs["pan"], pf, hist, p, variance=v)
    log_equal("reproject timed call twice", bits(res[0]), bits(res[1]))
    log_equal("reproject timed call vs numpy", bits(res[0]),
                     bits(np.concatenate([want[0], want[2], want[1]["colour"], want[1]["var"], want[1]["len"]])))


# ---- real planes -----------------------------------------------------------------------------------

def _final(w, h, frame=240, depth=3):
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", frame, g)
    g.xRes, g.yRes, g.max_depth = w, h, depth
    return built, g


def _frame(scene, g, frame, spp, seed, features=True):
    """(colour, feats) of one frame at spp samples with the RNG seed `seed`, CUDA tensors"""
    gs = dt.Globals.from_buffer_copy(g)
    gs.antialias_samples, gs.seed = spp, seed
    out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
    dt.render(scene, gs, frame, out)
    return out, (dt.render_features(scene, gs, frame) if features else None)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _rmse(a, b, ok):
    return float(np.sqrt(np.mean((a[ok].astype(np.float64) - b[ok].astype(np.float64)) ** 2)))


def test_accumulator_on_real_planes_and_render_unaffected(cuda):
    """final(240) at 64x36, 64 spp, the same frame pushed twice: the device pushes equal the host loop on the
    same planes bit for bit, and a render of the scene afterwards still gives dt_render's bits"""
    built, g = _final(64, 36)
    scene = dt.Scene(built, g)
    colour, feats = _frame(scene, g, 240, 64, g.seed)
    before = colour.cpu().numpy()
    acc, host = dt.TemporalAccumulator(), dt.TemporalAccumulator()
    hc, hf = before.copy(), _np(feats)
    for k in range(2):
        out = acc.push(g, colour, feats)
        want = host.push(g, hc, hf)
        log_equal("TemporalAccumulator push %d device vs host, final(240) 64x36" % (k + 1),
                         bits(out.cpu().numpy()), bits(want))
        log_equal("TemporalAccumulator push %d history length" % (k + 1),
                         bits(acc.history_length().cpu().numpy()), bits(host.history_length()))
    length = acc.history_length().cpu().numpy()
    assert set(np.unique(length)) <= {0.0, 1.0, 2.0} and np.mean(length == 2) > 0.5
    again, _ = _frame(scene, g, 240, 64, g.seed, features=False)
    log_equal("dt_render after two pushes vs before", bits(again.cpu().numpy()), bits(before))
    scene.close()


def test_static_gate_five_previews_accumulate_towards_the_converged_frame(cuda):
    """final(240) at 160x90, depth 10: a 1024-spp frame with seed s0 is the reference; five 64-spp previews with
    seeds s1..s5 are pushed in turn with the same camera. Gate: RMSE(accumulated) / RMSE(last raw preview) < 1
    over the non-NaN floats. Independent noise would give sqrt((1/5 + 1/16) / (1 + 1/16)) = 0.50; the measured
    ratio and the share of pixels that reached length 5 are in BASELINE.md."""
    built, g = _final(160, 90, depth=10)
    scene = dt.Scene(built, g)
    ref, _ = _frame(scene, g, 240, 1024, 1000, features=False)
    acc = dt.TemporalAccumulator()
    for s in range(1, 6):
        raw, feats = _frame(scene, g, 240, 64, 1000 + s)
        out = acc.push(g, raw, feats)
    scene.close()
    ref, raw, out = ref.cpu().numpy(), raw.cpu().numpy(), out.cpu().numpy()
    length = acc.history_length().cpu().numpy()
    ok = ~(np.isnan(ref) | np.isnan(raw) | np.isnan(out))
    r_raw, r_acc = _rmse(raw, ref, ok), _rmse(out, ref, ok)
    ratio, share5 = r_acc / r_raw, float(np.mean(length == 5))
    line = ("temporal static gate final(240) 160x90 5 x 64 spp vs 1024 spp: rmse raw=%.4f accumulated=%.4f ratio=%.4f "
            "(ideal 0.50) share_len5=%.4f shares by length 0..5=%s"
            % (r_raw, r_acc, ratio, share5, ["%.4f" % float(np.mean(length == k)) for k in range(6)]))
    print(line)
    _log(line)
    assert ratio < 1.0, line


# The last builder frame before 241 that float32 holds with six fraction bits. final(241) itself cannot be
# built: the scene's skeleton comes from the bone table, which holds the postures of the animation's frames
# (builder frames 0, 8, 16, ...) and is asked for posture (int)frame, so 241 is "no posture 241" while
# every frame in [240, 241) takes posture 240. The camera is a continuous function of the builder frame.
FRAME_B = 241 - 1.0 / 64


def test_moving_camera_gate_one_animation_step(cuda):
    """final at builder frames 240 and 241 - 1/64 (FRAME_B above stands in for 241, which has no posture: the
    camera turns by 0.414 degrees instead of 0.421, under a pixel at 160x90 either way), 64 spp each, pushed in
    order; the reference is the second frame at 1024 spp. Condition: at least half of the pixels have history
    length 2. Gate, over those pixels: RMSE(accumulated) / RMSE(raw) < 1. Logged without a gate: the same ratio
    after dt_denoise of both (spatial after temporal against spatial alone).

    Measured on an MI355X: share_len2 = 0.964, RMSE raw 2.2407, accumulated 1.9544, ratio 0.872 (ideal 0.73).
    Without the albedo test (albedo_tol = inf) the ratio is 1.327: histories cross texture and emitter edges
    that depth, normal and shape do not see. BASELINE.md, "Temporal reuse", has the figures."""
    acc = dt.TemporalAccumulator()
    for k, frame in enumerate((240, FRAME_B)):
        built, g = _final(160, 90, frame=frame, depth=10)
        scene = dt.Scene(built, g)
        raw, feats = _frame(scene, g, 240, 64, 2000 + k)
        out = acc.push(g, raw, feats)
        if k == 1:
            ref, _ = _frame(scene, g, 240, 1024, 1000, features=False)
            d_raw, d_out = dt.denoise(g, raw, feats), dt.denoise(g, out, feats)
            torch.cuda.synchronize()
        scene.close()
    ref, raw, out, d_raw, d_out = (a.cpu().numpy() for a in (ref, raw, out, d_raw, d_out))
    length = acc.history_length().cpu().numpy()
    share2 = float(np.mean(length == 2))
    two = np.repeat(length == 2, 3)
    ok = two & ~(np.isnan(ref) | np.isnan(raw) | np.isnan(out) | np.isnan(d_raw) | np.isnan(d_out))
    r_raw, r_acc = _rmse(raw, ref, ok), _rmse(out, ref, ok)
    rd_raw, rd_acc = _rmse(d_raw, ref, ok), _rmse(d_out, ref, ok)
    line = ("temporal moving gate final(240 -> 241 - 1/64) 160x90 64 spp vs 1024 spp: share_len2=%.4f rmse raw=%.4f "
            "accumulated=%.4f ratio=%.4f (ideal 0.73); after dt_denoise: raw=%.4f accumulated=%.4f ratio=%.4f"
            % (share2, r_raw, r_acc, r_acc / r_raw, rd_raw, rd_acc, rd_acc / rd_raw))
    print(line)
    _log(line)
    assert share2 >= 0.5, line
    assert r_acc / r_raw < 1.0, line
