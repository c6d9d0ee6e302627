"""numpy float32 restatement of include/dt.h dt_reproject: vectorised over pixels, a Python loop over the
four taps in the stated order, np.fmax / np.fmin for fmaxf / fminf, np.sqrt and / for the correctly rounded
sqrtf and division, np.floor for floorf. Every operation is one float32 operation, as in the host loop and
the kernel, so the three agree bit for bit. A helper, not collected by pytest; previous_frame() builds the
seeded previous frame and history that pair with denoise_ref.synthetic_planes() as the current frame, and
cameras() / frames() are the cases the host and the GPU tests share."""
import math

import numpy as np

import distraytracer_amd as dt
from distraytracer_amd._lib import TemporalParams

from denoise_ref import synthetic_planes
from denoise_var_ref import synthetic_variance

f32 = np.float32


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cam(c):
    """the record's vectors in float32, converted once"""
    return {k: np.array(list(getattr(c, k)), np.float64).astype(f32) for k in ("eye", "X", "Y", "Z")}


def reproject_ref(cur, colour, feats, prev, prev_feats, hist, p, variance=None):
    """(out, {"colour", "len"[, "var"]}, out_var or None) of dt_reproject for whole-frame float32 inputs in image
    indexing; cur / prev: Camera records, p: a TemporalParams; prev, prev_feats, hist all None: no history"""
    W, H = int(cur.xRes), int(cur.yRes)
    with np.errstate(all="ignore"):
        C = np.asarray(colour, f32).reshape(H, W, 3)
        A = np.asarray(feats["albedo"], f32).reshape(H, W, 3)
        N = np.asarray(feats["normal"], f32).reshape(H, W, 3)
        Z = np.asarray(feats["depth"], f32).reshape(H, W)
        has_var = variance is not None
        Vc = np.asarray(variance, f32).reshape(H, W, 3) if has_var else np.zeros((H, W, 3), f32)
        d = np.fmax(A, f32(0.0625)) if p.demodulate else np.ones_like(A)
        E = C / d
        Ve = Vc / (d * d)
        nan = np.isnan(C).any(axis=2)
        S = np.zeros((H, W, 3), f32)
        SV = np.zeros((H, W, 3), f32)
        SL = np.zeros((H, W), f32)
        Wt = np.zeros((H, W), f32)
        if prev is not None:
            cc, pc = _cam(cur), _cam(prev)
            r, x = np.mgrid[0:H, 0:W]
            y = H - 1 - r
            fW, fH = f32(W), f32(H)
            fa = f32(cur.l) + ((f32(cur.r) - f32(cur.l)) * x.astype(f32)) / fW
            fb = f32(cur.b) + ((f32(cur.t) - f32(cur.b)) * y.astype(f32)) / fH
            dirv = (fa[..., None] * cc["X"] + fb[..., None] * cc["Y"]) - f32(cur.near_plane) * cc["Z"]
            surf = Z > 0
            sc = Z / np.sqrt(_dot(dirv, dirv))
            pw = cc["eye"] + sc[..., None] * dirv
            v = np.where(surf[..., None], pw - pc["eye"], dirv)
            dq = np.sqrt(_dot(v, v))
            zc = -_dot(v, pc["Z"])
            pa = (f32(prev.near_plane) * _dot(v, pc["X"])) / zc
            pb = (f32(prev.near_plane) * _dot(v, pc["Y"])) / zc
            fx = ((pa - f32(prev.l)) * fW) / (f32(prev.r) - f32(prev.l))
            fy = ((pb - f32(prev.b)) * fH) / (f32(prev.t) - f32(prev.b))
            sought = (zc > 0) & (f32(-1) < fx) & (fx < fW) & (f32(-1) < fy) & (fy < fH)
            fxs, fys = np.where(sought, fx, f32(0)), np.where(sought, fy, f32(0))
            x0, y0 = np.floor(fxs), np.floor(fys)
            tx, ty = fxs - x0, fys - y0
            ix, iy = x0.astype(np.int64), y0.astype(np.int64)
            wx, wy = (f32(1) - tx, tx), (f32(1) - ty, ty)
            dtol = f32(p.depth_tol) * dq
            nt2 = f32(p.normal_tol) * f32(p.normal_tol)
            pN = np.asarray(prev_feats["normal"], f32).reshape(H, W, 3)
            pZ = np.asarray(prev_feats["depth"], f32).reshape(H, W)
            pA = np.asarray(prev_feats["albedo"], f32).reshape(H, W, 3)
            at2 = f32(p.albedo_tol) * f32(p.albedo_tol)
            hc = np.asarray(hist["colour"], f32).reshape(H, W, 3)
            hl = np.asarray(hist["len"], f32).reshape(H, W)
            hv = np.asarray(hist["var"], f32).reshape(H, W, 3) if has_var else None
            shapes = feats.get("shape") is not None and prev_feats.get("shape") is not None
            for j in (0, 1):
                for i in (0, 1):
                    w = wx[i] * wy[j]
                    u, t = ix + i, iy + j
                    inside = (u >= 0) & (u < W) & (t >= 0) & (t < H)
                    rt, ut = H - 1 - np.clip(t, 0, H - 1), np.clip(u, 0, W - 1)
                    h_l, h_c, zt = hl[rt, ut], hc[rt, ut], pZ[rt, ut]
                    dn = N - pN[rt, ut]
                    da = A - pA[rt, ut]
                    depth_ok = np.where(surf, np.abs(zt - dq) <= dtol, zt == 0)
                    valid = sought & inside & (w > 0) & (h_l > 0) & ~np.isnan(h_c).any(axis=2) & depth_ok \
                        & (_dot(dn, dn) <= nt2) & (_dot(da, da) <= at2)
                    if shapes:
                        valid &= np.asarray(feats["shape"]).reshape(H, W) == np.asarray(prev_feats["shape"]).reshape(H, W)[rt, ut]
                    Wt = np.where(valid, Wt + w, Wt)
                    S = np.where(valid[..., None], S + w[..., None] * h_c, S)
                    SL = np.where(valid, SL + w * h_l, SL)
                    if has_var:
                        SV = np.where(valid[..., None], SV + w[..., None] * hv[rt, ut], SV)
        blend = (Wt > 0) & ~nan
        n = np.fmin(SL / Wt + f32(1), f32(p.max_history))
        alpha = np.fmax(f32(p.alpha_min), f32(1) / n)
        om = f32(1) - alpha
        e_h = S / Wt[..., None]
        e_o = e_h + alpha[..., None] * (E - e_h)
        b3 = blend[..., None]
        oc = np.where(b3, e_o, E)
        out = np.where(b3, np.fmin(np.fmax(e_o * d, f32(0)), f32(255)), C)
        v_o = (om * om)[..., None] * (SV / Wt[..., None]) + (alpha * alpha)[..., None] * Ve
        ov = np.where(b3, v_o, Ve)
        out_var = np.where(b3, v_o * (d * d), Vc)
        ol = np.where(blend, n, np.where(nan, f32(0), f32(1)))
    flat = lambda a: np.ascontiguousarray(a.reshape(-1), dtype=f32)
    hist_out = {"colour": flat(oc), "len": flat(ol)}
    if has_var:
        hist_out["var"] = flat(ov)
    return flat(out), hist_out, flat(out_var) if has_var else None


def previous_frame(W, H, seed=23):
    """A seeded previous frame for synthetic_planes(W, H): its guides are the current frame's with a little
    noise (so that the depth, normal and albedo tests decide near their tolerances), its shape ids a checker of 5-pixel
    squares, its history lengths 0, 1, 7 and 32 mixed, and one NaN in the history colour. Returns
    (prev_feats, history, shape): dicts of float32 planes (shape int32), and the current frame's shape plane,
    which differs from the previous frame's in a block."""
    rng = np.random.default_rng(seed)
    c, f = synthetic_planes(W, H)
    n = W * H
    pN = (f["normal"] + rng.normal(0, 0.05, 3 * n)).astype(f32)
    pZ = (f["depth"] * (1 + rng.normal(0, 0.01, n))).astype(f32)
    pA = (f["albedo"] + rng.normal(0, 0.03, 3 * n)).astype(f32)   # |dA| about 0.05: the 0.0625 test decides
    r, x = np.mgrid[0:H, 0:W]
    pshape = ((r // 5) * 7 + x // 5).astype(np.int32).reshape(-1)
    shape = pshape.copy()
    shape.reshape(H, W)[H // 3:H // 3 + 3, W // 4:W // 4 + 4] = -1
    hc = (c / np.fmax(f["albedo"], f32(0.0625)) + rng.normal(0, 8.0, 3 * n)).astype(f32)
    hc[np.isnan(hc)] = 77.0
    if n > 3:
        hc[3 * (n // 3) + 2] = np.nan
    hl = rng.choice(f32([0, 1, 7, 32]), n).astype(f32)
    hv = rng.uniform(0.5, 300.0, 3 * n).astype(f32)
    return ({"albedo": pA, "normal": pN, "depth": pZ, "shape": pshape}, {"colour": hc, "len": hl, "var": hv}, shape)


# ---- the shared cases ------------------------------------------------------------------------------

def params(demodulate=1, alpha_min=0.05, max_history=32.0, depth_tol=0.02, normal_tol=0.25, albedo_tol=0.0625):
    return TemporalParams(demodulate, alpha_min, max_history, depth_tol, normal_tol, albedo_tol)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, "%s: %d of %d floats differ, first at %d: %r vs %r" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def _g(w, h):
    g = dt.globals_default()
    g.xRes, g.yRes = w, h
    return g


def _gaze(g):
    v = np.array(list(g.lookingAt)) - np.array(list(g.eye))
    return v / np.linalg.norm(v)


def _turned(g, degrees):
    """g with its gaze turned about the up vector"""
    up = np.array(list(g.up), float)
    up /= np.linalg.norm(up)
    v = np.array(list(g.lookingAt)) - np.array(list(g.eye))
    a = math.radians(degrees)
    w = v * math.cos(a) + np.cross(up, v) * math.sin(a) + up * np.dot(up, v) * (1 - math.cos(a))
    o = _g(g.xRes, g.yRes)
    for k in range(3):
        o.lookingAt[k] = g.eye[k] + w[k]
    return o


def cameras(w, h):
    """(current, {name: previous}): identical; a sub-pixel pan (0.37 of a pixel's angle: fractional fx, all
    four taps live); a 30 degree turn (the taps of the frame's left part fall outside); the previous eye 0.1
    further back along the gaze     (the synthetic depths are 4..16, so the relative depth difference is 0.6 .. 2.5 %: the 2 % test decides);
    a previous camera facing away (zc <= 0 everywhere)"""
    g = _g(w, h)
    cur = dt.camera(g)
    pixel = math.degrees(math.atan((cur.r - cur.l) / w / cur.near_plane))
    back = _g(w, h)
    away = _g(w, h)
    for k in range(3):
        back.eye[k] = g.eye[k] - 0.1 * _gaze(g)[k]
        away.lookingAt[k] = g.eye[k] - (g.lookingAt[k] - g.eye[k])
    return cur, {"identical": dt.camera(g), "pan": dt.camera(_turned(g, 0.37 * pixel)), "turn30": dt.camera(_turned(g, 30.0)),
                 "back": dt.camera(back), "away": dt.camera(away)}


CAMERAS = ("identical", "pan", "turn30", "back", "away")


def frames(w, h, variance=True, shapes=True):
    """the current frame (synthetic_planes, synthetic_variance) and the previous frame (a second seed)"""
    c, f = synthetic_planes(w, h)
    pf, hist, shape = previous_frame(w, h)
    f, pf, hist = dict(f), dict(pf), dict(hist)
    if shapes:
        f["shape"] = shape
    else:
        del pf["shape"]
    if not variance:
        del hist["var"]
    return c, f, pf, hist, (synthetic_variance(w, h) if variance else None)


def assert_result_bits(got, want, what):
    assert_same_bits(got[0], want[0], what + ": out")
    for k in want[1]:
        assert_same_bits(got[1][k], want[1][k], what + ": history " + k)
    assert set(got[1]) == set(want[1])
    assert (got[2] is None) == (want[2] is None)
    if want[2] is not None:
        assert_same_bits(got[2], want[2], what + ": out_var")
