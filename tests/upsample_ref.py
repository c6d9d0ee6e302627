"""numpy float32 restatement of the guided upsampling of include/dt.h (dt_upsample): vectorised over the
full-resolution pixels, a Python loop over the nine taps in the stated order, np.fmax / np.fmin for fmaxf /
fminf. Every operation is one float32 operation, as in the host loop and the kernel, so the three agree
bit for bit. A helper, not collected by pytest."""
import numpy as np

f32 = np.float32


def _R(x):
    t = np.fmax(f32(0.0), f32(1.0) - x)
    return t * t


def _T(t):
    return np.fmax(f32(0.0), f32(1.0) - np.abs(t) * f32(0.5))


def _dist2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def upsample_ref(W, H, s, colour_lo, feats_lo, feats_hi, demodulate, sigma_normal, sigma_depth, sigma_albedo,
                 info=None):
    """out (3*W*H float32) of dt_upsample for float32 inputs in image indexing (slot R*W + X; the low
    resolution is W/s x H/s). info (a dict, optional) gets "fallback": the H x W mask of the pixels with
    Wt == 0, and "copied": those of them whose nearest low-resolution pixel is bad."""
    w, h = W // s, H // s
    assert w * s == W and h * s == H
    with np.errstate(all="ignore"):
        Cl = np.asarray(colour_lo, f32).reshape(h, w, 3)
        Al = np.asarray(feats_lo["albedo"], f32).reshape(h, w, 3)
        Nl = np.asarray(feats_lo["normal"], f32).reshape(h, w, 3)
        Zl = np.asarray(feats_lo["depth"], f32).reshape(h, w)
        A = np.asarray(feats_hi["albedo"], f32).reshape(H, W, 3)
        N = np.asarray(feats_hi["normal"], f32).reshape(H, W, 3)
        Z = np.asarray(feats_hi["depth"], f32).reshape(H, W)
        sn, sz, sa = f32(sigma_normal), f32(sigma_depth), f32(sigma_albedo)
        isn = f32(1.0) / (sn * sn)
        isa = f32(1.0) / (sa * sa)
        isz = f32(1.0) / (sz * sz)
        fs = f32(s)
        dl = np.fmax(Al, f32(0.0625)) if demodulate else np.ones_like(Al)
        El = Cl / dl
        bad = np.isnan(Cl).any(axis=2)
        d = np.fmax(A, f32(0.0625)) if demodulate else np.ones_like(A)
        rz = f32(1.0) / (Z * Z + f32(1e-6))
        Rr, Xx = np.mgrid[0:H, 0:W]
        rc, xc = Rr // s, Xx // s
        fx = (Xx.astype(f32) + f32(0.5)) / fs - f32(0.5)
        fy = (Rr.astype(f32) + f32(0.5)) / fs - f32(0.5)
        S = np.zeros((H, W, 3), f32)
        Wt = np.zeros((H, W), f32)
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                rq, xq = rc + j, xc + i
                inside = (rq >= 0) & (rq < h) & (xq >= 0) & (xq < w)
                rr, xx = np.clip(rq, 0, h - 1), np.clip(xq, 0, w - 1)   # (an address; masked below)
                hsp = _T(fx - xq.astype(f32)) * _T(fy - rq.astype(f32))
                xn = _dist2(N, Nl[rr, xx]) * isn
                xa = _dist2(A, Al[rr, xx]) * isa
                dz = Z - Zl[rr, xx]
                xz = ((dz * dz) * rz) * isz
                wq = (hsp * (_R(xn) * _R(xz))) * _R(xa)
                take = inside & ~bad[rr, xx] & (wq > 0)
                S = np.where(take[..., None], S + wq[..., None] * El[rr, xx], S)
                Wt = np.where(take, Wt + wq, Wt)
        ok = Wt > 0
        E = np.where(ok[..., None], S / np.where(ok, Wt, f32(1.0))[..., None], El[rc, xc])
        out = np.fmin(np.fmax(E * d, f32(0.0)), f32(255.0))
        copied = ~ok & bad[rc, xc]
        out = np.where(copied[..., None], Cl[rc, xc], out)
        if info is not None:
            info["fallback"] = ~ok
            info["copied"] = copied
    return np.ascontiguousarray(out.reshape(-1), dtype=f32)


def upsample_ref_params(W, H, colour_lo, feats_lo, feats_hi, p, info=None):
    """upsample_ref with an UpsampleParams"""
    return upsample_ref(W, H, p.factor, colour_lo, feats_lo, feats_hi, p.demodulate, p.sigma_normal, p.sigma_depth,
                        p.sigma_albedo, info)


def replicate(W, H, s, colour_lo):
    """pixel replication of a W/s x H/s colour image to W x H (what a user without dt_upsample does)"""
    c = np.asarray(colour_lo, f32).reshape(H // s, W // s, 3)
    return np.ascontiguousarray(np.repeat(np.repeat(c, s, axis=0), s, axis=1).reshape(-1))
