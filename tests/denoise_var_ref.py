"""numpy restatements of include/dt.h dt_variance (float64) and dt_denoise_var (float32): vectorised over
pixels, a Python loop over the levels, the nine prefilter terms and the 25 taps in the stated order,
np.fmax / np.fmin for fmaxf / fminf. Every operation is one operation of its format, as in the host loops
and the kernels, so the three agree bit for bit. A helper, not collected by pytest; synthetic_variance()
is the seeded plane that pairs with denoise_ref.synthetic_planes()."""
import numpy as np

from denoise_ref import K, _dist2, _R

f32 = np.float32
G = (f32(0.5), f32(0.25))


def variance_ref(accum, accum2, count):
    """dt_variance: float32 plane for float64 sums (3 per pixel) and integer counts (1 per pixel)"""
    with np.errstate(all="ignore"):
        s1 = np.asarray(accum, np.float64).reshape(-1)
        s2 = np.asarray(accum2, np.float64).reshape(-1)
        n = np.repeat(np.asarray(count).reshape(-1).astype(np.uint32).astype(np.float64), 3)[:s1.size]
        d = s2 - (s1 * s1) / n
        v = np.fmax(d, 0.0) / (n * (n - 1.0))
        out = (v * 65025.0).astype(f32)
        return np.where(n < 2.0, f32(0.0), out).astype(f32)


def _shift(j, i, s, H, W):
    """(P, Q): the pixels p = (r, x) whose neighbour q = (r + j*s, x + i*s) lies inside the image, and those q"""
    r0, r1 = max(0, -j * s), min(H, H - j * s)
    x0, x1 = max(0, -i * s), min(W, W - i * s)
    if r0 >= r1 or x0 >= x1:
        return None
    return (slice(r0, r1), slice(x0, x1)), (slice(r0 + j * s, r1 + j * s), slice(x0 + i * s, x1 + i * s))


def denoise_var_ref(W, H, colour, variance, albedo, normal, depth, levels, demodulate, sigma_normal, sigma_depth,
                    sigma_albedo, sigma_variance, variance_floor):
    """out (3*W*H float32) of dt_denoise_var for whole-frame float32 inputs in image indexing (q = r*W + x)"""
    with np.errstate(all="ignore"):
        C = np.asarray(colour, f32).reshape(H, W, 3)
        Vc = np.asarray(variance, f32).reshape(H, W, 3)
        A = np.asarray(albedo, f32).reshape(H, W, 3)
        N = np.asarray(normal, f32).reshape(H, W, 3)
        Z = np.asarray(depth, f32).reshape(H, W)
        sn, sz, sa, sv, vf = (f32(v) for v in (sigma_normal, sigma_depth, sigma_albedo, sigma_variance, variance_floor))
        isn = f32(1.0) / (sn * sn)
        isa = f32(1.0) / (sa * sa)
        sv2 = sv * sv
        d = np.fmax(A, f32(0.0625)) if demodulate else np.ones_like(A)
        E = C / d
        rz = f32(1.0) / (Z * Z + f32(1e-6))
        x = ((Vc[..., 0] / (d[..., 0] * d[..., 0])) + (Vc[..., 1] / (d[..., 1] * d[..., 1]))) \
            + (Vc[..., 2] / (d[..., 2] * d[..., 2]))
        V = np.fmin(np.fmax(x, f32(0.0)), f32(1e12)).astype(f32)
        for l in range(levels):
            s = 1 << l
            szl = sz * f32(2.0 ** l)
            isz = f32(1.0) / (szl * szl)
            sg = np.zeros((H, W), f32)
            gw = np.zeros((H, W), f32)
            for b in range(-1, 2):
                for a in range(-1, 2):
                    pq = _shift(b, a, 1, H, W)
                    if pq is None:
                        continue
                    P, Q = pq
                    g = G[abs(a)] * G[abs(b)]
                    sg[P] = sg[P] + g * V[Q]
                    gw[P] = gw[P] + g
            vbar = sg / gw
            cv = f32(1.0) / (sv2 * (vbar + vf))
            S = np.zeros((H, W, 3), f32)
            Wt = np.zeros((H, W), f32)
            SV = np.zeros((H, W), f32)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    pq = _shift(j, i, s, H, W)
                    if pq is None:
                        continue
                    P, Q = pq
                    h = K[abs(i)] * K[abs(j)]
                    xn = _dist2(N[P], N[Q]) * isn
                    xa = _dist2(A[P], A[Q]) * isa
                    xc = _dist2(E[P], E[Q]) * cv[P]
                    dz = Z[P] - Z[Q]
                    xz = ((dz * dz) * rz[P]) * isz
                    w = (h * (_R(xn) * _R(xz))) * (_R(xa) * _R(xc))
                    take = w > 0
                    S[P] = np.where(take[..., None], S[P] + w[..., None] * E[Q], S[P])
                    Wt[P] = np.where(take, Wt[P] + w, Wt[P])
                    SV[P] = np.where(take, SV[P] + (w * w) * V[Q], SV[P])
            ok = Wt > 0
            safe = np.where(ok, Wt, f32(1.0))
            E = np.where(ok[..., None], S / safe[..., None], E)
            V = np.where(ok, SV / (safe * safe), V)
        out = np.fmin(np.fmax(E * d, f32(0.0)), f32(255.0))
        nan = np.isnan(C).any(axis=2)
        out = np.where(nan[..., None], C, out)
    return np.ascontiguousarray(out.reshape(-1), dtype=f32)


def denoise_var_ref_params(W, H, colour, variance, feats, p):
    """denoise_var_ref with a DenoiseVarParams and a dict of planes"""
    return denoise_var_ref(W, H, colour, variance, feats["albedo"], feats["normal"], feats["depth"], p.levels,
                           p.demodulate, p.sigma_normal, p.sigma_depth, p.sigma_albedo, p.sigma_variance,
                           p.variance_floor)


def synthetic_variance(W, H, seed=11):
    """A seeded variance plane (3*W*H float32, image indexing) for the planes of synthetic_planes(W, H): a
    low-variance left half (about 1) and a high-variance right half (about 400), an exact-0 block, and one
    NaN, one negative and one element above 1e12, each in a pixel of its own."""
    rng = np.random.default_rng(seed)
    r, x = np.mgrid[0:H, 0:W]
    base = np.where(x < (W + 1) // 2, 1.0, 400.0)[..., None] * rng.uniform(0.5, 1.5, (H, W, 3))
    V = np.ascontiguousarray(base, dtype=f32)
    V[H // 4:H // 4 + max(H // 6, 1), W // 5:W // 5 + max(W // 6, 1)] = 0.0
    if W * H > 3:
        flat = V.reshape(-1, 3)
        n = W * H
        flat[n // 7, 0] = np.nan
        flat[n // 2 + 1, 2] = -3.0
        flat[n - 2, 1] = 4e12
    return V.reshape(-1)
