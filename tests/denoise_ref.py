"""numpy float32 restatement of the edge-avoiding a-trous filter of include/dt.h (dt_denoise): vectorised
over pixels, a Python loop over the levels and the 25 taps in the stated order, np.fmax for fmaxf. Every
operation is one float32 operation, as in the host loop and the kernels, so the three agree bit for bit.
A helper, not collected by pytest; synthetic_planes() are the seeded planes the tests share."""
import numpy as np

f32 = np.float32
K = (f32(0.375), f32(0.25), f32(0.0625))


def _R(x):
    t = np.fmax(f32(0.0), f32(1.0) - x)
    return t * t


def _dist2(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def denoise_ref(W, H, colour, albedo, normal, depth, levels, demodulate, sigma_normal, sigma_depth, sigma_colour,
                sigma_albedo):
    """out (3*W*H float32) of dt_denoise for whole-frame float32 inputs in image indexing (q = r*W + x)"""
    with np.errstate(all="ignore"):
        C = np.asarray(colour, f32).reshape(H, W, 3)
        A = np.asarray(albedo, f32).reshape(H, W, 3)
        N = np.asarray(normal, f32).reshape(H, W, 3)
        Z = np.asarray(depth, f32).reshape(H, W)
        sn, sz, sc, sa = f32(sigma_normal), f32(sigma_depth), f32(sigma_colour), f32(sigma_albedo)
        isn = f32(1.0) / (sn * sn)
        isa = f32(1.0) / (sa * sa)
        d = np.fmax(A, f32(0.0625)) if demodulate else np.ones_like(A)
        E = C / d
        rz = f32(1.0) / (Z * Z + f32(1e-6))
        for l in range(levels):
            s = 1 << l
            scl, szl = sc * f32(2.0 ** -l), sz * f32(2.0 ** l)
            isc = f32(1.0) / (scl * scl)
            isz = f32(1.0) / (szl * szl)
            S = np.zeros((H, W, 3), f32)
            Wt = np.zeros((H, W), f32)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    # pixels p = (r, x) whose tap q = (r + j*s, x + i*s) lies inside the image
                    r0, r1 = max(0, -j * s), min(H, H - j * s)
                    x0, x1 = max(0, -i * s), min(W, W - i * s)
                    if r0 >= r1 or x0 >= x1:
                        continue
                    P = (slice(r0, r1), slice(x0, x1))
                    Q = (slice(r0 + j * s, r1 + j * s), slice(x0 + i * s, x1 + i * s))
                    h = K[abs(i)] * K[abs(j)]
                    xn = _dist2(N[P], N[Q]) * isn
                    xa = _dist2(A[P], A[Q]) * isa
                    xc = _dist2(E[P], E[Q]) * isc
                    dz = Z[P] - Z[Q]
                    xz = ((dz * dz) * rz[P]) * isz
                    w = (h * (_R(xn) * _R(xz))) * (_R(xa) * _R(xc))
                    take = w > 0
                    S[P] = np.where(take[..., None], S[P] + w[..., None] * E[Q], S[P])
                    Wt[P] = np.where(take, Wt[P] + w, Wt[P])
            ok = Wt > 0
            E = np.where(ok[..., None], S / np.where(ok, Wt, f32(1.0))[..., None], E)
        out = np.fmin(np.fmax(E * d, f32(0.0)), f32(255.0))
        nan = np.isnan(C).any(axis=2)
        out = np.where(nan[..., None], C, out)
    return np.ascontiguousarray(out.reshape(-1), dtype=f32)


def denoise_ref_params(W, H, colour, feats, p):
    """denoise_ref with a DenoiseParams and a dict of planes"""
    return denoise_ref(W, H, colour, feats["albedo"], feats["normal"], feats["depth"], p.levels, p.demodulate,
                       p.sigma_normal, p.sigma_depth, p.sigma_colour, p.sigma_albedo)


def synthetic_planes(W, H, seed=7):
    """Seeded planes with every edge the filter knows: a "sky" region with A = N = Z = 0 (the top rows), a
    normal edge (a vertical line at about W/2), a depth edge (a horizontal line at about 2H/3), an albedo
    checker of 3-pixel squares, noise on the colour, one NaN-colour pixel and one NaN-normal pixel.
    Returns (colour, {"albedo", "normal", "depth"}), float32, image indexing."""
    rng = np.random.default_rng(seed)
    r, x = np.mgrid[0:H, 0:W]
    sky = r < H // 5
    left = x < (W + 1) // 2
    N = np.where(left[..., None], f32([0.0, 1.0, 0.0]), f32([0.6, 0.0, -0.8])).astype(f32)
    N = (N + rng.normal(0, 0.01, (H, W, 3))).astype(f32)
    Z = np.where(r < (2 * H) // 3, 4.0, 9.0) + 0.05 * x + rng.normal(0, 0.01, (H, W))
    check = ((r // 3 + x // 3) % 2).astype(bool)
    A = np.where(check[..., None], f32([0.8, 0.7, 0.2]), f32([0.03, 0.3, 0.6])).astype(f32)
    A = (A + rng.uniform(-0.01, 0.01, (H, W, 3))).astype(f32)
    light = 90.0 + 60.0 * np.sin(x / 5.0) + 40.0 * np.cos(r / 3.0)
    C = A * light[..., None] * 1.6 + rng.normal(0, 6.0, (H, W, 3))
    C = np.clip(C, 0, 255)
    cover = (~sky).astype(f32)
    A, N, Z = A * cover[..., None], N * cover[..., None], Z * cover
    C = np.where(sky[..., None], f32([110.0, 150.0, 230.0]) + rng.normal(0, 3.0, (H, W, 3)), C)
    C, A, N, Z = (np.ascontiguousarray(v, dtype=f32) for v in (C, A, N, Z))
    if W * H > 1:   # one NaN-colour pixel (one channel) and one NaN-normal pixel, away from each other
        C[(H - 1) // 2, (W - 1) // 3, 1] = np.nan
        N[H - 1, W - 1, 0] = np.nan
    return C.reshape(-1), {"albedo": A.reshape(-1), "normal": N.reshape(-1), "depth": Z.reshape(-1)}
