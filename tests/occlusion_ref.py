"""The prediction of the occlusion feature buffers (include/dt.h dt_render_occlusion, dt_occlusion_ao_ray,
dt_occlusion_light_ray), built from the oracle's exports only.

Primary rays: G.or_primary_ray in dt_intersect_primary's numbering; their hits, points and fixNorm'ed normals:
tests/rayquery_ref.py RayQueryRef.trace. The draws: or_philox4x32 / or_u01 through ctypes. The two generators are
restated here in numpy, f64, one operation at a time (ball, ao_dir, light_dir). Every probe is answered by
RayQueryRef.occluded. The counts are integers; the planes are the two divisions of the header.

OcclusionRef follows every sample once and keeps per-sample, per-probe flags; planes(n, ao_rays) cuts at the
leading n samples and the leading ao_rays probes (probe r of sample i depends on nothing else). A helper, not
collected by pytest."""
import ctypes

import numpy as np

import oracle
from oracle import geom as G
from rayquery_ref import RayQueryRef, void_rays

f32 = np.float32
P_AO, P_OLIGHT = 6, 7
TRIES = 16
POINT, SPHERE, RECT = 1, 2, 3


def words(seed, frame, pixel, sample, purpose, sub):
    """Philox4x32-10, key (seed, (uint32)frame), counter (pixel, sample, 0, (purpose << 24) | sub): (N, 4) uint32.
    pixel, sample (N,); sub a scalar or (N,)"""
    o = oracle.oracle()
    pixel, sample = np.asarray(pixel, np.int64).reshape(-1), np.asarray(sample, np.int64).reshape(-1)
    sub = np.broadcast_to(np.asarray(sub, np.int64), pixel.shape)
    out = np.zeros((len(pixel), 4), np.uint32)
    c, k, w = (ctypes.c_uint32 * 4)(), (ctypes.c_uint32 * 2)(seed & 0xFFFFFFFF, frame & 0xFFFFFFFF), (ctypes.c_uint32 * 4)()
    c[2] = 0
    for i in range(len(pixel)):
        c[0], c[1], c[3] = int(pixel[i]), int(sample[i]), (purpose << 24) | int(sub[i])
        o.or_philox4x32(c, k, w)
        out[i] = w[0], w[1], w[2], w[3]
    return out


def u01(w0, w1):
    o = oracle.oracle()
    return np.array([o.or_u01(int(a), int(b)) for a, b in zip(w0, w1)], np.float64).reshape(len(w0))


def ball(seed, frame, pixel, sample, purpose, base):
    """v(purpose, base) per element: ((N, 3) f64, the accepted try a per element, TRIES where none was)"""
    pixel, sample = np.asarray(pixel, np.int64).reshape(-1), np.asarray(sample, np.int64).reshape(-1)
    base = np.broadcast_to(np.asarray(base, np.int64), pixel.shape)
    v, tries = np.zeros((len(pixel), 3)), np.full(len(pixel), TRIES)
    pending = np.arange(len(pixel))
    for a in range(TRIES):
        if pending.size == 0:
            break
        o = words(seed, frame, pixel[pending], sample[pending], purpose, base[pending] * 16 + a)
        x = o[:, 0].astype(np.float64) * 2.0 ** -31 - 1.0
        y = o[:, 1].astype(np.float64) * 2.0 ** -31 - 1.0
        z = o[:, 2].astype(np.float64) * 2.0 ** -31 - 1.0
        s = (x * x + y * y) + z * z
        ok = s <= 1.0
        v[pending[ok]] = np.stack([x, y, z], axis=1)[ok]
        tries[pending[ok]] = a
        pending = pending[~ok]
    return v, tries


def ao_rule(R, n, v):
    """dir[k] = R * (n[k] + v[k])"""
    return float(f32(R)) * (np.asarray(n, np.float64) + np.asarray(v, np.float64))


def ao_dir(seed, frame, pixel, sample, r, ao_radius, n):
    v, _ = ball(seed, frame, pixel, sample, P_AO, r)
    return ao_rule(ao_radius, np.asarray(n, np.float64).reshape(-1, 3), v)


def light_dir(seed, frame, pixel, sample, j, light, p):
    """light: an object with type, radius, center, A, B, D (a LightDesc); j a scalar or (N,)"""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    C = np.array(list(light.center), np.float64)
    if light.type == RECT:
        o = words(seed, frame, pixel, sample, P_OLIGHT, np.asarray(j, np.int64) * 16)
        u0, u1 = u01(o[:, 0], o[:, 1]), u01(o[:, 2], o[:, 3])
        A, B, D = (np.array(list(v), np.float64) for v in (light.A, light.B, light.D))
        T = (A[None, :] + u0[:, None] * (B - A)[None, :]) + u1[:, None] * (D - A)[None, :]
    elif light.type == SPHERE:
        v, _ = ball(seed, frame, pixel, sample, P_OLIGHT, j)
        T = C[None, :] + float(f32(light.radius)) * v
    else:
        T = np.broadcast_to(C, p.shape)
    return T - p


def first_occluder(rq, start, dir, skip_shape=None):
    """RayQueryRef.occluded's loop, but the answer is the first gathered shape whose or_shape_shadow holds (-1:
    none): which shapes the probes of a prediction are stopped by, for the tests' own assertions"""
    import math
    start, dir = np.asarray(start, np.float64).reshape(-1, 3), np.asarray(dir, np.float64).reshape(-1, 3)
    out = np.full(len(start), -1, np.int32)
    live = np.nonzero(~void_rays(start, dir))[0]
    with np.errstate(all="ignore"):
        inds = rq.gather(dir[live], start[live] + 1e-3 * dir[live])
    for r, gathered in zip(live, inds):
        d, s = dir[r], start[r]
        dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        nn = math.sqrt(dd)
        sn = d / nn if dd > 0 else d
        skip = -1 if skip_shape is None else int(skip_shape[r])
        for si in gathered:
            if si != skip and rq.orc.shadow(si, sn, s + 1e-3 * sn, f32(nn)):
                out[r] = si
                break
    return out


class OcclusionRef:
    CHUNK = 4096   # rays per vectorised gather (rays x nodes temporaries)

    def __init__(self, built, g, frame, n, ao_rays, ao_radius, lights):
        self.rq = RayQueryRef(built, g)
        desc = self.rq.desc
        W, H = g.xRes, g.yRes
        self.W, self.H, self.n, self.ao_rays, self.lights = W, H, n, ao_rays, tuple(lights)
        nb = (n + 7) // 8
        start, ray = G.or_primary_ray(g, frame, 0, nb * W * H * 8)
        i, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing="ij")
        r = (((i // 8) * W * H + y * W + x) * 8 + i % 8).transpose(1, 2, 0).reshape(-1)   # entry [y, x, i]
        start, ray = start.reshape(-1, 3)[r].copy(), ray.reshape(-1, 3)[r].copy()
        pixel = (y * W + x).transpose(1, 2, 0).reshape(-1)
        sample = i.transpose(1, 2, 0).reshape(-1)
        S = len(r)
        shape, pt, nrm = np.full(S, -1, np.int32), np.zeros((S, 3)), np.zeros((S, 3))
        self.prism = 0
        for c0 in range(0, S, self.CHUNK):
            out, seen = self.rq.trace(start[c0:c0 + self.CHUNK], ray[c0:c0 + self.CHUNK])
            shape[c0:c0 + self.CHUNK], pt[c0:c0 + self.CHUNK] = out["shape"], out["point"]
            nrm[c0:c0 + self.CHUNK] = out["normal"]
            self.prism += seen["prism_norm_fallback"]
        self.shape, self.hit = shape, shape >= 0
        at = np.nonzero(self.hit)[0]
        p, nn, px, sm = pt[at], nrm[at], pixel[at], sample[at]
        # per probe: unoccluded and tested (non-void) flags of every sample
        self.unocc = np.zeros((S, ao_rays + len(lights)), bool)
        self.tested = np.zeros((S, ao_rays + len(lights)), bool)
        self.dirs = []
        for k in range(ao_rays + len(lights)):
            if k < ao_rays:
                d, skip = ao_dir(g.seed, frame, px, sm, k, ao_radius, nn), None
            else:
                L = desc.lights[lights[k - ao_rays]]
                d = light_dir(g.seed, frame, px, sm, k - ao_rays, L, p)
                skip = np.full(len(at), L.shape_index, np.int32)
            occ = np.zeros(len(at), np.uint8)
            for c0 in range(0, len(at), self.CHUNK):
                s = slice(c0, c0 + self.CHUNK)
                occ[s] = self.rq.occluded(p[s], d[s], None if skip is None else skip[s])
            self.unocc[at, k] = occ == 0
            self.tested[at, k] = ~void_rays(p, d)
            self.dirs.append(d)
        self.at, self.p = at, p

    def planes(self, n, ao_rays=None):
        """({"ao": [y, x], "light": [y, x, slot], "coverage": [y, x]}, counters) of the leading n samples and the
        leading ao_rays AO probes"""
        A = self.ao_rays if ao_rays is None else ao_rays
        assert n <= self.n and A <= self.ao_rays
        assert n == self.n or self.prism == 0   # the fallback count is kept per call, not per sample
        W, H, K, L = self.W, self.H, self.ao_rays + len(self.lights), len(self.lights)
        un = self.unocc.reshape(H, W, self.n, K)[:, :, :n]
        te = self.tested.reshape(H, W, self.n, K)[:, :, :n]
        hit = self.hit.reshape(H, W, self.n)[:, :, :n]
        use = list(range(A)) + list(range(self.ao_rays, K))
        out = {"coverage": (hit.sum(axis=2).astype(np.float64) / float(n)).astype(f32)}
        if A > 0:
            V = un[:, :, :, :A].sum(axis=(2, 3)).astype(np.int64)
            out["ao"] = (V.astype(np.float64) / (float(n) * float(A))).astype(f32)
        if L > 0:
            Vj = un[:, :, :, self.ao_rays:].sum(axis=2).astype(np.int64)
            out["light"] = (Vj.astype(np.float64) / float(n)).astype(f32)
        cnt = {"shadow_rays": int(te[:, :, :, use].sum()), "prism_norm_fallback": self.prism,
               "hits": int(hit.sum())}
        return out, cnt
