"""The prediction of the occlusion queries at surface points (include/dt.h dt_points_occlusion), built from the
oracle's exports only: the probe directions are tests/occlusion_ref.py's ao_dir and light_dir with pixel = the
point's index i and sample = s, and every probe is answered by tests/rayquery_ref.py RayQueryRef.occluded.

PointsOcclusionRef follows every (point, sample, probe) once and keeps per-probe flags, so planes(n_points,
n_samples, ao_rays) is a prefix cut in each of the three: probe r of sample s of point i depends on nothing else.
A void point (a non-finite component in its point or normal) is never probed. A helper, not collected by
pytest."""
import numpy as np

from occlusion_ref import ao_dir, light_dir
from rayquery_ref import RayQueryRef, void_rays

f32 = np.float32


class PointsOcclusionRef:
    def __init__(self, built, g, frame, points, normals, n_samples, ao_rays, ao_radius, lights, rq=None):
        self.rq = rq if rq is not None else RayQueryRef(built, g)
        desc = self.rq.desc
        p = np.asarray(points, np.float64).reshape(-1, 3)
        nrm = np.asarray(normals, np.float64).reshape(-1, 3)
        N, K = len(p), ao_rays + len(lights)
        self.N, self.n, self.ao_rays, self.lights = N, n_samples, ao_rays, tuple(lights)
        self.live = np.isfinite(p).all(axis=1) & np.isfinite(nrm).all(axis=1)
        at = np.nonzero(self.live)[0]
        # entry [i, s, k]: probe k (k < ao_rays: AO probe k; else light slot k - ao_rays) of sample s of point i
        self.unocc = np.zeros((N, n_samples, K), bool)
        self.tested = np.zeros((N, n_samples, K), bool)
        pixel = np.repeat(at, n_samples)
        sample = np.tile(np.arange(n_samples), len(at))
        pp, nn = np.repeat(p[at], n_samples, axis=0), np.repeat(nrm[at], n_samples, axis=0)
        for k in range(K):
            if len(at) == 0:
                break
            if k < ao_rays:
                d, skip = ao_dir(g.seed, frame, pixel, sample, k, ao_radius, nn), None
            else:
                L = desc.lights[lights[k - ao_rays]]
                d = light_dir(g.seed, frame, pixel, sample, k - ao_rays, L, pp)
                skip = np.full(len(pixel), L.shape_index, np.int32)
            occ = self.rq.occluded(pp, d, skip)
            self.unocc[at, :, k] = (occ == 0).reshape(len(at), n_samples)
            self.tested[at, :, k] = (~void_rays(pp, d)).reshape(len(at), n_samples)

    def planes(self, n_points=None, n_samples=None, ao_rays=None):
        """({"ao": (n_points,), "light": (n_points, slots)}, the number of non-void probes) of the leading n_points
        points, n_samples samples and ao_rays AO probes"""
        N = self.N if n_points is None else n_points
        n = self.n if n_samples is None else n_samples
        A = self.ao_rays if ao_rays is None else ao_rays
        assert N <= self.N and n <= self.n and A <= self.ao_rays
        un, te = self.unocc[:N, :n], self.tested[:N, :n]
        out = {}
        if A > 0:
            V = un[:, :, :A].sum(axis=(1, 2)).astype(np.int64)
            out["ao"] = (V.astype(np.float64) / (float(n) * float(A))).astype(f32)
        if self.lights:
            Vj = un[:, :, self.ao_rays:].sum(axis=1).astype(np.int64)
            out["light"] = (Vj.astype(np.float64) / float(n)).astype(f32)
        use = list(range(A)) + list(range(self.ao_rays, un.shape[2]))
        return out, int(te[:, :, use].sum())
