"""The prediction of the transmittance queries of include/dt.h (dt_rays_transmittance, dt_points_occlusion_glass),
built on tests/rayquery_ref.py and tests/points_occlusion_ref.py from the oracle's exports alone: the gather of
RayQueryRef along dir from start + 1e-3 dir, per gathered shape the oracle's or_shape_shadow(sn, start + 1e-3 sn,
t_max), the material from the descriptor, and the rules of dt.h: a counting shape that is not glass blocks (-1),
the counting glass shapes are counted, their k smallest indices listed.

Also the scenes and the ray sets of the tests, generated here so that tests/test_transmittance_host.py can check
on the CPU, by the restatement alone, that every class of ray is present before tests/test_gpu_transmittance.py
compares the kernels with it. A helper, not collected by pytest."""
import functools
import math

import numpy as np

import scene_gen
from occlusion_ref import ao_dir, light_dir
from rayquery_ref import RayQueryRef, void_rays

f32 = np.float32
MAX_PANES = 8   # DT_TRANSMIT_MAX_PANES


class TransmitRef:
    def __init__(self, built, g, rq=None):
        self.rq = rq if rq is not None else RayQueryRef(built, g)
        d = self.rq.desc
        self.glass = np.array([d.shapes[i].material == scene_gen.GLASS for i in range(d.n_shapes)], bool)

    def counting(self, start, dir, skip_shape=None):
        """per ray the sorted indices of the shapes that count (void rays: none)"""
        rq = self.rq
        start, dir = np.asarray(start, np.float64).reshape(-1, 3), np.asarray(dir, np.float64).reshape(-1, 3)
        out = [[] for _ in range(len(start))]
        live = np.nonzero(~void_rays(start, dir))[0]
        with np.errstate(all="ignore"):
            inds = rq.gather(dir[live], start[live] + 1e-3 * dir[live])
        for r, gathered in zip(live, inds):
            d, s = dir[r], start[r]
            dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            nn = math.sqrt(dd)
            t_max = f32(nn)
            sn = d / nn if dd > 0 else d
            ss = s + 1e-3 * sn
            skip = -1 if skip_shape is None else int(skip_shape[r])
            out[r] = sorted(si for si in gathered if si != skip and rq.orc.shadow(si, sn, ss, t_max))
        return out

    def transmittance(self, start, dir, skip_shape=None, k=0):
        """dt_rays_transmittance: {"panes": int32 (n,), "pane_shape": int32 (n, k)}"""
        cnt = self.counting(start, dir, skip_shape)
        n = len(cnt)
        panes = np.zeros(n, np.int32)
        shape = np.full((n, k), -1, np.int32)
        for r, c in enumerate(cnt):
            if any(not self.glass[si] for si in c):
                panes[r] = -1
                continue
            panes[r] = len(c)
            for j, si in enumerate(c[:k]):
                shape[r, j] = si
        return {"panes": panes, "pane_shape": shape}


class PointsTransmitRef:
    """tests/points_occlusion_ref.py PointsOcclusionRef with every probe answered by TransmitRef: per probe its
    panes, so that planes(max_panes, ...) is a cut in points, samples and AO probes, for any max_panes"""

    def __init__(self, built, g, frame, points, normals, n_samples, ao_rays, ao_radius, lights, tr=None):
        self.tr = tr if tr is not None else TransmitRef(built, g)
        desc = self.tr.rq.desc
        p = np.asarray(points, np.float64).reshape(-1, 3)
        nrm = np.asarray(normals, np.float64).reshape(-1, 3)
        N, K = len(p), ao_rays + len(lights)
        self.N, self.n, self.ao_rays, self.lights = N, n_samples, ao_rays, tuple(lights)
        self.live = np.isfinite(p).all(axis=1) & np.isfinite(nrm).all(axis=1)
        at = np.nonzero(self.live)[0]
        self.panes = np.full((N, n_samples, K), -1, np.int64)    # of a void point: never read
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
            self.panes[at, :, k] = self.tr.transmittance(pp, d, skip)["panes"].reshape(len(at), n_samples)
            self.tested[at, :, k] = (~void_rays(pp, d)).reshape(len(at), n_samples)

    def planes(self, max_panes, n_points=None, n_samples=None, ao_rays=None):
        """({"ao", "light", "ao_panes", "light_panes"}, the number of non-void probes)"""
        N = self.N if n_points is None else n_points
        n = self.n if n_samples is None else n_samples
        A = self.ao_rays if ao_rays is None else ao_rays
        assert N <= self.N and n <= self.n and A <= self.ao_rays
        pn, te, live = self.panes[:N, :n], self.tested[:N, :n], self.live[:N]
        un = (pn >= 0) & (pn <= max_panes) & live[:, None, None]
        ps = np.where(un, pn, 0)
        out = {}
        if A > 0:
            den = float(n) * float(A)
            out["ao"] = (un[:, :, :A].sum(axis=(1, 2)).astype(np.float64) / den).astype(f32)
            out["ao_panes"] = (ps[:, :, :A].sum(axis=(1, 2)).astype(np.float64) / den).astype(f32)
        if self.lights:
            out["light"] = (un[:, :, self.ao_rays:].sum(axis=1).astype(np.float64) / float(n)).astype(f32)
            out["light_panes"] = (ps[:, :, self.ao_rays:].sum(axis=1).astype(np.float64) / float(n)).astype(f32)
        use = list(range(A)) + list(range(self.ao_rays, pn.shape[2]))
        return out, int(te[:, :, use].sum())


# ---------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------
def pane_stack(n_panes=5):
    """n_panes glass rectangles at z = 1 .. n_panes over x in [-2, 2], y in [0, 4], an opaque wall behind them at
    z = n_panes + 1 over the lower half (y in [0, 2]) only, and a glass sphere off to the side at (4, 2, 3).
    Shapes: panes 0 .. n_panes-1, the wall n_panes, the sphere n_panes + 1. No light."""
    b = scene_gen._Builder(1.0, (0.0, 0.0, 0.0))
    for j in range(n_panes):
        z = float(j + 1)
        scene_gen._rect(b, (-2, 0, z), (2, 0, z), (2, 4, z), (-2, 4, z), (0.9, 1.0, 0.9), flags=0,
                        material=scene_gen.GLASS)
    z = float(n_panes + 1)
    scene_gen._rect(b, (-2, 0, z), (2, 0, z), (2, 2, z), (-2, 2, z), (0.9, 0.5, 0.2), flags=0)
    b.shape(scene_gen.SPHERE, v=[(4.0, 2.0, 3.0)], radius=0.75, color=(0.9, 0.9, 1.0), material=scene_gen.GLASS,
            center=(4.0, 2.0, 3.0))
    g = b.globals((0.0, 2.0, -6.0), (0.0, 2.0, 0.0), 0.0625, 6.0)
    return scene_gen._shade_globals(b, g)


STACK_WALL, STACK_SPHERE = 5, 6           # pane_stack(5)
GLASS_FLOOR, GLASS_WALL, GLASS_SPHERE, GLASS_PANE = 0, 1, 2, 3   # scene_gen.shade_glass


def _jit(rng, n, w):
    return rng.uniform(-w, w, n)


def stack_rays(n=64 * 3 + 7, seed=11):
    """Rays of pane_stack(5), twelve recipes in turn (ray i: recipe i % 12), so that every wave holds every
    class and four distinct skip_shape values beside -1. From z = 0 towards +z, tilted by up to 0.15 in x and y
    over the whole segment; recipe 10 is axis-parallel (the inf_wave walk)."""
    rng = np.random.default_rng(seed)
    start, dir, skip = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, -1, np.int32)
    for i in range(n):
        rc = i % 12
        x, tx, ty = _jit(rng, 1, 1.6)[0], _jit(rng, 1, 0.15)[0], _jit(rng, 1, 0.15)[0]
        lower, upper = 0.4 + rng.uniform(0, 1.1), 2.6 + rng.uniform(0, 1.0)
        if rc == 0:     # ends before the first pane: clear
            s, d = (x, lower, 0), (tx, ty, 0.5)
        elif rc == 1:   # one pane
            s, d = (x, lower, 0), (tx, ty, 1.5)
        elif rc == 2:   # three panes
            s, d = (x, upper, 0), (tx, ty, 3.5)
        elif rc == 3:   # five panes, the wall beyond t_max
            s, d = (x, lower, 0), (tx, ty, 5.5)
        elif rc == 4:   # the wall: blocked
            s, d = (x, lower, 0), (tx, ty, 7.0)
        elif rc == 5:   # over the wall: five panes
            s, d = (x, upper, 0), (tx, ty, 7.0)
        elif rc == 6:   # the one pane crossed is the skip shape
            s, d, skip[i] = (x, lower, 0), (tx, ty, 1.5), 0
        elif rc == 7:   # three panes, the second skipped
            s, d, skip[i] = (x, upper, 0), (tx, ty, 3.5), 1
        elif rc == 8:   # ends inside the glass sphere
            s = (4.0 + tx, 2.0 + ty, 0.0)
            d = (4.0 + _jit(rng, 1, 0.2)[0] - s[0], 2.0 + _jit(rng, 1, 0.2)[0] - s[1], 3.0 + _jit(rng, 1, 0.2)[0])
        elif rc == 9:   # through the glass sphere, which is the skip shape
            s, d, skip[i] = (4.0 + tx, 2.0 + ty, 0.0), (-tx, -ty, 7.0), STACK_SPHERE
        elif rc == 10:  # axis-parallel: one pane
            s, d = (x, lower, 0), (0.0, 0.0, 1.5)
        else:           # the wall skipped: five panes
            s, d, skip[i] = (x, lower, 0), (tx, ty, 7.0), STACK_WALL
        start[i], dir[i] = s, d
    return start, dir, skip


def glass_rays(n=64 * 3 + 7, seed=12):
    """Rays of scene_gen.shade_glass, twelve recipes in turn: from z = 4 towards -z through the pane (x in
    [-2.5, -0.5], y in [0.25, 2.25], z in [1.25, 1.5]) or the sphere ((1.25, 1, 1), r 0.5625), and along +x
    through both."""
    rng = np.random.default_rng(seed)
    start, dir, skip = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, -1, np.int32)
    for i in range(n):
        rc = i % 12
        x, y = -1.5 + _jit(rng, 1, 0.8)[0], 1.25 + _jit(rng, 1, 0.75)[0]
        tx, ty = _jit(rng, 1, 0.1)[0], _jit(rng, 1, 0.1)[0]
        sx, sy = 1.25 + _jit(rng, 1, 0.15)[0], 1.0 + _jit(rng, 1, 0.15)[0]
        if rc == 0:     # ends before the pane: clear
            s, d = (x, y, 4), (tx, ty, -2.0)
        elif rc == 1:   # the pane; the wall beyond t_max
            s, d = (x, y, 4), (tx, ty, -4.0)
        elif rc == 2:   # to the wall, which is the skip shape: the pane, then the cylinder or nothing
            s, d, skip[i] = (x, y, 4), (tx, ty, -9.0), GLASS_WALL
        elif rc == 3:   # along x through pane and sphere
            s, d = (-3.5, 1.0 + ty, 1.3 + 0.5 * tx), (6.5, 0.5 * ty, 0.0)
        elif rc == 4:   # the same, steeper
            s, d = (-3.5, 1.0 + ty, 1.35 + 0.5 * tx), (6.5, ty, -0.1)
        elif rc == 5:   # the pane is the skip shape
            s, d, skip[i] = (x, y, 4), (tx, ty, -4.0), GLASS_PANE
        elif rc == 6:   # ends inside the sphere
            s, d = (sx, sy, 4), (1.25 + 2 * tx - sx, 1.0 + 2 * ty - sy, -3.0 + tx)
        elif rc == 7:   # ... which is the skip shape
            s, d, skip[i] = (sx, sy, 4), (1.25 + 2 * tx - sx, 1.0 + 2 * ty - sy, -3.0 + tx), GLASS_SPHERE
        elif rc == 8:   # over everything
            s, d = (x, 3.0 + ty, 4), (tx, ty, -4.0)
        elif rc == 9:   # axis-parallel through the pane
            s, d = (x, y, 4), (0.0, 0.0, -4.0)
        elif rc == 10:  # through the sphere to the wall: blocked
            s, d = (sx, sy, 4), (tx, ty, -9.0)
        else:           # pane and sphere, an unrelated skip shape
            s, d, skip[i] = (-3.5, 1.0 + ty, 1.3 + 0.5 * tx), (6.5, 0.5 * ty, 0.0), GLASS_FLOOR
        start[i], dir[i] = s, d
    return start, dir, skip


def blocked_wave_rays(n_clear, seed=13):
    """64 rays of pane_stack(5) that all end on the wall (blocked), but for the n_clear rays at lanes 37 .. that
    pass over it"""
    rng = np.random.default_rng(seed)
    start, dir = np.zeros((64, 3)), np.zeros((64, 3))
    for i in range(64):
        over = 37 <= i < 37 + n_clear
        start[i] = (_jit(rng, 1, 1.6)[0], (2.6 if over else 0.4) + rng.uniform(0, 1.0), 0.0)
        dir[i] = (_jit(rng, 1, 0.15)[0], _jit(rng, 1, 0.15)[0], 7.0)
    return start, dir, None


def floor_points(n):
    """n points (of 16 x 16) of the floor of shade_glass behind its pane as the first light sees it, row by row,
    with the floor's normal"""
    u = (np.arange(16) + 0.5) / 16
    x, z = np.meshgrid(-2.4 + 1.8 * u, -0.6 + 1.8 * u)
    p = np.stack([x.reshape(-1), np.zeros(256), z.reshape(-1)], axis=1)[:n]
    return np.ascontiguousarray(p), np.ascontiguousarray(np.tile([0.0, 1.0, 0.0], (len(p), 1)))


def classes(tr, start, dir, skip, k):
    """the classes of rays of a set, by the restatement alone: name -> bool per ray"""
    n = len(start)
    sk = skip if skip is not None else np.full(n, -1, np.int32)
    a = tr.transmittance(start, dir, skip)["panes"]
    far = tr.transmittance(start, 4.0 * dir, skip)["panes"]        # the same rays, four times as long
    unskipped = tr.counting(start, dir, None)
    sph = [i for i in range(len(tr.glass)) if tr.glass[i] and tr.rq.desc.shapes[i].type == scene_gen.SPHERE]
    inside = np.zeros(n, bool)
    for si in sph:
        sh = tr.rq.desc.shapes[si]
        c = np.array([sh.center[0], sh.center[1], sh.center[2]])
        inside |= np.linalg.norm(start + dir - c, axis=1) < sh.radius
    return {
        "clear": a == 0,
        "blocked": a == -1,
        "one pane": a == 1,
        "two panes or more": a >= 2,
        "more panes than k": a > k,
        "a pane that is the skip shape": np.array([sk[i] >= 0 and tr.glass[sk[i]] and sk[i] in unskipped[i]
                                                   for i in range(n)], bool),
        "ends inside a glass sphere": inside,
        "ends before the pane": (a >= 0) & ((far > a) | (far == -1)) &
                                np.array([len(c) == 0 for c in tr.counting(start, dir, skip)], bool),
        "opaque behind the pane beyond t_max": (a >= 1) & (far == -1),
    }


# ---------------------------------------------------------------------------------------------------
# the cases of the tests, computed once and never written to
# ---------------------------------------------------------------------------------------------------
K_CLASS = {"stack": 3, "glass": 1}   # the k of "more panes than k" per scene


@functools.lru_cache(maxsize=None)
def scene(name):
    desc, g, keep = pane_stack(5) if name == "stack" else scene_gen.shade_glass()
    return desc, g, keep, TransmitRef(desc, g)


@functools.lru_cache(maxsize=None)
def ray_set(name):
    """(start, dir, skip) of the main ray set of a scene, read-only"""
    s, d, k = stack_rays() if name == "stack" else glass_rays()
    for a in (s, d, k):
        a.setflags(write=False)
    return s, d, k


@functools.lru_cache(maxsize=None)
def prediction(name, k):
    tr = scene(name)[3]
    s, d, sk = ray_set(name)
    out = tr.transmittance(s, d, sk, k)
    for a in out.values():
        a.setflags(write=False)
    return out


POINTS = dict(n=256, frame=5, n_samples=5, ao_rays=4, ao_radius=0.75, lights=(0, 1))


@functools.lru_cache(maxsize=None)
def points_case():
    """(PointsTransmitRef of 256 floor points x 5 samples x (4 AO probes + 2 lights), points, normals)"""
    desc, g, keep, tr = scene("glass")
    p, nrm = floor_points(POINTS["n"])
    p[100] = (np.nan, 0.0, 0.0)   # a void point in the middle of the second wave
    for a in (p, nrm):
        a.setflags(write=False)
    ref = PointsTransmitRef(desc, g, POINTS["frame"], p, nrm, POINTS["n_samples"], POINTS["ao_rays"],
                            POINTS["ao_radius"], POINTS["lights"], tr=tr)
    return ref, p, nrm
