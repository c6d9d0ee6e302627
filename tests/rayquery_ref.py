"""The prediction of the ray queries of include/dt.h (dt_trace_rays, dt_rays_occluded), built from the oracle's
exports only: the tree of oracle.bvh, the slab test of oracle.c's box_intersect restated in numpy with its
float32 casts (vectorised over rays and nodes), the stack-order gather, and per gathered shape the oracle's
own or_shape_intersect / or_shape_shadow; the attributes of a hit as tests/test_gpu_features.py's predict
computes them per sample (or_shape_norm, or_fix_norm, the colour intersect() leaves, uv, texel).

The gather: oracle.bvh exports the nodes in the reference's stack-pop order (pre-order, last child first),
so the leaves in array order are the one order in which any ray gathers them; a ray keeps the leaves whose
box and whose ancestors' boxes it passes. A helper, not collected by pytest."""
import ctypes
import math

import numpy as np

import oracle
from oracle import geom as G

f32 = np.float32
FLT_MIN = np.finfo(np.float32).tiny
FLT_MAX = np.finfo(np.float32).max
F_TEXTURE = 1 << 2
ATTRS = ("point", "normal", "albedo")


def _desc(built):
    return built.desc if hasattr(built, "desc") else built


def void_rays(start, dir):
    """rays that are never traced: a non-finite component, or an all-zero direction"""
    start, dir = np.asarray(start, np.float64).reshape(-1, 3), np.asarray(dir, np.float64).reshape(-1, 3)
    return ~(np.isfinite(start).all(axis=1) & np.isfinite(dir).all(axis=1)) | (dir == 0).all(axis=1)


def box_pass(lb, ub, ray, start):
    """oracle.c box_intersect (bump 0) of every ray (R, 3) with every box (N, 3): (R, N) bool. The early
    returns of the C become a cleared `ok`: nothing after them has a side effect."""
    with np.errstate(all="ignore"):
        inv = 1.0 / ray
        ok = np.ones((len(ray), len(lb)), bool)
        tmin = tmax = None
        for a in range(3):
            r, ir, st = ray[:, a, None], inv[:, a, None], start[:, a, None]
            l, u = lb[None, :, a], ub[None, :, a]
            par = np.isinf(ir)
            inside = (st >= l) & (st <= u)
            lo, hi = np.where(r < 0, u, l), np.where(r < 0, l, u)
            amin = np.where(par, FLT_MIN, ((lo - st) * ir).astype(f32)).astype(f32)
            amax = np.where(par, FLT_MAX, ((hi - st) * ir).astype(f32)).astype(f32)
            ok &= np.where(par, inside, True)
            if a == 0:
                tmin, tmax = amin, amax
            else:
                ok &= ~((tmin > amax) | (amin > tmax))
                tmin = np.where(amin > tmin, amin, tmin)
                tmax = np.where(amax < tmax, amax, tmax)
        return ok & (tmax > 0)


def _texel(desc, sh, u, v):
    """oracle.c's light loop: float products, truncation, the clamped index, byte / 255.0"""
    T = desc.textures[sh.tex_frame]
    x_tex = int(f32(T.width - 1) * f32(u))
    y_tex = int(f32(T.height - 1) * f32(v))
    ind = int(y_tex * float(T.width) + x_tex)
    ind = min(max(ind, 0), T.width * T.height - 1)
    return [T.pixels[ind * T.channels + k] / 255.0 for k in range(3)]


class RayQueryRef:
    def __init__(self, built, g):
        self.built = built
        self.desc = _desc(built)
        nodes, idx = oracle.bvh(built, g)
        self.idx = idx
        n = len(nodes)
        self.lb = np.array([list(b.lbound) for b in nodes], np.float64).reshape(n, 3)
        self.ub = np.array([list(b.ubound) for b in nodes], np.float64).reshape(n, 3)
        self.parent = np.full(n, -1)
        last_at = {}
        for i, b in enumerate(nodes):
            if b.depth > 0:
                self.parent[i] = last_at[b.depth - 1]
            last_at[b.depth] = i
        self.leaves = [(i, b.first_index, b.n_indices) for i, b in enumerate(nodes) if b.leaf and b.n_indices > 0]
        rec, hrec = G.records_from_desc(self.desc)
        self.orc = G.Oracle(rec, hrec)

    def gather(self, ray, start):
        """per ray the shape indices the reference's stack walk gathers, in its order"""
        ray, start = np.asarray(ray, np.float64).reshape(-1, 3), np.asarray(start, np.float64).reshape(-1, 3)
        if len(self.lb) == 0:
            return [[] for _ in ray]
        ok = box_pass(self.lb, self.ub, ray, start)
        for i in range(len(self.lb)):   # pre-order: a parent comes before its children
            if self.parent[i] >= 0:
                ok[:, i] &= ok[:, self.parent[i]]
        return [[self.idx[first + k] for (i, first, cnt) in self.leaves if ok[r, i] for k in range(cnt)]
                for r in range(len(ray))]

    def trace(self, start, dir, attrs=True):
        """dt_trace_rays: ({shape, t[, point, normal, albedo]}, seen); seen holds the three stats counters, the
        number of rays traced and what kinds of hits occurred"""
        start, dir = np.asarray(start, np.float64).reshape(-1, 3), np.asarray(dir, np.float64).reshape(-1, 3)
        n = len(start)
        out = {"shape": np.full(n, -1, np.int32), "t": np.full(n, FLT_MAX, np.float32)}
        if attrs:
            for k in ATTRS:
                out[k] = np.zeros((n, 3))
        seen = {"rays": 0, "tex_fetches": 0, "uv_out_of_range": 0, "prism_norm_fallback": 0, "textured": 0,
                "checker": 0, "border": 0}
        live = np.nonzero(~void_rays(start, dir))[0]
        seen["rays"] = int(live.size)
        orc, o = self.orc, self.orc.o
        inds = self.gather(dir[live], start[live])
        for r, gathered in zip(live, inds):
            rp, sp = G._d(dir[r])[1], G._d(start[r])[1]
            t, t_min, hit_i, hit_hole, any_hit = ctypes.c_float(FLT_MAX), FLT_MAX, -1, -1, False
            for si in gathered:   # strict < in gather order, t carried from shape to shape
                ins, hole = ctypes.c_int(0), ctypes.c_int(-1)
                if o.or_shape_intersect(orc.dp, si, rp, sp, ctypes.byref(t), ctypes.byref(ins), ctypes.byref(hole)):
                    any_hit = True
                    if f32(t.value) < t_min:
                        hit_i, t_min, hit_hole = si, f32(t.value), hole.value
            if not any_hit or hit_i < 0:
                continue
            out["shape"][r], out["t"][r] = hit_i, t_min
            if not attrs:
                continue
            d, s, tt = dir[r], start[r], float(t_min)
            sh = self.desc.shapes[hit_i]
            p = s + tt * d
            nrm = np.zeros(3)
            seen["prism_norm_fallback"] += o.or_shape_norm(orc.dp, hit_i, G._d(p)[1], hit_hole, nrm.ctypes.data_as(G._D))
            rr = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            nrm = orc.fix_norm(d / math.sqrt(rr) if rr > 0 else d, nrm)
            col = np.zeros(3)
            o.or_shape_color_after_hit(orc.dp, hit_i, rp, sp, col.ctypes.data_as(G._D))
            c = [float(col[0]), float(col[1]), float(col[2])]
            if c != list(sh.color):
                seen["checker"] += 1
            if sh.flags & F_TEXTURE:
                uv, kind = orc.uv(hit_i, p)
                if kind == 2:
                    c = list(sh.bordercolor)
                    seen["border"] += 1
                elif kind == 1 and sh.tex_frame >= 0:
                    c = _texel(self.desc, sh, uv[0], uv[1])
                    seen["tex_fetches"] += 1
                    seen["textured"] += 1
                if kind != 0 and (uv[0] < 0 or uv[1] < 0 or uv[0] > 1 or uv[1] > 1):
                    seen["uv_out_of_range"] += 1
            out["point"][r], out["normal"][r], out["albedo"][r] = p, nrm, c
        return out, seen

    def occluded(self, start, dir, skip_shape=None):
        """dt_rays_occluded: uint8 per ray. oracle.c's light loop with sray = dir: the gather along dir from
        start + 1e-3 dir, or_shape_shadow(sn, start + 1e-3 sn, t_max) over the gathered shapes but skip_shape"""
        start, dir = np.asarray(start, np.float64).reshape(-1, 3), np.asarray(dir, np.float64).reshape(-1, 3)
        n = len(start)
        out = np.zeros(n, np.uint8)
        live = np.nonzero(~void_rays(start, dir))[0]
        with np.errstate(all="ignore"):
            inds = self.gather(dir[live], start[live] + 1e-3 * dir[live])
        for r, gathered in zip(live, inds):
            d, s = dir[r], start[r]
            dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            nn = math.sqrt(dd)
            t_max = f32(nn)
            sn = d / nn if dd > 0 else d   # normalized(): a vector whose squared length underflows stays as it is
            ss = s + 1e-3 * sn
            skip = -1 if skip_shape is None else int(skip_shape[r])
            for si in gathered:
                if si != skip and self.orc.shadow(si, sn, ss, t_max):
                    out[r] = 1
                    break
        return out
