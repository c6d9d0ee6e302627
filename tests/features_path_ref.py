"""The prediction of the specular-path feature buffers (include/dt.h dt_render_features_path, dt_guide_bounce),
built from the oracle's exports only.

Per segment: the gather of tests/rayquery_ref.py (RayQueryRef.gather) and its closest-hit loop over
or_shape_intersect, keeping `inside` as oracle.c's rayColor keeps it (the closest shape's), then or_shape_norm /
or_fix_norm, the colour intersect() leaves, uv and the texel, as RayQueryRef.trace computes them. The bounce
rule is restated here in numpy with its float32 casts (bounce_rule), vectorised over hits. Primary rays:
G.or_primary_ray in dt_intersect_primary's numbering. The sums are f64, left to right in sample order from +0
(np.add.accumulate is sequential); a sample that does not end on a surface adds zeros, which changes no bit
of a sum that started at +0.

PathRef.trace follows every sample for up to max_bounces segments beyond the first once and keeps every
segment's record; planes(n, K) cuts the paths at K <= max_bounces and sums the leading n samples: a sample's
path under K is its path under max_bounces up to segment K. A helper, not collected by pytest."""
import ctypes
import math

import numpy as np

from oracle import geom as G
from rayquery_ref import F_TEXTURE, FLT_MAX, RayQueryRef, _texel, f32, void_rays

GLASS, STEEL, ALUMINUM, WATER, LINOLEUM = 1, 2, 3, 4, 5
F_GLOSSY = 1 << 3
STOP, REFLECT, REFRACT = 0, 1, 2
EPS = float(f32(1e-3))   # 1e-3f, promoted where it meets a double
PLANES = ("albedo", "normal", "depth", "coverage", "shape", "bounces")
COUNTERS = ("rays", "reflect_errors", "tex_fetches", "uv_out_of_range", "prism_norm_fallback")


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def bounce_rule(g, material, flags, inside, in_, n, p):
    """dt_guide.h guide_bounce over N hits: material, flags, inside (N,), in_ = the normalised ray, n = the
    fixNorm'ed normal, p = the hit point (N, 3 f64) -> dict code (N,), dir, start (N, 3; meaningful where code is
    not STOP), refl_err, and the intermediate chk, rn (what the tests assert their cases by)"""
    material, flags, inside = np.asarray(material), np.asarray(flags).astype(np.int64), np.asarray(inside)
    in_, n, p = (np.asarray(a, np.float64).reshape(-1, 3) for a in (in_, n, p))
    with np.errstate(all="ignore"):
        refl_mat = np.isin(material, (GLASS, STEEL, ALUMINUM, WATER, LINOLEUM))
        glossy = (flags & F_GLOSSY) != 0
        specular = refl_mat & ~(glossy & (not g.nogloss)) if g.reflect else np.zeros(len(material), bool)
        cos_theta = _dot(n, -in_).astype(f32)
        ct = cos_theta.astype(np.float64)
        sin_theta = np.sqrt(1 - ct * ct).astype(f32)
        ra, rg = f32(g.refr_air), f32(g.refr_glass)
        r1 = np.where(inside != 0, rg, ra).astype(f32)
        r2 = np.where(inside != 0, ra, rg).astype(f32)
        q = r1 / r2
        qd, dn = q.astype(np.float64), _dot(in_, n)
        chk = (1 - (qd * qd) * (1 - dn * dn)).astype(f32)
        a, b, sq = q * sin_theta, f32(1) / sin_theta, np.sqrt(chk)
        assert a.dtype == b.dtype == sq.dtype == q.dtype == np.float32
        a, b, sq = (v.astype(np.float64)[:, None] for v in (a, b, sq))
        refr_dir = a * (b * (in_ + ct[:, None] * n)) - sq * n
        refr_start = p + EPS * in_
        refl = in_ - (2 * _dot(n, in_))[:, None] * n
        rn = _dot(refl, n)
        refl_start = p + EPS * refl
        refract = specular & (material == GLASS) & (chk >= 0)
        mirror = specular & ~refract
        refl_err = mirror & (rn <= 0)
        reflect = mirror & ~(rn <= 0) & ~(rn <= EPS)
    code = np.where(refract, REFRACT, np.where(reflect, REFLECT, STOP))
    return {"code": code, "dir": np.where(refract[:, None], refr_dir, refl),
            "start": np.where(refract[:, None], refr_start, refl_start), "refl_err": refl_err, "chk": chk, "rn": rn,
            "specular": specular}


class PathRef:
    GATHER_CHUNK = 4096   # rays per vectorised gather (rays x nodes temporaries)

    def __init__(self, built, g):
        self.rq = RayQueryRef(built, g)
        self.desc = self.rq.desc

    def _segment(self, start, dir):
        """one segment of len(start) rays: per ray traced, hit, shape, inside, t, point, normal, colour, the
        length t * |dir| and the counters of that hit (prism for the normal; tex, uv, and the kinds for the colour)"""
        R = len(start)
        out = {"traced": ~void_rays(start, dir), "hit": np.zeros(R, bool), "shape": np.full(R, -1, np.int32),
               "inside": np.zeros(R, np.int32), "p": np.zeros((R, 3)), "n": np.zeros((R, 3)), "in": np.zeros((R, 3)),
               "col": np.zeros((R, 3)), "len": np.zeros(R), "prism": np.zeros(R, np.int64),
               "tex": np.zeros(R, np.int64), "uv": np.zeros(R, np.int64), "border": np.zeros(R, bool),
               "checker": np.zeros(R, bool)}
        orc, o, desc = self.rq.orc, self.rq.orc.o, self.desc
        live = np.nonzero(out["traced"])[0]
        for c0 in range(0, live.size, self.GATHER_CHUNK):
            idx = live[c0:c0 + self.GATHER_CHUNK]
            for r, gathered in zip(idx, self.rq.gather(dir[idx], start[idx])):
                d, s = dir[r], start[r]
                rp, sp = G._d(d)[1], G._d(s)[1]
                t, t_min, hit_i, hit_hole, hit_ins, any_hit = ctypes.c_float(FLT_MAX), FLT_MAX, -1, -1, 0, False
                for si in gathered:   # strict < in gather order, t carried from shape to shape
                    ins, hole = ctypes.c_int(0), ctypes.c_int(-1)
                    if o.or_shape_intersect(orc.dp, si, rp, sp, ctypes.byref(t), ctypes.byref(ins), ctypes.byref(hole)):
                        any_hit = True
                        if f32(t.value) < t_min:
                            hit_i, t_min, hit_hole, hit_ins = si, f32(t.value), hole.value, ins.value
                if not any_hit or hit_i < 0:
                    continue
                tt = float(t_min)
                sh = desc.shapes[hit_i]
                p = s + tt * d
                nrm = np.zeros(3)
                out["prism"][r] = o.or_shape_norm(orc.dp, hit_i, G._d(p)[1], hit_hole, nrm.ctypes.data_as(G._D))
                rr = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                rn = math.sqrt(rr)
                in_ = d / rn if rr > 0 else d
                col = np.zeros(3)
                o.or_shape_color_after_hit(orc.dp, hit_i, rp, sp, col.ctypes.data_as(G._D))
                c = [float(col[0]), float(col[1]), float(col[2])]
                out["checker"][r] = c != list(sh.color)
                if sh.flags & F_TEXTURE:
                    uv, kind = orc.uv(hit_i, p)
                    if kind == 2:
                        c = list(sh.bordercolor)
                        out["border"][r] = True
                    elif kind == 1 and sh.tex_frame >= 0:
                        c = _texel(desc, sh, uv[0], uv[1])
                        out["tex"][r] = 1
                    if kind != 0 and (uv[0] < 0 or uv[1] < 0 or uv[0] > 1 or uv[1] > 1):
                        out["uv"][r] = 1
                out["hit"][r], out["shape"][r], out["inside"][r] = True, hit_i, hit_ins
                out["p"][r], out["n"][r], out["in"][r], out["col"][r] = p, orc.fix_norm(in_, nrm), in_, c
                out["len"][r] = tt * rn
        return out

    def trace(self, g, frame, n, max_bounces):
        """follow the samples 0 .. n-1 of every pixel of g for segments 0 .. max_bounces; the rule is evaluated
        at every hit (planes() ignores it at the cut)"""
        W, H = g.xRes, g.yRes
        nb = (n + 7) // 8
        start, ray = G.or_primary_ray(g, frame, 0, nb * W * H * 8)
        i, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing="ij")
        r = ((i // 8) * W * H + y * W + x) * 8 + i % 8
        # sample-major: entry [y, x, i]
        r = r.transpose(1, 2, 0).reshape(-1)
        start, ray = start.reshape(-1, 3)[r].copy(), ray.reshape(-1, 3)[r].copy()
        S = len(r)
        self.g, self.W, self.H, self.n, self.K = g, W, H, n, max_bounces
        self.seg = []
        at = np.arange(S)   # the samples still travelling
        mat = np.array([self.desc.shapes[k].material for k in range(self.desc.n_shapes)])
        flg = np.array([self.desc.shapes[k].flags for k in range(self.desc.n_shapes)], np.int64)
        for k in range(max_bounces + 1):
            seg = self._segment(start, ray)
            hs = np.where(seg["hit"], seg["shape"], 0)
            rule = bounce_rule(g, mat[hs], flg[hs], seg["inside"], seg["in"], seg["n"], seg["p"])
            seg["code"] = np.where(seg["hit"], rule["code"], STOP)
            seg["refl_err"] = seg["hit"] & rule["refl_err"]
            seg["chk"], seg["material"], seg["sample"] = rule["chk"], np.where(seg["hit"], mat[hs], -1), at
            self.seg.append(seg)
            go = seg["code"] != STOP
            at, start, ray = at[go], rule["start"][go], rule["dir"][go]
            if at.size == 0:
                break
        return self

    def planes(self, n, K):
        """({plane: array in image order [y, x]}, counters) of the leading n samples at max_bounces = K"""
        assert n <= self.n and K <= self.K
        W, H, S = self.W, self.H, self.W * self.H * self.n
        A, N, D = np.zeros((S, 3)), np.zeros((S, 3)), np.zeros(S)
        ended, end_shape, followed = np.zeros(S, bool), np.full(S, -1, np.int32), np.zeros(S)
        cnt = dict.fromkeys(COUNTERS, 0)
        length = np.zeros(S)   # L so far, per sample
        first = (np.arange(S) % self.n) < n
        for k, seg in enumerate(self.seg[:K + 1]):
            sm = seg["sample"]
            use = first[sm]
            cnt["rays"] += int((use & seg["traced"]).sum())
            hit = use & seg["hit"]
            cnt["prism_norm_fallback"] += int(seg["prism"][hit].sum())
            length[sm[hit]] = length[sm[hit]] + seg["len"][hit]
            goes = hit & (seg["code"] != STOP) if k < K else np.zeros(len(sm), bool)
            if k < K:
                cnt["reflect_errors"] += int((hit & seg["refl_err"]).sum())
            followed[sm[goes]] += 1
            end = hit & ~goes
            e = sm[end]
            ended[e], end_shape[e] = True, seg["shape"][end]
            A[e], N[e], D[e] = seg["col"][end], seg["n"][end], length[e]
            cnt["tex_fetches"] += int(seg["tex"][end].sum())
            cnt["uv_out_of_range"] += int(seg["uv"][end].sum())

        def total(v):   # the f64 left-to-right sum from +0 over the leading n samples
            v = v.reshape((H, W, self.n) + v.shape[1:])[:, :, :n]
            z = np.zeros((H, W, 1) + v.shape[3:])
            return np.add.accumulate(np.concatenate([z, v], axis=2), axis=2)[:, :, -1]

        nn = float(n)
        Hs = total(ended.astype(np.float64))
        with np.errstate(all="ignore"):
            depth = np.where(Hs > 0, (total(D) / Hs).astype(f32), f32(0)).astype(f32)
        out = {"albedo": (total(A) / nn).astype(f32), "normal": (total(N) / nn).astype(f32), "depth": depth,
               "coverage": (Hs / nn).astype(f32), "shape": end_shape.reshape(H, W, self.n)[:, :, 0].copy(),
               "bounces": (total(followed) / nn).astype(f32)}
        return out, cnt

    def per_sample(self, K):
        """(ended, followed) per sample [y, x, i] at max_bounces = K, for the tests' own assertions"""
        S = self.W * self.H * self.n
        ended, followed = np.zeros(S, bool), np.zeros(S, np.int64)
        for k, seg in enumerate(self.seg[:K + 1]):
            goes = seg["hit"] & (seg["code"] != STOP) if k < K else np.zeros(len(seg["sample"]), bool)
            followed[seg["sample"][goes]] += 1
            ended[seg["sample"][seg["hit"] & ~goes]] = True
        return ended.reshape(self.H, self.W, self.n), followed.reshape(self.H, self.W, self.n)
