"""The prediction of the path ray queries (include/dt.h dt_trace_rays_path), built from PathRef._segment and
bounce_rule of tests/features_path_ref.py only: the per-sample chain of dt_render_features_path with the caller's
ray as segment 0, answered per ray. The same planes and the same counters as the call.

RayPathRef.trace follows the rays segment by segment over the set still travelling. A segment's record is
PathRef._segment's (the void-ray rule, the closest hit with `inside`, p, the fixNorm'ed normal, the colour and its
counters, t * |dir|); the rule is bounce_rule, evaluated iff k < K. `log` keeps every segment's record and rule for
the tests' own assertions. A helper, not collected by pytest."""
import functools

import numpy as np

from features_path_ref import REFLECT, REFRACT, STOP, PathRef, bounce_rule
from oracle import geom as G

VOID, MISS, SURFACE, CUT = 0, 1, 2, 3   # DT_PATH_*
PLANES = ("end", "segments", "shape", "length", "point", "normal", "albedo", "last_start", "last_dir", "seg_shape",
          "seg_point")
COUNTERS = ("rays", "reflect_errors", "tex_fetches", "uv_out_of_range", "prism_norm_fallback")


GLASS_SPHERE, STEEL_SPHERE = 1, 2   # their indices in scene_gen.features
GLASS_CENTRE, GLASS_RADIUS = (0.5, 1.0, 0.0), 0.6
STEEL_CENTRE, STEEL_RADIUS = (-1.2, 0.7, 0.5), 0.5


def unit_scene(aa=1):
    """the 24x16 "unit" scene of tests/test_gpu_features_path.py (_unit: scene_gen.features with the eye moved
    closer to the glass and the steel sphere), with nogloss = 1"""
    import scene_gen
    desc, g, keep = scene_gen.features(*scene_gen.CASES["unit"])
    g.xRes, g.yRes, g.antialias_samples = 24, 16, aa
    for a, v in enumerate((-2.2, 1.5, 3.2)):
        g.eye[a] = v
    for a, v in enumerate((-0.3, 0.8, 0.2)):
        g.lookingAt[a] = v
    g.nogloss = 1
    return desc, g, keep


def hand_made_rays():
    """rays the camera does not shoot, on the unit scene: (start, dir, {name: indices})"""
    nan, inf = float("nan"), float("inf")
    gc, gr, sc, sr = GLASS_CENTRE, GLASS_RADIUS, STEEL_CENTRE, STEEL_RADIUS
    rays, names = [], {}

    def add(name, s, d):
        names.setdefault(name, []).append(len(rays))
        rays.append((s, d))

    add("nan_start", (0.0, nan, 0.0), (0.0, -1.0, 0.0))
    add("zero_dir", (0.0, 2.0, 0.0), (0.0, 0.0, 0.0))
    add("inf", (0.0, 2.0, 0.0), (inf, -1.0, 0.0))
    # through the glass sphere's centre: normal incidence, the successor is a void ray
    add("through_centre", (gc[0], gc[1], gc[2] + 3.0), (0.0, 0.0, -1.0))
    # from inside the glass sphere, near its surface, towards it at a shallow angle: total internal reflection
    for dy, dz in ((1.0, 0.2), (1.0, -0.3), (-1.0, 0.25), (0.7, 1.0)):
        add("inside", (gc[0] + 0.5, gc[1], gc[2]), (0.05, dy, dz))
    # from inside, steeply: refraction out
    add("inside_out", (gc[0] + 0.1, gc[1], gc[2]), (1.0, 0.2, 0.1))
    add("miss", (3.0, 5.0, 0.0), (0.0, 1.0, 0.1))
    # grazing the steel sphere: along x, a hair inside its silhouette
    for delta in (2e-8, 5e-8, 1e-7, 2e-7):
        add("grazing", (sc[0] - 2.0, sc[1], sc[2] + sr - delta), (1.0, 0.0, 0.0))
    # at the steel sphere squarely, and at the floor
    add("steel", (-3.0, 2.0, 2.0), (sc[0] + 3.0, sc[1] - 2.0 + 0.1, sc[2] - 2.0))
    add("floor", (0.0, 2.0, 2.0), (0.3, -1.0, 0.2))
    add("glass", (-2.0, 2.0, 2.5), (gc[0] + 2.0 + 0.2, gc[1] - 2.0, gc[2] - 2.5))
    start = np.array([r[0] for r in rays], np.float64)
    dir = np.array([r[1] for r in rays], np.float64)
    return start, dir, {k: np.array(v) for k, v in names.items()}


def camera_rays_ref(g, frame, n):
    """the samples 0 .. n-1 of every pixel of g as PathRef.trace takes them: (start, dir), entry [y, x, i]"""
    W, H = g.xRes, g.yRes
    nb = (n + 7) // 8
    start, ray = G.or_primary_ray(g, frame, 0, nb * W * H * 8)
    i, y, x = np.meshgrid(np.arange(n), np.arange(H), np.arange(W), indexing="ij")
    r = (((i // 8) * W * H + y * W + x) * 8 + i % 8).transpose(1, 2, 0).reshape(-1)
    return start.reshape(-1, 3)[r].copy(), ray.reshape(-1, 3)[r].copy()


def followed(end, segments):
    """the segments a path followed beyond the first as dt_features_path_kernel counts them: a bounce counts when
    the rule says go, also where its successor is a void ray that is never traced"""
    end, segments = np.asarray(end), np.asarray(segments)
    return np.maximum(segments - 1, 0) + ((end == VOID) & (segments >= 1))


class RayPathRef:
    def __init__(self, built, g):
        self.pr = PathRef(built, g)
        self.g = g
        desc = self.pr.desc
        self.mat = np.array([desc.shapes[k].material for k in range(desc.n_shapes)])
        self.flg = np.array([desc.shapes[k].flags for k in range(desc.n_shapes)], np.int64)

    def trace(self, start, dir, K, normal=True, albedo=True):
        """(planes, counters, log) at max_bounces = K. normal, albedo: whether those planes are wanted (their
        counters belong to them; the normal is computed at every hit with k < K regardless)"""
        start = np.array(start, np.float64).reshape(-1, 3)
        dir = np.array(dir, np.float64).reshape(-1, 3)
        n = len(start)
        out = {"end": np.full(n, VOID, np.int32), "segments": np.zeros(n, np.int32), "shape": np.full(n, -1, np.int32),
               "length": np.zeros(n), "point": np.zeros((n, 3)), "normal": np.zeros((n, 3)), "albedo": np.zeros((n, 3)),
               "last_start": np.zeros((n, 3)), "last_dir": np.zeros((n, 3)),
               "seg_shape": np.full((n, K + 1), -1, np.int32), "seg_point": np.zeros((n, K + 1, 3))}
        cnt = dict.fromkeys(COUNTERS, 0)
        log = []
        at, s, d = np.arange(n), start, dir   # the rays still travelling
        for k in range(K + 1):
            if at.size == 0:
                break
            seg = self.pr._segment(s, d)
            tr, hit = seg["traced"], seg["hit"]
            cnt["rays"] += int(tr.sum())
            a = at[tr]
            out["segments"][a] = k + 1
            out["last_start"][a], out["last_dir"][a] = s[tr], d[tr]
            out["seg_shape"][a, k] = np.where(hit[tr], seg["shape"][tr], -1)
            out["seg_point"][a, k] = np.where(hit[tr][:, None], seg["p"][tr], 0.0)
            out["end"][at[tr & ~hit]] = MISS
            out["length"][at[hit]] = out["length"][at[hit]] + seg["len"][hit]
            if k < K or normal:
                cnt["prism_norm_fallback"] += int(seg["prism"][hit].sum())
            hs = np.where(hit, seg["shape"], 0)
            rule = bounce_rule(self.g, self.mat[hs], self.flg[hs], seg["inside"], seg["in"], seg["n"], seg["p"])
            goes = hit & (rule["code"] != STOP) if k < K else np.zeros(len(at), bool)
            if k < K:
                cnt["reflect_errors"] += int((hit & rule["refl_err"]).sum())
            ends = hit & ~goes
            e = at[ends]
            out["end"][e] = SURFACE if k < K else CUT
            out["shape"][e], out["point"][e] = seg["shape"][ends], seg["p"][ends]
            if normal:
                out["normal"][e] = seg["n"][ends]
            if albedo:
                out["albedo"][e] = seg["col"][ends]
                cnt["tex_fetches"] += int(seg["tex"][ends].sum())
                cnt["uv_out_of_range"] += int(seg["uv"][ends].sum())
            log.append({"ray": at, "seg": seg, "rule": rule, "goes": goes, "evaluated": k < K,
                        "material": np.where(hit, self.mat[hs], -1)})
            at, s, d = at[goes], rule["start"][goes], rule["dir"][goes]   # end stays VOID until a segment is traced
        return out, cnt, log


@functools.lru_cache(maxsize=None)
def ray_set():
    """the rays of tests/test_gpu_raypath.py on the unit scene: sample 0 of every other pixel (64 * 3 camera rays),
    then the 17 hand-made ones: 64 * 3 + 17 rays, a partial last wave. (start, dir, {name: indices})"""
    desc, g, keep = unit_scene()
    cs, cd = camera_rays_ref(g, 0, 1)
    hs, hd, names = hand_made_rays()
    cs, cd = cs[::2], cd[::2]
    assert len(cs) == 64 * 3 and len(hs) == 17
    return np.concatenate([cs, hs]), np.concatenate([cd, hd]), {k: v + len(cs) for k, v in names.items()}


@functools.lru_cache(maxsize=None)
def unit_ref():
    desc, g, keep = unit_scene()
    return RayPathRef(desc, g), desc, g, keep


@functools.lru_cache(maxsize=None)
def prediction(K, normal=True, albedo=True):
    """(planes, counters, log) of ray_set() at max_bounces = K; computed once, shared, not to be written to"""
    s, d, _ = ray_set()
    return unit_ref()[0].trace(s, d, K, normal=normal, albedo=albedo)


def codes_seen(log):
    """the rule's answers over the hits where it was evaluated"""
    seen = set()
    for rec in log:
        if rec["evaluated"]:
            seen |= set(rec["rule"]["code"][rec["seg"]["hit"]].tolist())
    return seen


__all__ = ["RayPathRef", "camera_rays_ref", "followed", "codes_seen", "PLANES", "COUNTERS", "VOID", "MISS", "SURFACE",
           "CUT", "REFLECT", "REFRACT", "STOP"]
