"""The prediction of the mutual visibility of two point sets (include/dt.h dt_points_visibility), composed in numpy
from tests/rayquery_ref.py RayQueryRef.occluded (every pair answered as dt_rays_occluded answers the ray a_i,
b_j - a_i, skip_b[j]: the oracle's answer) and the cosine restatement of tests/points_irradiance_ref.py (the host
export dt_irradiance_cosine), in the header's order: per tile of TILE targets the f64 sum in ascending j from 0.0,
then the tile sums in ascending tile order from 0.0.

VisibilityRef answers every pair of a case once and keeps the per-pair terms; a pair depends on nothing else, so
planes(cols=...) of a range of targets is the prediction of a call on those targets alone (its tiles count from
the range's first target). scene() is the test scene, case() its point sets, classes() what the sets exercise, by
the restatement alone. A helper, not collected by pytest."""
import functools

import numpy as np

import scene_gen
from points_irradiance_ref import cosine
from rayquery_ref import RayQueryRef, void_rays

TILE = 256
N_A, N_B = 64 * 2 + 7, 256 + 37
NAN_A, NAN_B = 64 + 32, 100          # the void source (the middle of the second wave) and the void target
SAME_A, SAME_B = 10, 290             # b[SAME_B] == a[SAME_A]: the void-ray pair
PLANES = ("bits", "count_a", "count_b", "weight_a")


def scene():
    """A floor, a free-standing wall between most sources and the targets, a sphere, and the rectangle the targets
    lie on (x = 4, facing -x): (desc, g, keepalive, the rectangle's shape index)"""
    b = scene_gen._Builder(1.0, (0.0, 0.0, 0.0))
    scene_gen._rect(b, (-6, 0, 6), (6, 0, 6), (6, 0, -6), (-6, 0, -6), (0.5, 0.5, 0.5), flags=0)           # floor
    scene_gen._rect(b, (1, 0, -3), (1, 0, 0.5), (1, 1.25, 0.5), (1, 1.25, -3), (0.8, 0.3, 0.2), flags=0)   # wall
    b.shape(scene_gen.SPHERE, v=[(2.5, 1.0, 1.5)], radius=0.75, color=(0.2, 0.4, 0.9), center=(2.5, 1.0, 1.5))
    panel = scene_gen._rect(b, (4, 0.5, -3), (4, 0.5, 3), (4, 3.5, 3), (4, 3.5, -3), (0.9, 0.9, 0.9), flags=0)
    b.light(scene_gen.POINT_LIGHT, center=(0, 5, 0), color=(0.8, 0.8, 0.8))
    g = b.globals((-5.0, 2.0, 5.0), (2.0, 1.0, 0.0), 0.0, 6.0)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth, g.brdf_samples = 32, 16, 1, 2, 1
    desc, keep = b.desc()
    return desc, g, keep, panel


@functools.lru_cache(maxsize=None)
def case():
    """(a, normal_a, b, normal_b, skip_b, desc, g, keep, panel), read-only. Sources: 120 sensors a quarter above the
    floor in front of the wall, row by row (neighbours in the array are neighbours in space), then 15 behind the
    panel; targets: 280 texel centres of the panel, then 13 floating half a unit in front of it with no skip shape."""
    desc, g, keep, panel = scene()
    a = np.zeros((N_A, 3))
    for k in range(120):
        ix, iz = k % 15, k // 15
        a[k] = (-4.0 + 0.35 * ix, 0.25, -2.8 + 0.8 * iz)
    for k in range(120, N_A):
        a[k] = (5.0, 0.75 + 0.125 * (k - 120), -2.1 + 0.3 * (k - 120))
    na = np.tile([0.0, 1.0, 0.0], (N_A, 1))
    na[120:] = (-1.0, 0.0, 0.0)
    b = np.zeros((N_B, 3))
    for k in range(280):
        iz, iy = k % 20, k // 20
        b[k] = (4.0, 0.5 + (iy + 0.5) * (3.0 / 14.0), -3.0 + (iz + 0.5) * 0.3)
    for k in range(280, N_B):
        b[k] = (3.5, 0.75 + 0.2 * (k - 280), -2.4 + 0.4 * (k - 280))
    nb = np.tile([-1.0, 0.0, 0.0], (N_B, 1))
    skip = np.full(N_B, panel, np.int32)
    skip[280:] = -1
    a[NAN_A, 1] = np.nan
    b[NAN_B, 2] = np.nan
    b[SAME_B] = a[SAME_A]
    for arr in (a, na, b, nb, skip):
        arr.setflags(write=False)
    return a, na, b, nb, skip, desc, g, keep, panel


def pairs(a, b):
    """the materialised segments, source-major: (start, dir) of pair (i, j) at row i * n_b + j"""
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    start = np.repeat(a, len(b), axis=0)
    with np.errstate(all="ignore"):
        return start, np.tile(b, (len(a), 1)) - start


def pack(vis):
    """the bits plane of a bool (n_a, n_b) matrix: bit (j & 31) of word j >> 5 of row i"""
    n_a, n_b = vis.shape
    words = (n_b + 31) // 32
    padded = np.zeros((n_a, words * 32), np.uint64)
    padded[:, :n_b] = vis
    w = (padded.reshape(n_a, words, 32) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2)
    return w.astype(np.uint32)


class VisibilityRef:
    def __init__(self, built, g, a, b, skip_b=None, normal_a=None, normal_b=None, rq=None):
        self.rq = rq if rq is not None else RayQueryRef(built, g)
        a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
        self.n_a, self.n_b = len(a), len(b)
        self.live_a, self.live_b = np.isfinite(a).all(axis=1), np.isfinite(b).all(axis=1)
        self.have_normals = normal_a is not None and normal_b is not None
        shape = (self.n_a, self.n_b)
        start, dir = pairs(a, b)
        both = (self.live_a[:, None] & self.live_b[None, :]).reshape(-1)
        self.traced = (both & ~void_rays(start, dir)).reshape(shape)
        skip = None if skip_b is None else np.tile(np.asarray(skip_b, np.int32), self.n_a)
        at = np.nonzero(self.traced.reshape(-1))[0]
        occ = np.zeros(len(start), np.uint8)
        occ[at] = self.rq.occluded(start[at], dir[at], None if skip is None else skip[at])
        # a void ray between two live points is reported as not occluded: visible
        self.vis_points = both.reshape(shape) & (occ.reshape(shape) == 0)
        self.term = None
        if self.have_normals:
            normal_a = np.asarray(normal_a, np.float64).reshape(-1, 3)
            normal_b = np.asarray(normal_b, np.float64).reshape(-1, 3)
            self.norm_a, self.norm_b = np.isfinite(normal_a).all(axis=1), np.isfinite(normal_b).all(axis=1)
            d = dir[at]
            ca = cosine(np.repeat(normal_a, self.n_b, axis=0)[at], d)
            cb = cosine(np.tile(normal_b, (self.n_a, 1))[at], -d)
            cc = np.zeros(len(start))
            dd = np.ones(len(start))
            with np.errstate(all="ignore"):
                cc[at] = ca * cb
                dd[at] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            self.term = (cc.reshape(shape), dd.reshape(shape))

    def planes(self, falloff=0, want=PLANES, cols=None):
        """({plane: array} for the planes of `want`, the pairs traced) of the targets cols (a slice; None: all).
        With weight_a wanted a point whose normal has a non-finite component is void as well."""
        cols = slice(0, self.n_b) if cols is None else cols
        vis, traced = self.vis_points[:, cols].copy(), self.traced[:, cols].copy()
        if "weight_a" in want:
            assert self.have_normals
            ok = self.norm_a[:, None] & self.norm_b[None, cols]
            vis &= ok
            traced &= ok
        out = {}
        if "bits" in want:
            out["bits"] = pack(vis)
        if "count_a" in want:
            out["count_a"] = vis.sum(axis=1).astype(np.int32)
        if "count_b" in want:
            out["count_b"] = vis.sum(axis=0).astype(np.int32)
        if "weight_a" in want:
            cc, dd = self.term[0][:, cols], self.term[1][:, cols]
            with np.errstate(all="ignore"):
                w = np.where(vis & traced, cc / dd if falloff else cc, 0.0)
            total = np.zeros(self.n_a)
            for t0 in range(0, vis.shape[1], TILE):   # the tile sums in ascending tile order, from 0.0
                s = np.zeros(self.n_a)
                for j in range(t0, min(t0 + TILE, vis.shape[1])):   # ascending j, from 0.0
                    s = s + w[:, j]
                total = total + s
            out["weight_a"] = total
        return out, int(traced.sum())


@functools.lru_cache(maxsize=None)
def reference():
    """the prediction of case(), and the same pairs answered with no skip shape and with the panel skipped for every
    target (classes() only): computed once, never written to"""
    a, na, b, nb, skip, desc, g, keep, panel = case()
    ref = VisibilityRef(desc, g, a, b, skip, na, nb)
    none = VisibilityRef(desc, g, a, b, None, rq=ref.rq)
    allp = VisibilityRef(desc, g, a, b, np.full(N_B, panel, np.int32), rq=ref.rq)
    return ref, none, allp


def classes():
    """what case() exercises, from the restatement alone: name -> count (or share)"""
    a, na, b, nb, skip, desc, g, keep, panel = case()
    ref, none, allp = reference()
    live = ref.live_a[:, None] & ref.live_b[None, :]
    vis = ref.vis_points
    words = pack(vis)
    full = (1 << 32) - 1
    w0, _ = ref.planes(0, want=("weight_a",))
    w1, _ = ref.planes(1, want=("weight_a",))
    t0, _ = ref.planes(0, want=("weight_a",), cols=slice(0, TILE))
    t1, _ = ref.planes(0, want=("weight_a",), cols=slice(TILE, N_B))
    return {
        "live_pairs": int(live.sum()),
        "visible": int((vis & live).sum()),
        "hidden": int((~vis & live).sum()),
        "hidden_only_without_skip": int((live & ~vis & allp.vis_points & (skip == -1)[None, :]).sum()),
        "visible_only_with_skip": int((live & vis & ~none.vis_points & (skip >= 0)[None, :]).sum()),
        "mixed_words": int(((words[:, :N_B // 32] != 0) & (words[:, :N_B // 32] != full)).sum()),
        "void_sources": int((~ref.live_a).sum()),
        "void_targets": int((~ref.live_b).sum()),
        "void_ray_pairs": int((live & ~ref.traced).sum()),
        "void_ray_pair_visible": bool(vis[SAME_A, SAME_B] and not ref.traced[SAME_A, SAME_B]),
        "weight_in_both_tiles": int(((t0["weight_a"] > 0) & (t1["weight_a"] > 0)).sum()),
        "falloff_changes_weight": int((w0["weight_a"] != w1["weight_a"]).sum()),
    }
