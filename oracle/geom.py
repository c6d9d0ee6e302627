"""TEST INFRASTRUCTURE ONLY -- the geometry.cpp parity vectors: what is drawn, how a backend answers, how
answers compare. Two backends answer the same questions about a flat shape record (ShapeDesc):

  Ref     the reference's geometry.cpp, compiled unmodified against oracle/ref/eigen_shim
          (oracle/_ref/libref_geom.so, oracle/ref/geom_harness.cpp); absent where the reference is
  Oracle  oracle/oracle.c through its test-only or_shape_* / or_box_* entry points

tools/gen_golden_geom.py draws the vectors (draw), lets Ref answer them (evaluate) and writes
tests/golden/geom_ref.npz; tests/test_oracle_geom.py lets Oracle answer the stored vectors and compares
bit patterns (mismatches). The fixture holds data only: shape records, rays, points, answers."""
import ctypes
import os

import numpy as np

from distraytracer_amd._lib import Globals, LightDesc, SceneDesc, ShapeDesc

from . import HERE, oracle

REF_GEOM_SO = os.path.join(HERE, "_ref", "libref_geom.so")
SHAPE_DT = np.dtype(ShapeDesc)
GLOBALS_DT = np.dtype(Globals)
T_INIT = np.float32(-7.0)    # *t before a call: what stays where the method leaves t unwritten
FLT_MAX = np.float32(3.4028234663852886e38)
F_MESH, F_UV = 1 << 5, 1 << 6

P = ctypes.POINTER
_D = P(ctypes.c_double)


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_D)


def shapes_from_records(rec):
    """structured array (SHAPE_DT) -> ctypes array of ShapeDesc"""
    rec = np.ascontiguousarray(rec, dtype=SHAPE_DT)
    arr = (ShapeDesc * max(len(rec), 1))()
    ctypes.memmove(arr, rec.ctypes.data, rec.nbytes)
    return arr


def records_from_shapes(shapes):
    arr = (ShapeDesc * len(shapes))(*shapes)
    return np.frombuffer(bytes(arr), dtype=SHAPE_DT).copy()


def records_from_desc(desc):
    """(shape records, hole records) of a dt_scene_desc, e.g. one a scene builder made"""
    def grab(ptr, n):
        if n <= 0:
            return np.zeros(0, dtype=SHAPE_DT)
        return np.frombuffer(ctypes.string_at(ptr, n * ctypes.sizeof(ShapeDesc)), dtype=SHAPE_DT).copy()
    return grab(desc.shapes, desc.n_shapes), grab(desc.holes, desc.n_holes)


# scene builders whose constructor-derived members (center, length, width: host_scenes.cpp) are compared
# with the reference's constructors: (builder, frame, use_model)
BUILDER_SCENES = [("final", 240, 0), ("final", 240, 1), ("final", 1200, 0), ("prismcyl", 30, 0), ("hw4", 0, 0),
                  ("spheres", 0, 0), ("dof", 0, 0)]
BUILDER_PER_TYPE = 8      # shapes of each type taken from each scene, evenly spaced over its shapes


def builder_sample(dt, scene, frame, use_model):
    """(built scene, shape records, hole records, indices of the sampled shapes)"""
    g = dt.globals_default()
    g.use_model = use_model
    built = dt.build_scene(scene, frame, g)
    rec, hrec = records_from_desc(built.desc)
    idx = []
    for t in np.unique(rec["type"]):
        of_t = np.nonzero(rec["type"] == t)[0]
        idx += list(of_t[np.unique(np.linspace(0, len(of_t) - 1, BUILDER_PER_TYPE).astype(int))])
    return built, rec, hrec, np.array(sorted(idx), dtype=np.int32)


def scene_desc(shapes, holes, lights=None, n_shapes=None):
    """(SceneDesc, keepalive) over ctypes arrays"""
    n = len(shapes) if n_shapes is None else n_shapes
    d = SceneDesc(n, 0 if lights is None else len(lights), 0, 0, shapes, lights, None,
                  0 if holes is None else len(holes), 0, holes)
    return d, (shapes, holes, lights)


class Oracle:
    name = "oracle"

    def __init__(self, shape_rec, hole_rec):
        self.o = o = oracle()
        self.shapes = shapes_from_records(shape_rec)
        self.holes = shapes_from_records(hole_rec)
        self.d, self._keep = scene_desc(self.shapes, self.holes, n_shapes=len(shape_rec))
        self.d.n_holes = len(hole_rec)
        self.dp = ctypes.pointer(self.d)
        pf, pi = P(ctypes.c_float), P(ctypes.c_int)
        S = [P(SceneDesc), ctypes.c_int]
        o.or_shape_intersect.argtypes = S + [_D, _D, pf, pi, pi]
        o.or_shape_color_after_hit.argtypes = S + [_D, _D, _D]
        o.or_shape_shadow.argtypes = S + [_D, _D, ctypes.c_float]
        o.or_shape_intersect_cap.argtypes = S + [_D, _D, pf, pi]
        o.or_shape_norm.argtypes = S + [_D, ctypes.c_int, _D]
        o.or_shape_uv.argtypes = S + [_D, _D]
        o.or_shape_bounds.argtypes = S + [_D, _D]
        o.or_shape_bounds.restype = None
        o.or_checker_cyl_objM.argtypes = S + [_D]
        o.or_checker_cyl_objM.restype = None
        o.or_box_intersect.argtypes = S + [ctypes.c_int, _D, _D, _D, _D, _D]
        o.or_fix_norm.argtypes = [_D] * 3
        o.or_fix_norm.restype = None
        o.or_barycentric3d.argtypes = [_D] * 5
        o.or_barycentric3d.restype = None
        o.or_segment_intersect.argtypes = [_D] * 4

    def intersect(self, si, ray, start):
        (_, r), (_, s) = _d(ray), _d(start)
        t, ins, hole = ctypes.c_float(T_INIT), ctypes.c_int(0), ctypes.c_int(-1)
        hit = self.o.or_shape_intersect(self.dp, si, r, s, ctypes.byref(t), ctypes.byref(ins), ctypes.byref(hole))
        # the hole whose body is the hit: only a RectPrismWithCylinder that was hit names one
        sh = self.shapes[si]
        assert hole.value == -1 or (hit and sh.type == 9 and 0 <= hole.value < sh.n_holes), (si, hole.value)
        self.last_hole = hole.value
        col, cp = _d(np.zeros(3))
        self.o.or_shape_color_after_hit(self.dp, si, r, s, cp)
        return hit, np.float32(t.value), ins.value, col

    def shadow(self, si, ray, start, t_max):
        return self.o.or_shape_shadow(self.dp, si, _d(ray)[1], _d(start)[1], ctypes.c_float(t_max))

    def cap(self, si, ray, start):
        t, ins = ctypes.c_float(T_INIT), ctypes.c_int(0)
        hit = self.o.or_shape_intersect_cap(self.dp, si, _d(ray)[1], _d(start)[1], ctypes.byref(t), ctypes.byref(ins))
        return hit, np.float32(t.value), ins.value

    def norm(self, si, p, pre_ray=None, pre_start=None):
        """(normal, last_hit, threw): the closest-hit normal as the render loop takes it: after an
        intersect (pre_ray) with the hole index that intersect reported, else with hole = -1. The hole
        only matters past the three face tests, where the reference throws (threw = 1)."""
        out, op = _d(np.zeros(3))
        hole = -1
        if pre_ray is not None:
            self.intersect(si, pre_ray, pre_start)
            hole = self.last_hole
        fb = self.o.or_shape_norm(self.dp, si, _d(p)[1], hole, op)
        return out, -1, int(fb > 0 and self.shapes[si].type == 9)

    def uv(self, si, p):
        out, op = _d(np.zeros(2))
        valid = self.o.or_shape_uv(self.dp, si, _d(p)[1], op)
        return out, valid

    def bounds(self, si):
        (lb, lp), (ub, up) = _d(np.zeros(3)), _d(np.zeros(3))
        self.o.or_shape_bounds(self.dp, si, lp, up)
        return lb, ub

    def objM(self, si):
        out, op = _d(np.zeros(16))
        self.o.or_checker_cyl_objM(self.dp, si, op)
        return out

    def box(self, si, leaf, ray=None, inv_ray=None, start=None):
        (lb, lp), (ub, up) = _d(np.zeros(3)), _d(np.zeros(3))
        if ray is None:
            r = self.o.or_box_intersect(self.dp, si, leaf, None, None, None, lp, up)
        else:
            r = self.o.or_box_intersect(self.dp, si, leaf, _d(ray)[1], _d(inv_ray)[1], _d(start)[1], lp, up)
        return r, lb, ub

    def fix_norm(self, ray, nrm):
        out, op = _d(np.zeros(3))
        self.o.or_fix_norm(_d(ray)[1], _d(nrm)[1], op)
        return out

    def bary(self, p, A, B, C):
        out, op = _d(np.zeros(3))
        self.o.or_barycentric3d(_d(p)[1], _d(A)[1], _d(B)[1], _d(C)[1], op)
        return out

    def segment(self, A, B, ray, origin):
        return self.o.or_segment_intersect(_d(A)[1], _d(B)[1], _d(ray)[1], _d(origin)[1])


class Ref:
    name = "reference"

    @staticmethod
    def available():
        return os.path.exists(REF_GEOM_SO)

    def __init__(self, shape_rec, hole_rec):
        self.r = r = ctypes.CDLL(REF_GEOM_SO)
        self.shapes = shapes_from_records(shape_rec)
        self.holes = shapes_from_records(hole_rec)
        pf, pi, S = P(ctypes.c_float), P(ctypes.c_int), P(ShapeDesc)
        r.ref_intersect.argtypes = [S, S, _D, _D, pf, pi, _D, pi]
        r.ref_shadow.argtypes = [S, S, _D, _D, ctypes.c_float]
        r.ref_intersect_max.argtypes = [S, _D, _D, pf]
        r.ref_intersect_cap.argtypes = [S, _D, _D, pf, pi]
        r.ref_norm.argtypes = [S, S, _D, _D, _D, _D, pi]
        r.ref_bounds.argtypes = [S, S, _D, _D]
        r.ref_bounds.restype = None
        r.ref_uv.argtypes = [S, S, _D, _D, pi]
        r.ref_derived.argtypes = [S, S, _D, _D, pf, _D]
        r.ref_derived.restype = None
        r.ref_fix_norm.argtypes = [_D] * 3
        r.ref_fix_norm.restype = None
        r.ref_build_cob.argtypes = [_D] * 2
        r.ref_build_cob.restype = None
        r.ref_barycentric3d.argtypes = [_D] * 5
        r.ref_barycentric3d.restype = None
        r.ref_shortest_line.argtypes = [_D] * 4 + [pf, pf]
        r.ref_shortest_line.restype = None
        r.ref_segment_intersect.argtypes = [_D] * 4 + [pf]
        r.ref_line_intersect.argtypes = [_D] * 4 + [pf]
        r.ref_box.argtypes = [S, S, ctypes.c_int, _D, _D, _D, _D, _D]

    def _s(self, si):
        return ctypes.pointer(self.shapes[si])

    def intersect(self, si, ray, start):
        t, ins, lh = ctypes.c_float(T_INIT), ctypes.c_int(0), ctypes.c_int(-1)
        col, cp = _d(np.zeros(3))
        hit = self.r.ref_intersect(self._s(si), self.holes, _d(ray)[1], _d(start)[1], ctypes.byref(t),
                                   ctypes.byref(ins), cp, ctypes.byref(lh))
        return hit, np.float32(t.value), ins.value, col

    def shadow(self, si, ray, start, t_max):
        return self.r.ref_shadow(self._s(si), self.holes, _d(ray)[1], _d(start)[1], ctypes.c_float(t_max))

    def intersect_max(self, si, ray, start):
        t = ctypes.c_float(T_INIT)
        hit = self.r.ref_intersect_max(self._s(si), _d(ray)[1], _d(start)[1], ctypes.byref(t))
        return hit, np.float32(t.value)

    def cap(self, si, ray, start):
        t, ins = ctypes.c_float(T_INIT), ctypes.c_int(0)
        hit = self.r.ref_intersect_cap(self._s(si), _d(ray)[1], _d(start)[1], ctypes.byref(t), ctypes.byref(ins))
        return hit, np.float32(t.value), ins.value

    def norm(self, si, p, pre_ray=None, pre_start=None):
        out, op = _d(np.zeros(3))
        lh = ctypes.c_int(-1)
        pr = _d(pre_ray)[1] if pre_ray is not None else None
        ps = _d(pre_start)[1] if pre_start is not None else None
        threw = self.r.ref_norm(self._s(si), self.holes, _d(p)[1], pr, ps, op, ctypes.byref(lh))
        return out, lh.value, threw

    def uv(self, si, p):
        out, op = _d(np.zeros(2))
        valid = ctypes.c_int(-1)
        if self.r.ref_uv(self._s(si), self.holes, _d(p)[1], op, ctypes.byref(valid)):
            raise RuntimeError("reference getUV threw")
        return out, valid.value

    def bounds(self, si):
        (lb, lp), (ub, up) = _d(np.zeros(3)), _d(np.zeros(3))
        self.r.ref_bounds(self._s(si), self.holes, lp, up)
        return lb, ub

    def derived(self, si):
        """center[3], axis[3], (length, width, height, radius) float32, objM[16]"""
        (c, cp), (a, ap), (m, mp) = _d(np.zeros(3)), _d(np.zeros(3)), _d(np.zeros(16))
        f = np.zeros(4, dtype=np.float32)
        self.r.ref_derived(self._s(si), self.holes, cp, ap, f.ctypes.data_as(P(ctypes.c_float)), mp)
        return c, a, f, m

    def objM(self, si):
        return self.derived(si)[3]

    def box(self, si, leaf, ray=None, inv_ray=None, start=None):
        (lb, lp), (ub, up) = _d(np.zeros(3)), _d(np.zeros(3))
        if ray is None:
            r = self.r.ref_box(self._s(si), self.holes, leaf, None, None, None, lp, up)
        else:
            r = self.r.ref_box(self._s(si), self.holes, leaf, _d(ray)[1], _d(inv_ray)[1], _d(start)[1], lp, up)
        return r, lb, ub

    def fix_norm(self, ray, nrm):
        out, op = _d(np.zeros(3))
        self.r.ref_fix_norm(_d(ray)[1], _d(nrm)[1], op)
        return out

    def build_cob(self, z):
        out, op = _d(np.zeros(16))
        self.r.ref_build_cob(_d(z)[1], op)
        return out

    def bary(self, p, A, B, C):
        out, op = _d(np.zeros(3))
        self.r.ref_barycentric3d(_d(p)[1], _d(A)[1], _d(B)[1], _d(C)[1], op)
        return out

    def shortest_line(self, P1, P2, P3, P4):
        u = (ctypes.c_float(T_INIT), ctypes.c_float(T_INIT))
        self.r.ref_shortest_line(_d(P1)[1], _d(P2)[1], _d(P3)[1], _d(P4)[1], ctypes.byref(u[0]), ctypes.byref(u[1]))
        return np.float32(u[0].value), np.float32(u[1].value)

    def segment(self, A, B, ray, origin):
        t = ctypes.c_float(T_INIT)
        return self.r.ref_segment_intersect(_d(A)[1], _d(B)[1], _d(ray)[1], _d(origin)[1], ctypes.byref(t))

    def line(self, l1, o1, l2, o2):
        t = ctypes.c_float(T_INIT)
        return self.r.ref_line_intersect(_d(l1)[1], _d(o1)[1], _d(l2)[1], _d(o2)[1], ctypes.byref(t))


# ---------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------
def _shape(t, v, **kw):
    s = ShapeDesc()
    s.type = t
    s.tex_frame = -1
    for i, p in enumerate(v):
        for a in range(3):
            s.v[i][a] = float(p[a])
    for k, val in kw.items():
        if k == "uv":
            for i in range(3):
                for a in range(2):
                    s.uv[i][a] = val[i][a]
        elif isinstance(val, (list, tuple, np.ndarray)):
            for a in range(len(val)):
                getattr(s, k)[a] = float(val[a])
        else:
            setattr(s, k, val)
    return s


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _box(lo, hi, R=None, c=None):
    """A..H of geometry.cpp's prisms: ABCD the top face, E..H under A..D"""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = np.array([(x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0),
                  (x0, y0, z1), (x1, y0, z1), (x1, y0, z0), (x0, y0, z0)], dtype=np.float64)
    if R is not None:
        c = v.mean(0) if c is None else np.asarray(c)
        v = (v - c) @ R.T + c
    return v


def make_shapes():
    """The shapes of the fixture (names, ShapeDesc list, hole list): every dt_shape_type, each
    axis-aligned with dyadic coordinates (exact edge and vertex hits) and once oblique."""
    R1 = _rot((1, 2, 0.5), 0.7)
    rect0 = [(-1, -1, -4), (1, -1, -4), (1, 0.5, -4), (-1, 0.5, -4)]
    rect1 = (np.array(rect0) - (0, 0, -4)) @ R1.T + (0.3, 0.1, -4.2)
    floor = [(-2, -1, -2), (2, -1, -2), (2, -1, -6), (-2, -1, -6)]
    hole = [(-0.5, -1, -3.5), (0.75, -1, -3.5), (0.75, -1, -4.5), (-0.5, -1, -4.5)]
    col, c1, c2 = (0.8, 0.3, 0.2), (0.9, 0.9, 0.9), (0.1, 0.1, 0.3)
    names, shapes = [], []

    def add(name, s):
        names.append(name)
        shapes.append(s)

    add("sphere", _shape(1, [(0.5, -0.25, -3)], radius=1.25, color=col))
    add("sphere_small", _shape(1, [(-0.731, 0.412, -2.377)], radius=0.37, color=col))
    add("cylinder_y", _shape(2, [(0, -1, -4), (0, 1, -4)], radius=0.5, color=col))
    add("cylinder_oblique", _shape(2, [(-1, 0.2, -5), (1.3, 0.9, -3.5)], radius=0.3, color=col))
    add("triangle", _shape(3, [(-1, -1, -3), (1, -1, -3), (0, 1, -3.5)], color=col))
    add("triangle_mesh_uv", _shape(3, [(-0.8, -0.6, -2.9), (0.9, -0.7, -3.6), (0.1, 0.8, -3.1)], color=col,
                                   flags=F_MESH | F_UV, mesh_normal=(0.2, 0.1, 1.0),
                                   uv=[(0.1, 0.2), (0.9, 0.15), (0.45, 0.95)]))
    add("rectangle", _shape(4, rect0, color=col))
    add("rectangle_oblique", _shape(4, rect1, color=col))
    add("prism", _shape(5, _box((-1, -1, -5), (1, 1, -3)), color=col))
    add("prism_oblique", _shape(5, _box((-0.7, -0.4, -4.6), (0.6, 0.5, -3.2), R1), color=col))
    add("checkerboard", _shape(6, floor, color=c1, color1=c1, color2=c2, S=0.5))
    add("checkerboard_hole", _shape(7, floor + hole, color=c1, color1=c1, color2=c2, S=1.0, borderwidth=0.1))
    add("checker_cylinder_y", _shape(8, [(0, -1, -4), (0, 1, -4)], radius=0.5, color=col, S=0.25,
                                     borderwidth=0.02))
    add("checker_cylinder_oblique", _shape(8, [(-1, 0.2, -5), (1.3, 0.9, -3.5)], radius=0.3, color=col, S=0.2,
                                           borderwidth=0.03))
    add("checker_cylinder_x", _shape(8, [(-1, 0.5, -4), (1, 0.5, -4)], radius=0.4, color=col, S=0.3,
                                     borderwidth=0.02))       # axis along x: buildCOB's second basis choice
    add("prism_cyl", _shape(9, _box((-1.5, -1, -5), (1.5, 1, -4)), color=col, hole_first=0, n_holes=2))
    holes = [_shape(2, [(-0.75, 0, -3.5), (-0.75, 0, -5.5)], radius=0.4, color=(0.2, 0.6, 0.9)),
             _shape(2, [(0.75, 0.25, -4.0), (0.75, 0.25, -5.0)], radius=0.3, color=(0.9, 0.6, 0.1))]
    return names, shapes, holes


def derive_fields(ref, shapes):
    """center / length / width of every record exactly as the reference's constructor computes them"""
    for si, s in enumerate(shapes):
        c, _, f, _ = ref.derived(si)
        for a in range(3):
            s.center[a] = c[a]
        if s.type in (4, 5, 6, 7, 9):
            s.length, s.width = float(f[0]), float(f[1])


# ---------------------------------------------------------------------------------------------------
# drawing the vectors
# ---------------------------------------------------------------------------------------------------
def _nxt(x, k=1):
    x = np.float64(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def _f32_next(t, up):
    return np.nextafter(np.float32(t), np.float32(np.inf if up else -np.inf))


def _bisect(f, a, b, emit, tag):
    """f(s) -> hashable outcome on s in [0,1]; a, b with different outcomes. Halve until the two ends are
    adjacent doubles; emit both ends and a few values further out (both sides of the threshold)."""
    fa = f(a)
    for _ in range(80):
        m = 0.5 * (a + b)
        if m == a or m == b:
            break
        if f(m) == fa:
            a = m
        else:
            b = m
    gap = abs(b - a)
    for s in (a, b, a - 3 * gap * np.sign(b - a), b + 3 * gap * np.sign(b - a),
              a - 1e-9 * np.sign(b - a), b + 1e-9 * np.sign(b - a)):
        emit(min(max(s, 0.0), 1.0), tag)


def draw(backend, shapes, holes, seed, n_random=40, n_bisect=10):
    """The input vectors, per function: {fn: {field: array}}. `backend` (the one that will answer) is
    asked where thresholds lie: starts on a surface come from its own t, and pairs of rays with
    different answers are bisected down to adjacent doubles."""
    rng = np.random.default_rng(seed)
    isect = {"shape": [], "ray": [], "start": [], "tag": []}
    shadow = {"shape": [], "ray": [], "start": [], "t_max": [], "tag": []}
    cap = {"shape": [], "ray": [], "start": []}
    norm = {"shape": [], "p": [], "pre": [], "pre_ray": [], "pre_start": []}
    uv = {"shape": [], "p": []}
    box = {"shape": [], "leaf": [], "ray": [], "start": []}

    def add_isect(si, ray, start, tag):
        isect["shape"].append(si)
        isect["ray"].append(np.array(ray, dtype=np.float64))
        isect["start"].append(np.array(start, dtype=np.float64))
        isect["tag"].append(tag)

    def add_shadow(si, ray, start, t_max, tag):
        shadow["shape"].append(si)
        shadow["ray"].append(np.array(ray, dtype=np.float64))
        shadow["start"].append(np.array(start, dtype=np.float64))
        shadow["t_max"].append(np.float32(t_max))
        shadow["tag"].append(tag)

    def add_norm(si, p, pre_ray=None, pre_start=None):
        norm["shape"].append(si)
        norm["p"].append(np.array(p, dtype=np.float64))
        norm["pre"].append(0 if pre_ray is None else 1)
        norm["pre_ray"].append(np.zeros(3) if pre_ray is None else np.array(pre_ray, dtype=np.float64))
        norm["pre_start"].append(np.zeros(3) if pre_start is None else np.array(pre_start, dtype=np.float64))

    def add_box(si, leaf, ray, start):
        box["shape"].append(si)
        box["leaf"].append(leaf)
        box["ray"].append(np.array(ray, dtype=np.float64))
        box["start"].append(np.array(start, dtype=np.float64))

    for si, s in enumerate(shapes):
        lb, ub = backend.bounds(si)
        c, R = 0.5 * (lb + ub), 0.5 * float(np.linalg.norm(ub - lb))
        has_uv = s.type in (4, 5, 7, 8, 9) or (s.type == 3 and s.flags & F_UV)
        rays = []
        # seeded rays toward the shape, unnormalized as the reference's primary rays are
        for k in range(n_random):
            start = c + rng.normal(size=3) * (2.5 * R) * rng.uniform(0.5, 1.5)
            target = c + rng.uniform(-1, 1, 3) * (ub - lb) * 0.62
            ray = (target - start) * rng.uniform(0.2, 4.0)
            rays.append((ray, start, 0))
        # the start inside the bounds, and rays that leave the shape behind them (negative roots)
        for k in range(6):
            rays.append((rng.normal(size=3), c + rng.uniform(-0.2, 0.2, 3) * (ub - lb), 1))
        for ray, start, _ in list(rays[:6]):
            rays.append((-ray, start, 2))
        # exactly-zero components: one, then two (cwiseInverse gives +-inf; the box tests' isinf branch)
        for ax in range(3):
            e = np.zeros(3)
            e[ax] = 1.0
            for sgn in (1.0, -1.0):
                for off in (np.zeros(3), rng.uniform(-0.45, 0.45, 3) * (ub - lb)):
                    rays.append((sgn * e * 1.5, c + off - sgn * e * 3 * R, 3))
            o1, o2 = (ax + 1) % 3, (ax + 2) % 3
            ray = np.zeros(3)
            ray[o1], ray[o2] = rng.uniform(0.3, 1), -rng.uniform(0.3, 1)
            tgt = c + rng.uniform(-0.3, 0.3, 3) * (ub - lb)
            rays.append((ray, tgt - 2.5 * R * ray, 3))
            rays.append((ray, np.where(np.arange(3) == ax, lb, tgt - 2.5 * R * ray), 3))   # start on a bound
        # the shape's own deliberate cases
        rays += _special_rays(s, holes, lb, ub, rng)
        for ray, start, tag in rays:
            add_isect(si, ray, start, tag)
        # second pass: what the backend answered decides the surface starts, t_max values and bisections
        answers = [backend.intersect(si, r, st) for r, st, _ in rays]
        hits = [i for i, a in enumerate(answers) if a[0] and a[1] != T_INIT and np.isfinite(a[1])]
        for i in hits[:10]:
            ray, start, _ = rays[i]
            t = np.float64(answers[i][1])
            p = start + t * ray
            add_isect(si, ray, p, 4)                      # start on the surface, going on
            add_isect(si, -ray, p, 4)                     # ... and back out
            add_isect(si, rng.normal(size=3), p, 4)
            add_isect(si, ray, start + (t - 0.001) * ray, 4)   # the hit one eps ahead
            add_isect(si, ray, start + (t - 0.0001) * ray, 4)
        for i in hits[:14]:
            ray, start, _ = rays[i]
            t = answers[i][1]
            if i in hits[:8]:
                for tm in (_f32_next(t, False), t, _f32_next(t, True), FLT_MAX, np.float32(0.5) * t,
                           np.float32(1e-3), np.float32(1e-4)):
                    add_shadow(si, ray, start, tm, 5)
            p = start + np.float64(t) * ray
            add_norm(si, p)
            if s.type == 9:
                add_norm(si, p, ray, start)
            if has_uv:
                uv["shape"].append(si)
                uv["p"].append(p)
        for i in range(len(rays)):
            if i not in hits[:8] and (i % 3 == 0 or (rays[i][2] == 8 and s.type in (1, 2, 8))):
                add_shadow(si, rays[i][0], rays[i][1], FLT_MAX if i % 2 else np.float32(2.0), rays[i][2])
        # thresholds: pairs of rays with different answers, halved down to adjacent doubles
        key = [(a[0], a[2]) for a in answers]
        pairs = [(i, j) for i in range(len(rays)) for j in range(i + 1, len(rays)) if key[i] != key[j]]
        rng.shuffle(pairs)
        for i, j in pairs[:n_bisect]:
            (r0, s0, _), (r1, s1, _) = rays[i], rays[j]

            def at(x):
                return (1 - x) * r0 + x * r1, (1 - x) * s0 + x * s1

            def f(x):
                a = backend.intersect(si, *at(x))
                return (a[0], a[2])

            _bisect(f, 0.0, 1.0, lambda x, tag: add_isect(si, *at(x), tag), 6)
        # moving the start along a hitting ray through the surface: every eps on t, from both sides
        for i in hits[:n_bisect // 2]:
            ray, start, _ = rays[i]
            t = np.float64(answers[i][1])

            def at2(x):
                return ray, start + (t * (0.5 + x)) * ray

            def f2(x):
                a = backend.intersect(si, *at2(x))
                return (a[0], a[2])

            if f2(0.0) != f2(1.0):
                _bisect(f2, 0.0, 1.0, lambda x, tag: add_isect(si, *at2(x), tag), 7)

            if s.type in (1, 2, 8, 9):                       # ... and out through the far side
                p_in = start + (t * 1.01 + 1e-3) * ray
                a_in = backend.intersect(si, ray, p_in)
                if a_in[0] and a_in[2] and np.isfinite(a_in[1]):
                    far = 2.0 * np.float64(a_in[1])

                    def at4(x):
                        return ray, p_in + (far * x) * ray

                    def f4(x):
                        a = backend.intersect(si, *at4(x))
                        return (a[0], a[2])

                    if f4(0.0) != f4(1.0):
                        _bisect(f4, 0.0, 1.0, lambda x, tag: add_isect(si, *at4(x), tag), 7)

            def f3(x):
                return backend.shadow(si, ray, start + (t * (0.5 + x)) * ray, FLT_MAX)

            if f3(0.0) != f3(1.0):
                _bisect(f3, 0.0, 1.0, lambda x, tag: add_shadow(si, ray, start + (t * (0.5 + x)) * ray, FLT_MAX, tag), 7)
        if s.type in (2, 8):
            for ray, start, _ in rays[:n_random] + [r for r in rays if r[2] >= 3]:
                cap["shape"].append(si)
                cap["ray"].append(np.array(ray, dtype=np.float64))
                cap["start"].append(np.array(start, dtype=np.float64))
        # BoundingVolume over the shape: leaf and inner node, rays incl. the zero-component ones
        for i, (ray, start, tag) in enumerate(rays):
            if tag == 3 or i % 3 == 0:
                add_box(si, i % 2, ray, start)
        blb, bub = backend.box(si, 1)[1:]
        for ax in range(3):          # start exactly on / one ulp off a padded bound, ray along another axis
            e = np.zeros(3)
            e[(ax + 1) % 3] = 1.0
            for bound in (blb[ax], bub[ax]):
                for k in (-1, 0, 1):
                    st = c.copy()
                    st[ax] = _nxt(bound, k)
                    add_box(si, 1, e, st - 3 * R * e)
            out_ = np.zeros(3)                                # leaving through a bound it starts on: tmax == 0
            out_[ax] = 1.0
            for bound, sgn in ((bub[ax], 1.0), (blb[ax], -1.0)):
                for k in (-1, 0, 1):
                    st = c.copy()
                    st[ax] = _nxt(bound, k)
                    add_box(si, 1, sgn * out_ * 0.75, st)
                    skew = np.array([1e-3, -2e-3, 1.5e-3])    # ... with no zero component: the final tmax > 0
                    skew[ax] = sgn * 0.75
                    add_box(si, 1, skew, st)
        _special_points(s, si, lb, ub, rng, add_norm, uv)
    out = {"intersect": isect, "shadow": shadow, "cap": cap, "norm": norm, "uv": uv, "box": box}
    out.update(_free_function_cases(rng))
    return {fn: {k: np.array(v) for k, v in d.items()} for fn, d in out.items()}


def _special_rays(s, holes, lb, ub, rng):
    v = np.array([[s.v[i][a] for a in range(3)] for i in range(8)])
    t = s.type
    out = []
    down = np.array([0.0, 0.0, -1.0])
    if t == 1:
        cx, r = v[0], float(s.radius)
        out.append((rng.normal(size=3), cx, 8))                               # start at the centre
        for k in (-3, -1, 0, 1, 3):                                            # grazing: discriminant ~ 0
            out.append((np.array([0, 1.0, 0]), np.array([_nxt(cx[0] + r, k), cx[1] - 5, cx[2]]), 8))
            out.append((np.array([0, 0.37, 0]), np.array([cx[0] + r * (1 + k * 2e-8), cx[1] - 5, cx[2]]), 8))
        out.append((down * 2, cx + (0, 0, 4.0), 8))
    if t in (2, 8):
        c1, c2, r = v[0], v[1], float(s.radius)
        ax = c2 - c1
        for scale in (1.0, -0.4):                                              # parallel to the axis
            out.append((ax * scale, c1 - 1.5 * ax + (0.1 * r, 0, 0.05 * r), 8))  # inside the radius
            out.append((ax * scale, c1 - 1.5 * ax + (2 * r, 0, 0), 8))           # outside it
        side = np.cross(ax, (0.3, 0.2, 1.0))
        side /= np.linalg.norm(side)
        for h in (-0.05, 0.0, 1e-9, 0.5, 1.0, 1.02):                           # body against cap, cap rim
            out.append((-side, c1 + h * ax + 3 * r * side, 8))
        for k in (0.5, 0.999, 1.0, 1.001):                                     # through the cap plane
            out.append((ax, c1 - 0.8 * ax + k * r * side, 8))
        out.append((ax + 0.3 * side, c1 - 0.8 * ax, 8))
        # dyadic cases of an axis-aligned cylinder: unit vectors e, e2 exactly perpendicular to the axis
        units = [u for u in np.eye(3) if u.dot(ax) == 0]
        if len(units) == 2:
            e1, e2 = units
            for k in (-2, -1, 0, 1, 2):                                        # grazing: discriminant exactly 0
                out.append((-e1, c1 + 0.5 * ax + _nxt(r, k) * e2 + 4 * e1, 8))
            for cap_c in (c1, c2):
                for k in (-1, 0, 1):                                           # p exactly on a cap's plane (the rim)
                    off = (_nxt(1.0, k) - 1.0) * ax
                    out.append((-e1, cap_c + off + 4 * e1, 8))                 # ... from outside (near root)
                    out.append((-e1, cap_c + off, 8))                          # ... from the axis (far root)
                    out.append((-e1 * 0.5, cap_c + off + 0.25 * r * e2, 8))
        a = ax / np.linalg.norm(ax)
        e = np.float64(np.float32(1e-3))
        for k in (-2, -1, 0, 1, 2):                                            # a cap plane at t = eps exactly
            out.append((a, c1 - _nxt(e, k) * a, 8))
            out.append((-a, c2 + _nxt(e, k) * a, 8))
    if t == 3:
        A, B, C = v[0], v[1], v[2]
        for p in (A, B, C, 0.5 * (A + B), 0.5 * (B + C), 0.5 * (A + C), (A + B + C) / 3):   # vertices, edges
            out.append((down, p + (0, 0, 3.0), 8))
            out.append((down, np.array([_nxt(p[0] + 0, 1), _nxt(p[1], -1), p[2] + 3.0]), 8))
        out.append((B - A, A - 2 * (B - A), 8))                                # in the plane, along an edge
        out.append((C - A + 0.2 * (B - A), A - 0.5 * (C - A), 8))
        n = np.cross(B - A, C - A)
        for k in (0.99e-4, 1e-4, 1.01e-4):                                     # det against +-0.0001
            d = (B - A) + 0.3 * (C - A)
            out.append((d / np.linalg.norm(d) + n / n.dot(n) * k, (A + B + C) / 3 - d, 8))
    if t in (4, 6, 7):
        A, B, C, D = v[0], v[1], v[2], v[3]
        n = np.cross(B - A, C - A)
        n /= np.linalg.norm(n)
        for p in (A, B, C, D, 0.5 * (A + B), 0.5 * (B + C), 0.5 * (C + D), 0.5 * (A + D), 0.25 * (A + B + C + D)):
            out.append((-n, p + 3 * n, 8))
            out.append((-n * 0.7, p + 3 * n + (B - A) * 2e-16, 8))
            out.append((n, p - 2 * n, 8))
        out.append((B - A, A - 0.5 * (B - A), 8))                              # in the plane: along edge AB
        out.append((C - A, A - 0.25 * (C - A), 8))                             # ... along the diagonal
        out.append((B - A, 0.5 * (A + D) - 2 * (B - A), 8))                    # ... across, through AD and BC
        out.append((B - A, A + 2 * (D - A) - 2 * (B - A), 8))                  # ... beside the rectangle
        if t in (6, 7):
            S = float(s.S)
            u, w = (B - A) / np.linalg.norm(B - A), (D - A) / np.linalg.norm(D - A)
            for i in range(0, 5):                                              # checker square boundaries
                for k in (-1, 0, 1):
                    p = A + _nxt(i * S, k) * u + (0.3 * S + i * S) * w
                    out.append((-n, p + 2 * n, 8))
        if t == 7:
            H = v[4:8]
            for p in (H[0], H[1], 0.5 * (H[0] + H[1]), H.mean(0), H[0] - 0.01 * (H[1] - H[0])):   # the hole
                out.append((-n, p + 2 * n, 8))
                out.append((-n + 0.1 * (B - A), p + 2 * n - 0.2 * (B - A), 8))
    if t in (5, 9):
        ctr = v.mean(0)
        for i in range(8):                                                     # vertices, then edge midpoints
            out.append((down, v[i] + (0, 0, 4.0), 8))
            out.append((ctr - v[i], 2 * v[i] - ctr, 8))                        # along the diagonal, through the vertex
        for i, j in ((0, 1), (1, 2), (0, 4), (1, 5), (4, 5)):
            out.append((down, 0.5 * (v[i] + v[j]) + (0, 0, 4.0), 8))
            out.append((np.array([-1.0, 0, 0]), 0.5 * (v[i] + v[j]) + (4.0, 0, 0), 8))
        ctr = v.mean(0)
        for k in range(4):                                                     # the eye inside the prism
            out.append((rng.normal(size=3), ctr + rng.uniform(-0.2, 0.2, 3), 8))
    if t == 9:
        for h in holes[s.hole_first:s.hole_first + s.n_holes]:
            c1 = np.array([h.v[0][a] for a in range(3)])
            c2 = np.array([h.v[1][a] for a in range(3)])
            ax, r = c2 - c1, float(h.radius)
            for off in (0.0, 0.5, 0.99, 1.01, 1.5):                            # through the hole's front cap plane
                out.append((ax, c1 - 2 * ax + (off * r, 0, 0), 8))
                out.append((ax + (0.25, 0.1, 0), c1 - 2 * ax + (off * r, 0, 0), 8))
                out.append((-ax + (0.3, 0.05, 0), c2 + 2 * ax + (off * r, 0, 0), 8))
            out.append((np.array([1.0, 0.2, 0]), 0.5 * (c1 + c2), 8))          # from inside the hole
        for e in (0.5e-4, 0.99e-4, 1e-4, 1.01e-4, 2e-4):                       # |ray[i]| against eps = 1e-4
            for ax_ in range(3):
                ray = np.array([0.3, -0.2, -1.0])
                ray[ax_] = e
                out.append((ray, 0.5 * (lb + ub) - 3 * ray, 8))
                out.append((ray, np.where(np.arange(3) == ax_, ub + 0.5, 0.5 * (lb + ub) - 3 * ray), 8))
    return out


def _special_points(s, si, lb, ub, rng, add_norm, uv):
    v = np.array([[s.v[i][a] for a in range(3)] for i in range(8)])
    t = s.type

    def add_uv(p):
        uv["shape"].append(si)
        uv["p"].append(np.array(p, dtype=np.float64))

    if t == 5:
        ctr = v.mean(0)
        for p in list(v) + [0.5 * (v[0] + v[1]), 0.5 * (v[4] + v[6]), v[[0, 1, 2, 3]].mean(0), v[[0, 1, 5, 4]].mean(0),
                            v[[1, 2, 6, 5]].mean(0)]:
            add_norm(si, p)
            add_norm(si, p + rng.normal(size=3) * 2e-4)                        # the 1e-3 test on |cos|
            add_norm(si, p + (p - ctr) * 1.5e-3)
        add_norm(si, ctr + (0.31, 0.17, 0.23) * (ub - lb))                     # on no face: the fallback (prints)
        add_norm(si, ctr + (2.0, 1.3, -1.7) * (ub - lb))
    if t == 9:
        for p in (v[[0, 1, 2, 3]].mean(0), v[[4, 5, 6, 7]].mean(0), v[[0, 1, 5, 4]].mean(0), v[[3, 0, 4, 7]].mean(0),
                  v[[1, 2, 6, 5]].mean(0), v[0], v[6]):
            add_norm(si, p)
            add_uv(p)
    if t in (1, 2, 8):
        add_norm(si, 0.5 * (lb + ub) + (0.3, -0.2, 0.1))
    if t == 3 and s.flags & F_UV:
        A, B, C = v[0], v[1], v[2]
        for w in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, 0.5, 0), (1 / 3, 1 / 3, 1 / 3), (1.1, -0.05, -0.05),
                  (0.2, 0.9, -0.1)) + tuple(tuple(x) for x in rng.dirichlet((1, 1, 1), 12)):
            add_uv(w[0] * A + w[1] * B + w[2] * C)
    if t in (4, 5, 7):
        A, B, D = v[0], v[1], v[3]
        for k in range(16):
            a, b = rng.uniform(-0.1, 1.1, 2)
            add_uv(A + a * (B - A) + b * (D - A))
        for a in (0.0, 0.25, 0.5, 1.0):
            add_uv(A + a * (B - A) + a * (D - A))
    if t == 7:
        A, B, D = v[0], v[1], v[3]
        S, bw = float(s.S), float(s.borderwidth)
        L, W = np.linalg.norm(B - A), np.linalg.norm(D - A)
        u, w = (B - A) / L, (D - A) / W
        for i in (0, 1, 2, 3):                                                 # square borders: valid = 2
            for d_ in (-0.6 * bw, -0.5 * bw, -0.4 * bw, 0.0, 0.4 * bw, 0.5 * bw, 0.6 * bw):
                add_uv(A + (i * S + d_ + (0 if i else 0.7 * bw)) * u + (0.37 * S + (i % 2) * S) * w)
                add_uv(A + (0.41 * S) * u + (i * S + d_ + (0 if i else 0.7 * bw)) * w)
        for p in (v[4:8].mean(0), v[4], 0.5 * (v[4] + v[5])):                  # in and on the hole
            add_uv(p)
    if t == 8:
        c1, c2, r = v[0], v[1], float(s.radius)
        ax = c2 - c1
        L = np.linalg.norm(ax)
        a = ax / L
        e1 = np.cross(a, (0.2, 0.3, 1.0))
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(a, e1)
        S = float(s.S)
        for k in range(24):
            th, h = rng.uniform(0, 2 * np.pi), rng.uniform(0.02, 0.98) * L
            add_uv(c1 + h * a + r * (np.cos(th) * e1 + np.sin(th) * e2))
        for i in range(1, 4):                                                  # square boundaries along the axis
            for k in (-1e-3, 1e-3, 0.4 * float(s.borderwidth), 0.6 * float(s.borderwidth)):
                add_uv(c1 + (i * S + k) * a + r * e1)
        if c1[0] == 0:                                                         # p[0] == 0: u stays 0
            add_uv(np.array([0.0, c1[1] + 0.3 * L, c1[2] + r]))
            add_uv(np.array([0.0, c1[1] + 0.6 * L, c1[2] - r]))


def _free_function_cases(rng):
    fix = {"ray": [], "n": []}
    for k in range(40):
        fix["ray"].append(rng.normal(size=3) * rng.uniform(0.1, 5))
        fix["n"].append(rng.normal(size=3))
    for ray, n in (((1, 0, 0), (0, 1, 0)), ((1, 0, 0), (1e-300, 1, 0)), ((1, 0, 0), (-1e-300, 1, 0)),
                   ((0, 0, 0), (0, 0, 1)), ((1, 2, 3), (0, 0, 0)), ((1e-5, 0, 0), (1e-5, 0, 0))):
        fix["ray"].append(np.array(ray, dtype=np.float64))
        fix["n"].append(np.array(n, dtype=np.float64))
    cob = {"z": [rng.normal(size=3) * rng.uniform(0.1, 3) for _ in range(30)]}
    cob["z"] += [np.array(z, dtype=np.float64) for z in ((1, 0, 0), (-2, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0),
                                                          (1, 1e-13, 0), (1, 1e-11, 0), (3, 0, 4))]
    bary = {"p": [], "A": [], "B": [], "C": []}
    for k in range(60):
        A, B, C = rng.normal(size=(3, 3)) * 2
        w = rng.dirichlet((1, 1, 1)) if k % 3 else rng.uniform(-0.5, 1.5, 3)
        p = w[0] * A + w[1] * B + w[2] * C
        if k % 5 == 0:
            p = p + rng.normal(size=3) * 0.1
        if k < 3:
            p = (A, B, C)[k]
        if k == 59:
            C = A + 2 * (B - A)    # degenerate: n = 0
        for key, val in zip("pABC", (p, A, B, C)):
            bary[key].append(val)
    seg = {"A": [], "B": [], "ray": [], "origin": []}
    for k in range(60):
        A, B = rng.normal(size=(2, 3)) * 2
        x = rng.uniform(-0.2, 1.2)
        target = A + x * (B - A)
        origin = target + rng.normal(size=3) * 2
        ray = (target - origin) * rng.uniform(0.3, 3)
        if k % 4 == 1:
            ray = ray + rng.normal(size=3) * 10.0 ** rng.uniform(-6, -2)       # near misses around 1e-4
        if k % 4 == 2:
            ray = -ray
        if k == 58:
            ray = B - A                                                        # parallel lines: 0 / 0
        if k == 59:
            origin, ray = A.copy(), B - A
        for key, val in zip(("A", "B", "ray", "origin"), (A, B, ray, origin)):
            seg[key].append(val)
    return {"fix_norm": fix, "build_cob": cob, "barycentric": bary, "segment": seg}


# ---------------------------------------------------------------------------------------------------
# answering and comparing
# ---------------------------------------------------------------------------------------------------
def evaluate(backend, cases, only=None):
    """{fn: {field: array}}: the backend's answers to the drawn vectors. Functions only the reference
    has (intersectMax, shortestLine's coefficients, lineIntersect, derived members) are answered by a
    backend that has them."""
    out = {}

    def want(fn):
        return fn in cases and (only is None or fn in only)

    if want("intersect"):
        c = cases["intersect"]
        r = [backend.intersect(int(si), ray, st) for si, ray, st in zip(c["shape"], c["ray"], c["start"])]
        out["intersect"] = {"hit": np.array([x[0] for x in r], dtype=np.int32),
                            "t": np.array([x[1] for x in r], dtype=np.float32),
                            "inside": np.array([x[2] for x in r], dtype=np.int32),
                            "color": np.array([x[3] for x in r], dtype=np.float64)}
    if want("shadow"):
        c = cases["shadow"]
        out["shadow"] = {"hit": np.array([backend.shadow(int(si), ray, st, tm) for si, ray, st, tm in
                                          zip(c["shape"], c["ray"], c["start"], c["t_max"])], dtype=np.int32)}
    if want("cap"):
        c = cases["cap"]
        r = [backend.cap(int(si), ray, st) for si, ray, st in zip(c["shape"], c["ray"], c["start"])]
        out["cap"] = {"hit": np.array([x[0] for x in r], dtype=np.int32),
                      "t": np.array([x[1] for x in r], dtype=np.float32),
                      "inside": np.array([x[2] for x in r], dtype=np.int32)}
    if want("norm"):
        c = cases["norm"]
        r = [backend.norm(int(si), p, pr if pre else None, ps if pre else None)
             for si, p, pre, pr, ps in zip(c["shape"], c["p"], c["pre"], c["pre_ray"], c["pre_start"])]
        out["norm"] = {"n": np.array([x[0] for x in r], dtype=np.float64),
                       "last_hit": np.array([x[1] for x in r], dtype=np.int32),
                       "threw": np.array([x[2] for x in r], dtype=np.int32)}
    if want("uv"):
        c = cases["uv"]
        r = [backend.uv(int(si), p) for si, p in zip(c["shape"], c["p"])]
        out["uv"] = {"uv": np.array([x[0] for x in r], dtype=np.float64),
                     "valid": np.array([x[1] for x in r], dtype=np.int32)}
    if want("box"):
        c = cases["box"]
        with np.errstate(divide="ignore"):
            inv = 1.0 / c["ray"]
        r = [backend.box(int(si), int(leaf), ray, iv, st)
             for si, leaf, ray, iv, st in zip(c["shape"], c["leaf"], c["ray"], inv, c["start"])]
        out["box"] = {"hit": np.array([x[0] for x in r], dtype=np.int32),
                      "lb": np.array([x[1] for x in r], dtype=np.float64),
                      "ub": np.array([x[2] for x in r], dtype=np.float64)}
    if want("fix_norm"):
        c = cases["fix_norm"]
        out["fix_norm"] = {"n": np.array([backend.fix_norm(r, n) for r, n in zip(c["ray"], c["n"])])}
    if want("barycentric"):
        c = cases["barycentric"]
        out["barycentric"] = {"w": np.array([backend.bary(*x) for x in zip(c["p"], c["A"], c["B"], c["C"])])}
    if want("segment"):
        c = cases["segment"]
        out["segment"] = {"hit": np.array([backend.segment(*x) for x in zip(c["A"], c["B"], c["ray"], c["origin"])],
                                          dtype=np.int32)}
    return out


def evaluate_shapes(backend, n_shapes, types):
    """per-shape answers: getBounds, the BoundingVolume bounds (leaf / inner), CheckerCylinder::objM"""
    lb, ub, blb, bub, objM = [], [], [], [], []
    for si in range(n_shapes):
        l, u = backend.bounds(si)
        lb.append(l)
        ub.append(u)
        for leaf in (1, 0):
            _, l2, u2 = backend.box(si, leaf)
            blb.append(l2)
            bub.append(u2)
        objM.append(backend.objM(si) if types[si] == 8 else np.zeros(16))
    return {"lb": np.array(lb), "ub": np.array(ub), "box_lb": np.array(blb).reshape(n_shapes, 2, 3),
            "box_ub": np.array(bub).reshape(n_shapes, 2, 3), "objM": np.array(objM)}


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def differs(a, b):
    """per vector: True where a and b differ. Integers as integers; floats by bit pattern, except that
    any NaN equals any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind == "f":
        d = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
    else:
        d = a != b
    return d.reshape(len(a), -1).any(axis=1) if a.ndim > 1 else d


def comparable(fn, field, want, types_of_vector):
    """Which vectors of a field the oracle answers at all. RectPrismWithCylinder::getNorm: the reference
    keeps lastHit from an intersect that returned false and answers with that hole's normal, or throws
    past the three face tests; the render loop (and so the oracle) asks for a normal only after a hit,
    when lastHit is -1, and counts the throw. Those vectors are stored, not compared."""
    n = len(want[field])
    ok = np.ones(n, dtype=bool)
    if fn == "norm":
        rpc = types_of_vector == 9
        if field == "n":
            ok &= ~(rpc & ((want["last_hit"] >= 0) | (want["threw"] != 0)))
        if field in ("last_hit", "threw"):
            ok &= ~(rpc & (want["last_hit"] >= 0))
            if field == "threw":
                ok &= rpc
    return ok


def mismatches(fn, want, got, types_of_vector=None):
    """{field: indices of vectors where got differs from want}"""
    out = {}
    for field in want:
        d = differs(want[field], got[field])
        if types_of_vector is not None:
            d &= comparable(fn, field, want, types_of_vector)
        out[field] = np.nonzero(d)[0]
    return out


# ---------------------------------------------------------------------------------------------------
# one-shape camera scenes (tests/test_gpu_geom.py)
# ---------------------------------------------------------------------------------------------------
def or_primary_ray(g, frame, first, n):
    o = oracle()
    o.or_primary_ray.argtypes = [P(Globals), ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, _D, _D]
    start, d = np.zeros((n, 3)), np.zeros((n, 3))
    rc = o.or_primary_ray(ctypes.byref(g), int(frame), int(first), int(n), start.ctypes.data_as(_D),
                          d.ctypes.data_as(_D))
    if rc:
        raise RuntimeError("or_primary_ray failed %d" % rc)
    return start, d


def globals_from_record(rec):
    g = Globals()
    rec = np.ascontiguousarray(rec, dtype=GLOBALS_DT)
    ctypes.memmove(ctypes.byref(g), rec.ctypes.data, rec.nbytes)
    return g


def record_from_globals(g):
    """field by field into a zeroed record: the struct's padding bytes are not data"""
    rec = np.zeros((), dtype=GLOBALS_DT)
    for name, _ in Globals._fields_:
        v = getattr(g, name)
        rec[name] = list(v) if hasattr(v, "__len__") else v
    return rec


def one_shape_scene(shape_rec, hole_rec):
    """(SceneDesc, keepalive): the one shape (with the holes of a RectPrismWithCylinder) and a point light"""
    shapes = shapes_from_records(np.array([shape_rec], dtype=SHAPE_DT))
    holes = shapes_from_records(hole_rec) if shapes[0].n_holes else None
    lights = (LightDesc * 1)()
    lights[0].type, lights[0].shape_index = 1, -1
    for a in range(3):
        lights[0].center[a] = (3.0, 5.0, 2.0)[a]
        lights[0].color[a] = 1.0
    d, keep = scene_desc(shapes, holes, lights, n_shapes=1)
    if holes is not None:
        d.n_holes = len(hole_rec)
    return d, keep
