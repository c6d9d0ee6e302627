"""Deterministic synthetic scenes under a similarity transform, built through the ABI's descriptor
structs as a caller of dt_scene_create would (a plain helper module, imported by the tests).

Every scene is written in unit coordinates and takes a scale s and an offset t; x -> s*x + t is
applied to everything that carries a position (vertices, centres, light frames, holes, eye,
lookingAt, cap_center) and s alone to everything that carries a length (radius, S, borderwidth,
length, width, focal_length, aperture, near_plane, far_dist, move_per_frame, tot_move, accel_t).
Colours, directions (up, baxis), fov and the sample counts are untouched. With a power of two for
s the scene's own proportions survive exactly. Each function returns (desc, g, keepalive).

The culling structures (host_shadowgrid.cpp, host_primlists.cpp, host_fasttree.cpp) hold absolute
margins chosen at room scale, as do the reference's own constants (shadow rays start 1e-3 along the
ray); CASES are the transforms that move a scene away from that scale: tests/test_scale_host.py,
tests/test_gpu_scale.py.
"""
import math

import distraytracer_amd as dt
from distraytracer_amd import _lib

F_LIGHT, F_MOTION, F_GLOSSY, F_NAMED_RECT = 1, 2, 8, 16   # include/dt.h DT_F_*
SPHERE, CYLINDER, TRIANGLE, RECTANGLE, PRISM_V2, CHECKER, CHECKER_HOLE = 1, 2, 3, 4, 5, 6, 7
PHONG, OREN_NAYAR, COOK_TORRANCE, RAW = 0, 1, 2, 3
GLASS, STEEL, LINOLEUM = 1, 2, 5
POINT_LIGHT, SPHERE_LIGHT, RECT_LIGHT = 1, 2, 3

# name -> (s, t): powers of two, so that s*x + t is exact for the scenes' short coordinates
CASES = {
    "unit": (1.0, (0.0, 0.0, 0.0)),
    "tiny": (2.0 ** -8, (0.0, 0.0, 0.0)),
    "tiny-shifted": (2.0 ** -8, (16.0, -8.0, 32.0)),
    "shifted": (1.0, (4096.0, -2048.0, 8192.0)),
    "huge": (2.0 ** 8, (0.0, 0.0, 0.0)),
}

_POSITIONS = ("center", "A", "B", "D")            # light fields; shapes: v and center
_LENGTHS = ("radius", "S", "borderwidth", "length", "width")


class _Builder:
    """Collects shape, hole and light records in unit coordinates and writes them transformed."""

    def __init__(self, s, t):
        self.s, self.t = float(s), tuple(float(v) for v in t)
        self.shapes, self.lights = [], []

    def pos(self, p):
        return tuple(self.s * float(p[a]) + self.t[a] for a in range(3))

    def shape(self, t, **kw):
        """A shape record; v and center are positions, _LENGTHS lengths, everything else as given."""
        r = _lib.ShapeDesc()
        r.type = t
        r.tex_frame = -1
        for k, v in kw.items():
            if k == "v":
                for i, p in enumerate(v):
                    q = self.pos(p)
                    for a in range(3):
                        r.v[i][a] = q[a]
            elif k == "center":
                q = self.pos(v)
                for a in range(3):
                    r.center[a] = q[a]
            elif k in _LENGTHS:
                setattr(r, k, self.s * v)
            elif isinstance(v, (list, tuple)):
                for a in range(len(v)):
                    getattr(r, k)[a] = v[a]
            else:
                setattr(r, k, v)
        self.shapes.append(r)
        return len(self.shapes) - 1

    def light(self, t, shape_index=-1, radius=0.0, **kw):
        r = _lib.LightDesc()
        r.type, r.shape_index, r.radius = t, shape_index, self.s * radius
        for k, v in kw.items():
            q = self.pos(v) if k in _POSITIONS else v
            for a in range(3):
                getattr(r, k)[a] = q[a]
        self.lights.append(r)
        return len(self.lights) - 1

    def globals(self, eye, looking_at, aperture, focal_length):
        g = dt.globals_default()
        g.use_model = 0
        e, l, c = self.pos(eye), self.pos(looking_at), self.pos(tuple(g.cap_center))
        for a in range(3):
            g.eye[a], g.lookingAt[a], g.cap_center[a] = e[a], l[a], c[a]
        g.aperture, g.focal_length = self.s * aperture, self.s * focal_length
        for k in ("near_plane", "far_dist", "move_per_frame", "tot_move", "accel_t"):
            setattr(g, k, self.s * getattr(g, k))
        return g

    def desc(self):
        arr = (_lib.ShapeDesc * len(self.shapes))(*self.shapes)
        lights = (_lib.LightDesc * len(self.lights))(*self.lights)
        return _lib.SceneDesc(len(self.shapes), len(self.lights), 0, 0, arr, lights, None), (arr, lights)


def features(s=1.0, t=(0.0, 0.0, 0.0)):
    """A synthetic scene for the shading paths the shipped builders never use: a glass sphere
    (refraction + Fresnel, Q5), a steel mirror sphere, an Oren-Nayar sphere, a raw triangle, a
    plain Checkerboard floor (geometry.cpp:2248-2341), a sphere light with a bounding axis
    (rejection sampling, Q11), a rectangle light and a point light."""
    b = _Builder(s, t)
    A, B, C, D = (-5, 0, 5), (5, 0, 5), (5, 0, -5), (-5, 0, -5)
    b.shape(CHECKER, v=[A, B, C, D], color=(0.5, 0.5, 0.5), color1=(0.9, 0.9, 0.9), color2=(0.1, 0.1, 0.3), S=1.0,
            length=10.0, width=10.0, center=(0, 0, 0))
    b.shape(SPHERE, v=[(0.5, 1.0, 0.0)], radius=0.6, color=(0.9, 0.9, 1.0), material=GLASS, center=(0.5, 1.0, 0.0))
    b.shape(SPHERE, v=[(-1.2, 0.7, 0.5)], radius=0.5, color=(0.8, 0.8, 0.8), material=STEEL, center=(-1.2, 0.7, 0.5))
    b.shape(SPHERE, v=[(1.8, 0.5, -0.8)], radius=0.5, color=(0.9, 0.4, 0.2), model=OREN_NAYAR, roughness=0.3,
            center=(1.8, 0.5, -0.8))
    b.shape(TRIANGLE, v=[(-2, 0, -2), (-1, 2, -2), (0, 0, -2)], color=(0.2, 0.8, 0.3), model=RAW,
            center=(-1, 2 / 3, -2))
    sl = b.shape(SPHERE, v=[(0, 3.5, 1)], radius=0.3, color=(1, 1, 0.9), emit=1, flags=F_LIGHT, center=(0, 3.5, 1))
    ra, rb, rc, rd = (-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1)
    rl = b.shape(RECTANGLE, v=[ra, rb, rc, rd], color=(0.8, 0.8, 0.8), emit=2, flags=F_LIGHT, length=1.0, width=1.0,
                 center=(0, 4, 0))
    b.light(SPHERE_LIGHT, sl, 0.3, center=(0, 3.5, 1), color=(1, 1, 0.9), baxis=(0, -1, 0))
    b.light(RECT_LIGHT, rl, center=(0, 4, 0), color=(0.8, 0.8, 0.8), A=ra, B=rb, D=rd)
    b.light(POINT_LIGHT, center=(3, 3, 3), color=(0.6, 0.6, 0.6))
    g = b.globals((-4.0, 2.5, 4.0), (0.3, 0.8, -0.2), 0.1, 6.0)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth, g.brdf_samples = 160, 120, 9, 5, 2
    desc, keep = b.desc()
    return desc, g, keep


def _rect(b, A, B, C, D, color, flags=F_NAMED_RECT, **kw):
    """Rectangle(a, b, c, d) as the builders make it: float length |B-A| and width |D-A|, the centre the
    corners' mean, named "rectangle" (it shifts in the motion-blur passes) unless flags says otherwise"""
    cen = tuple((A[a] + B[a] + C[a] + D[a]) / 4 for a in range(3))
    return b.shape(RECTANGLE, v=[A, B, C, D], color=color, flags=flags, length=math.dist(A, B), width=math.dist(A, D),
                   center=cen, **kw)


def _cylinder(b, c1, c2, radius, color, **kw):
    cen = tuple((c1[a] + c2[a]) / 2 for a in range(3))
    return b.shape(CYLINDER, v=[c1, c2], radius=radius, color=color, center=cen, **kw)


# The plate of the room family: 6 x 6 at y = 2 under the point light at (0, 3.5, 0). The umbra proof of
# host_shadowgrid.cpp wants every crossing point mu >= 3e-3 inside the face and the cells mud >= 2e-3 below
# it, absolute lengths: at s = 2^-8 the plate is 0.023 wide and 0.0078 above the floor, and whole 8 x 4
# blocks of grid cells under it still pass (a 3 x 3 plate at y = 1.5 left none there). Its shadow covers
# the floor and ends on the walls at y = 1.5.
PLATE = ((-3, 2, 3), (3, 2, 3), (3, 2, -3), (-3, 2, -3))


def room(s=1.0, t=(0.0, 0.0, 0.0), plate=True, motion=None):
    """Shapes, lights and materials of the room builds only (DT_ROOM_FEATURES: dt_trace_kernel below 64
    spp, dt_trace_kernel_w5 from 64): a glossy linoleum checkerboard floor (with a small hole in a back
    corner: the plain Checkerboard is not a room feature, nor is a sphere, so the round shapes are
    cylinders), a back and a side wall, a Phong and a Cook-Torrance cylinder standing on the floor, a
    steel one lying on it, a RectPrismV2, and a plain rectangle plate hovering over most of the
    floor under a point light, so that whole blocks of grid cells lie in that light's umbra; a second
    point light low at the side (it lights the room under the plate) and a rectangle light with its emitter at the ceiling.
    plate=False leaves the plate out (what its shadow changes: tests/test_scale_host.py).
    motion=(move_per_frame, accel_t), in unit lengths: the motion family -- the lying cylinder, the prism
    and a "rectangle" panel are DT_F_MOTION, so samples that hit them re-trace with every "rectangle"
    shifted in y and the leaf boxes bumped (cpp:1095-1210); render at a frame >= frame_blur."""
    b = _Builder(s, t)
    mv = F_MOTION if motion else 0
    b.shape(CHECKER_HOLE, v=[(-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4),
                             (2.5, 0, -2.5), (3.5, 0, -2.5), (3.5, 0, -3.5), (2.5, 0, -3.5)],
            color=(0.58, 0.82, 1.0), color1=(0.58, 0.82, 1.0), color2=(1.0, 0.416, 0.835), S=1.0, length=8.0,
            width=8.0, center=(0, 0, 0), material=LINOLEUM, flags=F_GLOSSY, roughness=0.6, refr=(1.543, 0.0))
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99))          # back wall
    _rect(b, (4, 0, -4), (4, 0, 4), (4, 4, 4), (4, 4, -4), (0.9, 0.8, 0.3))                # side wall
    _cylinder(b, (-2.5, 0, -1.5), (-2.5, 1.5, -1.5), 0.5, (0.9, 0.3, 0.2))
    _cylinder(b, (2.25, 0, 0.5), (2.25, 1.0, 0.5), 0.5, (0.95, 0.64, 0.54), model=COOK_TORRANCE, roughness=0.4,
              refr=(2.75, 3.79))
    _cylinder(b, (-1.5, 0.375, 2.0), (-0.5, 0.375, 2.5), 0.375, (0.8, 0.8, 0.8), material=STEEL, flags=mv)
    pa, pb, pc, pd = (0.5, 0, -2), (1.5, 0, -2), (1.5, 0, -3), (0.5, 0, -3)
    up = lambda p: (p[0], p[1] + 0.75, p[2])
    b.shape(PRISM_V2, v=[pa, pb, pc, pd, up(pa), up(pb), up(pc), up(pd)], color=(0.3, 0.9, 0.4), length=1.0, width=1.0,
            center=(1.0, 0.375, -2.5), flags=mv)
    if plate:
        _rect(b, *PLATE, (0.7, 0.7, 0.75), flags=0)
    if motion:
        _rect(b, (-3.5, 0.25, 1.0), (-2.5, 0.25, 1.0), (-2.5, 1.5, 1.0), (-3.5, 1.5, 1.0), (0.9, 0.9, 0.2),
              flags=F_NAMED_RECT | F_MOTION)
    ra, rb, rc, rd = (1.5, 3.75, -1.5), (2.5, 3.75, -1.5), (2.5, 3.75, -2.5), (1.5, 3.75, -2.5)
    rl = b.shape(RECTANGLE, v=[ra, rb, rc, rd], color=(0.8, 0.8, 0.8), emit=2, flags=F_LIGHT, length=1.0, width=1.0,
                 center=(2.0, 3.75, -2.0))
    b.light(POINT_LIGHT, center=(0, 3.5, 0), color=(0.9, 0.9, 0.9))
    b.light(POINT_LIGHT, center=(-3.5, 1.0, 3.0), color=(0.5, 0.5, 0.5))
    b.light(RECT_LIGHT, rl, center=(2.0, 3.75, -2.0), color=(0.7, 0.7, 0.7), A=ra, B=rb, D=rd)
    g = b.globals((0.5, 1.25, 6.5), (0.0, 0.75, 0.0), 0.0625, 6.0)
    if motion:
        g.move_per_frame, g.accel_t = s * motion[0], s * motion[1]
    g.xRes, g.yRes, g.antialias_samples, g.max_depth, g.brdf_samples = 96, 64, 4, 4, 2
    desc, keep = b.desc()
    return desc, g, keep


# the motion family's shifts val = move_per_frame d + accel_t d^3, d in [0, frame_range = 1], in unit lengths:
# small against the 8-unit room, and up to 3.5 units, about half of it (bumped leaf boxes outgrow their
# parents: the bump tree's ancestor-chain test; padded lists overflow: the pass-0 grid)
MOTION_SHIFTS = {"small": (2.0 ** -6, 2.0 ** -7), "large": (0.5, 3.0)}


def motion(s=1.0, t=(0.0, 0.0, 0.0), shift="small"):
    """room() with shapes in motion; returns (desc, g, keepalive) for a render at MOTION_FRAME"""
    return room(s, t, motion=MOTION_SHIFTS[shift])


MOTION_FRAME = 1600   # the default frame_blur: val takes the cubic term as well (Q19)

FAMILIES = {
    "room": (room, 0),
    "features": (features, 0),
    "motion-small": (lambda s, t: motion(s, t, "small"), MOTION_FRAME),
    "motion-large": (lambda s, t: motion(s, t, "large"), MOTION_FRAME),
}


def build(family, case):
    """(desc, g, keepalive, frame) of a family under a case's transform"""
    fn, frame = FAMILIES[family]
    s, t = CASES[case]
    desc, g, keep = fn(s, t)
    return desc, g, keep, frame


# ---------------------------------------------------------------------------------------------------
# The shaded-ray scenes of tests/golden/shade_ref.npz (tools/gen_golden_shade.py): every one
# deterministic once its primary rays are given -- point lights, or area lights without extent -- so that
# the reference's own rayColor answers them without its unseeded RNG. 32 x 16 pixels at 1 spp, depth 4,
# depth of field on, unless said otherwise; lights dim enough that few channels clamp.
# ---------------------------------------------------------------------------------------------------
F_TEXTURE, F_UV_VERTS = 4, 64   # include/dt.h DT_F_*
SHADE_TEXTURE = "models/Column_LP_obj/Textures/Marble_Base_Color.jpg.rgb"   # under the package's DATA_DIR

_MODEL_KW = {PHONG: {}, OREN_NAYAR: dict(roughness=0.3), COOK_TORRANCE: dict(roughness=0.4, refr=(2.75, 3.79)), RAW: {}}


def _triangle(b, A, B, C, color, **kw):
    cen = tuple(((A[a] + B[a]) + C[a]) / 3 for a in range(3))     # Triangle's constructor: (A + B + C) / 3
    return b.shape(TRIANGLE, v=[A, B, C], color=color, center=cen, **kw)


def _shade_globals(b, g, res=(32, 16), spp=1, depth=4):
    g.xRes, g.yRes, g.antialias_samples, g.max_depth, g.brdf_samples = res[0], res[1], spp, depth, 2
    desc, keep = b.desc()
    return desc, g, keep


def _two_lights(b):
    """one point light above a hovering plate (its umbra covers part of the floor), one low at the side"""
    _rect(b, (-3.5, 2.5, 2.0), (-1.0, 2.5, 2.0), (-1.0, 2.5, -1.0), (-3.5, 2.5, -1.0), (0.7, 0.7, 0.75), flags=0)
    b.light(POINT_LIGHT, center=(-2.5, 3.5, 0.5), color=(0.45, 0.45, 0.45))
    b.light(POINT_LIGHT, center=(3.0, 3.0, 3.0), color=(0.35, 0.35, 0.3))


def shade_model(model, triangle=True, res=(32, 16), spp=1):
    """A floor, a back wall, a standing cylinder and (triangle=True) a triangle of one shading model under
    two point lights, one partly occluded by a plate: pixels lit by none, one and both. Without the triangle
    the Phong and Cook-Torrance scenes hold room features only, with it (or with Oren-Nayar) mesh features."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    kw = dict(model=model, **_MODEL_KW[model])
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=0, **kw)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99), flags=0, **kw)
    _cylinder(b, (0.25, 0, 0.5), (0.25, 2.0, 0.5), 1.0, (0.95, 0.64, 0.54), **kw)
    if triangle:
        _triangle(b, (-3.0, 0.25, 1.0), (-1.5, 0.25, 1.5), (-2.25, 2.0, 0.5), (0.2, 0.8, 0.3), **kw)
    # a panel in the back wall's own plane, after it in the shape list: rays that hit both at the same float t
    # keep the first of the gather order (the closest hit's strict <)
    _rect(b, (1.5, 1.0, -4), (3.0, 1.0, -4), (3.0, 2.5, -4), (1.5, 2.5, -4), (0.9, 0.2, 0.2), flags=0, **kw)
    # a panel 1.5e-3 above the second light: a shadow ray that starts 1e-3 along its direction reaches it
    # beyond t_max whatever its angle, one that started 2e-3 along would reach it before t_max when steep
    _rect(b, (1.5, 3.0015, 4.5), (4.5, 3.0015, 4.5), (4.5, 3.0015, 1.5), (1.5, 3.0015, 1.5), (0.7, 0.7, 0.75), flags=0)
    _two_lights(b)
    return _shade_globals(b, b.globals((0.5, 1.25, 6.5), (0.0, 0.75, 0.0), 0.0625, 6.0), res, spp)


def shade_mirror(triangle=False):
    """Steel, not glossy: a lying cylinder and a wall panel; the floor is glossy linoleum and nogloss = 1, so
    it takes the mirror path too. Room features only; with a (steel) triangle, mesh features."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    if triangle:
        _triangle(b, (-3.5, 0.25, 2.0), (-2.0, 0.25, 2.5), (-2.75, 1.75, 1.5), (0.8, 0.8, 0.8), material=STEEL)
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=F_GLOSSY, material=LINOLEUM,
          roughness=0.6, refr=(1.543, 0.0))
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99), flags=0)
    _rect(b, (-3.0, 0.5, -3.5), (-0.5, 0.5, -3.0), (-0.5, 3.0, -3.0), (-3.0, 3.0, -3.5), (0.8, 0.8, 0.8), flags=0,
          material=STEEL)
    _cylinder(b, (0.5, 0.5, 1.0), (2.5, 0.5, 0.0), 0.5, (0.8, 0.8, 0.8), material=STEEL)
    _cylinder(b, (-1.5, 0, 1.0), (-1.5, 1.5, 1.0), 0.4, (0.9, 0.3, 0.2))
    b.light(POINT_LIGHT, center=(-2.5, 3.5, 2.5), color=(0.4, 0.4, 0.4))
    b.light(POINT_LIGHT, center=(3.0, 3.0, 3.0), color=(0.3, 0.3, 0.3))
    g = b.globals((0.5, 1.25, 6.5), (0.0, 0.75, 0.0), 0.0625, 6.0)
    g.nogloss = 1
    return _shade_globals(b, g)


def shade_glass():
    """A glass sphere and a glass pane (RectPrismV2) over a floor before a wall: rays enter and leave both;
    off-centre hits on the sphere are the rays whose Fresnel weights are NaN on both sides (Q25). The sphere
    is small: a ray that leaves it through its middle reads the reference's uninitialised `inside` (Q5), and
    the compiled reference and the defined reading must agree on 98 % of the class."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=0)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.9, 0.5, 0.2), flags=0)
    b.shape(SPHERE, v=[(1.25, 1.0, 1.0)], radius=0.5625, color=(0.9, 0.9, 1.0), material=GLASS, center=(1.25, 1.0, 1.0))
    pa, pb, pc, pd = (-2.5, 0.25, 1.5), (-0.5, 0.25, 1.5), (-0.5, 0.25, 1.25), (-2.5, 0.25, 1.25)
    up = lambda p: (p[0], p[1] + 2.0, p[2])
    b.shape(PRISM_V2, v=[pa, pb, pc, pd, up(pa), up(pb), up(pc), up(pd)], color=(0.9, 1.0, 0.9), material=GLASS,
            length=2.0, width=0.25, center=(-1.5, 1.25, 1.375))
    _cylinder(b, (-1.5, 0, -1.5), (-1.5, 1.5, -1.5), 0.5, (0.9, 0.3, 0.2))
    b.light(POINT_LIGHT, center=(-2.5, 3.5, 2.5), color=(0.4, 0.4, 0.4))
    b.light(POINT_LIGHT, center=(3.0, 3.0, 3.0), color=(0.3, 0.3, 0.3))
    return _shade_globals(b, b.globals((0.5, 1.25, 6.5), (0.0, 0.75, 0.0), 0.0625, 6.0))


def shade_emitters():
    """The camera sees a "spherelight" and a "rectanglelight" shape directly (their emission formulas); the
    floor and wall are lit by a point light, the emitters only occlude."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=0)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99), flags=0)
    b.shape(SPHERE, v=[(1.5, 1.25, 0.5)], radius=0.75, color=(0.6, 0.55, 0.4), emit=1, flags=F_LIGHT, center=(1.5, 1.25, 0.5))
    ra, rb, rc, rd = (-3.0, 0.5, -1.0), (-1.0, 0.5, 0.0), (-1.0, 2.0, 0.0), (-3.0, 2.0, -1.0)
    b.shape(RECTANGLE, v=[ra, rb, rc, rd], color=(0.5, 0.6, 0.6), emit=2, flags=F_LIGHT, length=1.0, width=1.0,
            center=tuple((ra[a] + rb[a] + rc[a] + rd[a]) / 4 for a in range(3)))
    b.light(POINT_LIGHT, center=(0.0, 3.5, 3.0), color=(0.5, 0.5, 0.5))
    return _shade_globals(b, b.globals((0.5, 1.25, 6.5), (0.0, 0.75, 0.0), 0.0625, 6.0))


def shade_textured(pixels, width, height):
    """A textured triangle with UV vertices and a textured CheckerboardWithHole floor with a border (getUV
    types 1 and 2; its hole type 0) under one point light. pixels: width * height * 3 bytes, kept alive by
    the returned keepalive."""
    import ctypes
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    b.shape(CHECKER_HOLE, v=[(-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4),
                             (1.5, 0, 2.5), (2.5, 0, 2.5), (2.5, 0, 1.5), (1.5, 0, 1.5)],
            color=(0.58, 0.82, 1.0), color1=(0.58, 0.82, 1.0), color2=(1.0, 0.416, 0.835), S=2.0, length=8.0, width=8.0,
            borderwidth=0.25, bordercolor=(0.3, 0.1, 0.4), center=(0, 0, 0), flags=F_TEXTURE, tex_frame=0)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99), flags=0)
    A, B, C = (-2.5, 0.25, 0.0), (1.5, 0.25, -1.0), (-0.5, 3.0, -1.5)
    _triangle(b, A, B, C, (0.2, 0.8, 0.3), flags=F_TEXTURE | F_UV_VERTS, tex_frame=0,
              uv=[(0.0, 0.0), (1.0, 0.125), (0.5, 1.0)])
    b.light(POINT_LIGHT, center=(0.5, 3.5, 3.0), color=(0.6, 0.6, 0.6))
    desc, g, keep = _shade_globals(b, b.globals((0.5, 1.5, 6.5), (0.0, 0.5, 0.0), 0.0625, 6.0))
    buf = (ctypes.c_uint8 * len(pixels)).from_buffer_copy(bytes(pixels))
    tex = (_lib.TextureDesc * 1)()
    tex[0].width, tex[0].height, tex[0].channels = width, height, 3
    tex[0].pixels = ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8))
    desc.n_textures, desc.textures = 1, tex
    return desc, g, (keep, buf, tex)


def shade_area():
    """Area lights without extent: a rectangle light with A == B == D (and C) and a sphere light of radius 0.
    A + x (B - A) + y (D - A) and radius * (...) + center then do not depend on the draws. Both light objects
    are shapes of the scene too, but shapes without extent that no shadow ray can hit: this class pins the
    area-light shadow path and the light colour, not the own-shape skip (shade_own_shape does)."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=0)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99), flags=0)
    _cylinder(b, (0.25, 0, 0.5), (0.25, 2.0, 0.5), 1.0, (0.95, 0.64, 0.54))
    p, q = (-2.5, 3.5, 1.5), (3.0, 3.0, 2.0)
    rl = b.shape(RECTANGLE, v=[p, p, p, p], color=(0.8, 0.8, 0.8), emit=2, flags=F_LIGHT, length=1.0, width=1.0, center=p)
    sl = b.shape(SPHERE, v=[q], radius=0.0, color=(1.0, 1.0, 0.9), emit=1, flags=F_LIGHT, center=q)
    b.light(RECT_LIGHT, rl, center=p, color=(0.45, 0.45, 0.45), A=p, B=p, D=p)
    b.light(SPHERE_LIGHT, sl, 0.0, center=q, color=(0.35, 0.35, 0.3))
    return _shade_globals(b, b.globals((0.5, 1.25, 6.5), (0.0, 0.75, 0.0), 0.0625, 6.0))


def shade_own_shape():
    """The light-is-this-shape skip of the shadow loop: a rectangle light WITH extent, a shape of the scene,
    over a floor and a low wall of the raw model. A raw surface's contribution is its own colour whatever the
    light's direction, so a sample's colour depends on the draws only through the shadow verdict; nothing but
    the light's own rectangle lies on a segment to a point of it, so every draw is unoccluded once the own
    shape is skipped (the surface's colour) -- and occluded by it, 1e-3 before t_max, if it were not (black).
    No sphere light: sphereLight::sampleRay returns the sampled point itself (Q11), a direction that does not
    aim at the sphere, so its own-shape skip is out of a deterministic scene's reach."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=0, model=RAW)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 2, -4), (-4, 2, -4), (0.0, 0.81, 0.99), flags=0, model=RAW)
    ra, rb, rc, rd = (-3.0, 3.5, 1.0), (-2.0, 3.5, 1.0), (-2.0, 3.5, 0.0), (-3.0, 3.5, 0.0)
    rl = b.shape(RECTANGLE, v=[ra, rb, rc, rd], color=(0.8, 0.8, 0.8), emit=2, flags=F_LIGHT, length=1.0, width=1.0,
                 center=(-2.5, 3.5, 0.5))
    b.light(RECT_LIGHT, rl, center=(-2.5, 3.5, 0.5), color=(0.45, 0.45, 0.45), A=ra, B=rb, D=rd)
    return _shade_globals(b, b.globals((0.5, 1.25, 6.5), (0.0, 0.75, 0.0), 0.0625, 6.0))


def shade_grazing():
    """The mirror branch's `refl_ray . n > eps` cut (eps = 1e-3f). The camera looks level from y = 1 through a
    lens of 2^-10, so the rays of pixel row 8 are level to 1e-4; a steel strip rises towards the back by
    1.1e-3 per unit and meets them about 3.6 away. Along the row |ray| grows from 1 to 1.25, so the cosine
    between ray and strip runs from about 1.2e-3 in the middle to 0.8e-3 at the ends: rays on both sides of
    the cut. The reflected rays climb to the (wide) back wall. Every other row passes over or under the strip."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=0)
    _rect(b, (-12, 0, -4), (12, 0, -4), (12, 4, -4), (-12, 4, -4), (0.9, 0.5, 0.2), flags=0)   # wide: every reflection meets it
    y = lambda z: 1.0 + 1.1e-3 * (2.9 - z)
    _rect(b, (-4, y(5.0), 5.0), (4, y(5.0), 5.0), (4, y(0.0), 0.0), (-4, y(0.0), 0.0), (0.8, 0.8, 0.8), flags=0,
          material=STEEL)
    _cylinder(b, (-1.5, 0, -1.5), (-1.5, 1.5, -1.5), 0.5, (0.9, 0.3, 0.2))
    b.light(POINT_LIGHT, center=(-2.5, 3.5, 2.5), color=(0.4, 0.4, 0.4))
    b.light(POINT_LIGHT, center=(3.0, 3.0, 3.0), color=(0.3, 0.3, 0.3))
    return _shade_globals(b, b.globals((0.0, 1.0, 6.5), (0.0, 1.0, 0.0), 2.0 ** -10, 6.0))


# class name -> scene function; the wave5 scenes are 8 x 4 pixels at 64 spp (2048 rays: the smallest image
# that selects the 5-wave builds), "averaged" 16 x 8 at 4 spp
SHADE_SCENES = {
    "phong": lambda: shade_model(PHONG),
    "oren-nayar": lambda: shade_model(OREN_NAYAR),
    "cook-torrance": lambda: shade_model(COOK_TORRANCE),
    "raw": lambda: shade_model(RAW),
    "mirror": shade_mirror,
    "glass": shade_glass,
    "emitters": shade_emitters,
    "area": shade_area,
    "wave5-phong": lambda: shade_model(PHONG, triangle=False, res=(8, 4), spp=64),
    "wave5-cook-torrance": lambda: shade_model(COOK_TORRANCE, triangle=False, res=(8, 4), spp=64),
    "wave5-oren-nayar": lambda: shade_model(OREN_NAYAR, res=(8, 4), spp=64),
    "averaged": lambda: shade_model(PHONG, res=(16, 8), spp=4),
    # mesh-featured twins: the 4-wave and 5-wave mesh builds get the mirror, Phong and Cook-Torrance loops too
    "mirror-mesh": lambda: shade_mirror(triangle=True),
    "wave5-phong-mesh": lambda: shade_model(PHONG, res=(8, 4), spp=64),
    "wave5-cook-torrance-mesh": lambda: shade_model(COOK_TORRANCE, res=(8, 4), spp=64),
    "own-shape": shade_own_shape,
    "grazing": shade_grazing,
}


# ---------------------------------------------------------------------------------------------------
# The stochastic scenes of tests/golden/shade_sampling_ref.npz (tools/gen_golden_shade_sampling.py): area
# lights WITH extent, sphere lights with a radius, glossy reflectors with nogloss = 0, shapes in motion.
# The draw-tape build of the reference answers their rays with the draws the oracle logged
# (or_sample_color_log) as the tape. No glass; blur_samples = 0 in the stored globals (the blur passes are
# renderImage's, not rayColor's). Lights are dim and mostly of one channel each: a channel then says which
# light lit a sample.
# ---------------------------------------------------------------------------------------------------
_GLOSSY_KW = dict(material=LINOLEUM, roughness=0.6, refr=(1.543, 0.0))
_CAMERA = ((0.5, 1.25, 6.5), (0.0, 0.75, 0.0), 0.0625, 6.0)


def _sampling_globals(b, g, res, spp, depth, brdf):
    g.xRes, g.yRes, g.antialias_samples, g.max_depth, g.brdf_samples = res[0], res[1], spp, depth, brdf
    g.nogloss, g.blur_samples = 0, 0
    desc, keep = b.desc()
    return desc, g, keep


def _rect_light(b, A, B, D, color, shape=False):
    """a rectangle light over A, B, D (C = B + D - A); shape=True: also the "rectanglelight" shape it is"""
    C = tuple(B[a] + D[a] - A[a] for a in range(3))
    cen = tuple((A[a] + B[a] + C[a] + D[a]) / 4 for a in range(3))
    si = -1
    if shape:
        si = b.shape(RECTANGLE, v=[A, B, C, D], color=(0.8, 0.8, 0.8), emit=2, flags=F_LIGHT, length=1.0, width=1.0,
                     center=cen)
    return b.light(RECT_LIGHT, si, center=cen, color=color, A=A, B=B, D=D)


def sampling_rect_light():
    """Rectangle lights with extent over a Phong floor. Light 0 (red, the only red one) hangs over a plate:
    floor pixels fully lit by it, in its penumbra (the red channel present in some samples of a pixel and not
    in others) and in its umbra. Lights 0 and 1 share one Philox draw (words 0-1 and 2-3); light 1 is a shape of
    the scene too (the own-shape skip with real sampling); lights 2 and 3 are point lights; light 4 is a
    rectangle light at an even index, with a draw of its own. 16 x 8 at 4 spp."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.9, 0.9, 0.9), flags=0)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.6, 0.9, 0.9), flags=0)
    _cylinder(b, (1.5, 0, 0.5), (1.5, 1.5, 0.5), 0.5, (0.95, 0.64, 0.54))
    _rect(b, (-2.5, 2.0, 2.0), (-0.5, 2.0, 2.0), (-0.5, 2.0, 0.0), (-2.5, 2.0, 0.0), (0.7, 0.7, 0.75), flags=0)
    _rect_light(b, (-2.0, 3.5, 1.5), (-1.0, 3.5, 1.5), (-2.0, 3.5, 0.5), (0.5, 0.0, 0.0))
    _rect_light(b, (1.0, 3.5, 0.5), (2.5, 3.5, 0.5), (1.0, 3.5, -1.0), (0.0, 0.4, 0.0), shape=True)
    b.light(POINT_LIGHT, center=(3.0, 3.0, 3.0), color=(0.0, 0.0, 0.3))
    b.light(POINT_LIGHT, center=(-3.5, 1.0, 3.0), color=(0.0, 0.0, 0.2))
    _rect_light(b, (3.9, 1.0, -1.0), (3.9, 1.0, -2.5), (3.9, 2.5, -1.0), (0.0, 0.25, 0.25))
    return _sampling_globals(b, b.globals(*_CAMERA), (16, 8), 4, 3, 2)


def sampling_sphere_light():
    """Sphere lights with a radius over a Phong floor and wall. sampleRay returns the sampled POINT (Q11): the
    shadow ray leaves the surface in the direction of that position vector. Light 0 (red) has no baxis: half of
    its first draws face away and the mirror image is taken. Light 1 (blue) has baxis = -y and hangs to the side,
    so that for floor points away from it neither the draw nor its mirror image passes both tests and it draws
    again. Light 2 (green) is the sphere shape at (0, 3, 0): from a floor point near the origin the segment
    along the sampled position vector ends inside or behind that very sphere, so those points are green only
    because the light's own sphere is skipped."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.9, 0.9, 0.9), flags=0)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.6, 0.9, 0.9), flags=0)
    _cylinder(b, (-1.5, 0, -1.0), (-1.5, 1.5, -1.0), 0.5, (0.95, 0.64, 0.54))
    sl = b.shape(SPHERE, v=[(0.0, 3.0, 0.0)], radius=1.0, color=(0.6, 0.6, 0.5), emit=1, flags=F_LIGHT,
                 center=(0.0, 3.0, 0.0))
    b.light(SPHERE_LIGHT, -1, 0.75, center=(-2.0, 2.0, 1.0), color=(0.5, 0.0, 0.0))
    b.light(SPHERE_LIGHT, -1, 0.5, center=(3.0, 2.5, 1.0), color=(0.0, 0.0, 0.5), baxis=(0.0, -1.0, 0.0))
    b.light(SPHERE_LIGHT, sl, 1.0, center=(0.0, 3.0, 0.0), color=(0.0, 0.5, 0.0))
    return _sampling_globals(b, b.globals(*_CAMERA), (32, 16), 1, 3, 2)


def sampling_glossy():
    """Glossy reflectors with nogloss = 0 under point lights: every draw is a glossy sample's. The camera looks
    level along -x from (6, 0.375, 0) with depth of field off: the floor is seen from steep (near) to grazing (far,
    where the squeeze loops move the vertices of the sample rectangle and samples below the surface force the
    resample loop); the wall at x = -4 has an x-normal, and the ray of pixel (W/2, H/2) is exactly (-c, 0, 0),
    so that gloss_ray x (1, 0, 0) vanishes and the isApprox fallback runs. 8 x 16 at 4 spp (rows 0.05 apart in slope): without a lens the
    four samples of a pixel are one ray with four draw sequences."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (8, 0, 4), (8, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=F_GLOSSY, **_GLOSSY_KW)
    _rect(b, (-4, 0, 4), (-4, 0, -4), (-4, 4, -4), (-4, 4, 4), (0.9, 0.8, 0.3), flags=F_GLOSSY, **_GLOSSY_KW)
    _rect(b, (-4, 0, -4), (8, 0, -4), (8, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99), flags=0)
    _cylinder(b, (0.0, 0, 2.0), (0.0, 1.5, 2.0), 0.5, (0.9, 0.3, 0.2))
    _cylinder(b, (2.0, 0, -2.0), (2.0, 2.0, -2.0), 0.5, (0.3, 0.9, 0.4))
    b.light(POINT_LIGHT, center=(2.0, 3.5, 2.0), color=(0.4, 0.4, 0.4))
    b.light(POINT_LIGHT, center=(0.0, 3.0, -3.0), color=(0.3, 0.3, 0.3))
    return _sampling_globals(b, b.globals((6.0, 0.375, 0.0), (0.0, 0.375, 0.0), 0.0, 6.0), (8, 16), 4, 3, 3)


def sampling_glossy_area(triangle=False, res=(32, 16), spp=1):
    """Glossy children landing on surfaces lit by rectangle lights: a glossy floor and a glossy side wall (two
    levels of k / brdf_samples at depth 4), a plain back wall and a Cook-Torrance cylinder (the one user of
    the float libm in these classes), a rectangle light with extent
    that is a shape and one that is not. The draws happen at child node keys. triangle=True: the mesh twin."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=F_GLOSSY, **_GLOSSY_KW)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99), flags=0)
    _rect(b, (4, 0, -4), (4, 0, 4), (4, 4, 4), (4, 4, -4), (0.9, 0.8, 0.3), flags=F_GLOSSY, **_GLOSSY_KW)
    _cylinder(b, (-1.5, 0, 0.5), (-1.5, 1.5, 0.5), 0.5, (0.95, 0.64, 0.54), model=COOK_TORRANCE,
              **_MODEL_KW[COOK_TORRANCE])
    if triangle:
        _triangle(b, (0.5, 0.25, 1.0), (2.0, 0.25, 1.5), (1.25, 2.0, 0.5), (0.2, 0.8, 0.3))
    _rect_light(b, (-1.0, 3.75, 1.0), (1.0, 3.75, 1.0), (-1.0, 3.75, -1.0), (0.45, 0.45, 0.4), shape=True)
    _rect_light(b, (-3.9, 1.0, 2.0), (-3.9, 1.0, 0.5), (-3.9, 2.5, 2.0), (0.3, 0.25, 0.3))
    return _sampling_globals(b, b.globals(*_CAMERA), res, spp, 4, 2)


def sampling_in_motion():
    """in_motion, which every deeper rayColor call overwrites: a moving cylinder seen directly; a static steel
    panel showing it; a MOVING steel cylinder showing static walls; a glossy floor whose last sample decides.
    Point lights: every draw is a glossy sample's."""
    b = _Builder(1.0, (0.0, 0.0, 0.0))
    _rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0), flags=F_GLOSSY, **_GLOSSY_KW)
    _rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99), flags=0)
    _rect(b, (-3.0, 0.5, -3.5), (-0.5, 0.5, -3.0), (-0.5, 3.0, -3.0), (-3.0, 3.0, -3.5), (0.8, 0.8, 0.8), flags=0,
          material=STEEL)
    _cylinder(b, (-2.0, 0, -0.5), (-2.0, 1.75, -0.5), 0.5, (0.9, 0.3, 0.2), flags=F_MOTION)
    _cylinder(b, (0.5, 0.5, 1.0), (2.5, 0.5, 0.0), 0.5, (0.8, 0.8, 0.8), material=STEEL, flags=F_MOTION)
    _cylinder(b, (2.5, 0, -2.0), (2.5, 1.5, -2.0), 0.5, (0.3, 0.9, 0.4))
    b.light(POINT_LIGHT, center=(-2.5, 3.5, 2.5), color=(0.4, 0.4, 0.4))
    b.light(POINT_LIGHT, center=(3.0, 3.0, 3.0), color=(0.3, 0.3, 0.3))
    return _sampling_globals(b, b.globals(*_CAMERA), (32, 16), 1, 4, 2)


# class name -> scene function (the wave5 twins: 8 x 4 at 64 spp, the smallest image of the 5-wave builds)
SAMPLING_SCENES = {
    "rect-light": sampling_rect_light,
    "sphere-light": sampling_sphere_light,
    "glossy": sampling_glossy,
    "glossy-area": sampling_glossy_area,
    "in-motion": sampling_in_motion,
    "wave5-glossy-area": lambda: sampling_glossy_area(res=(8, 4), spp=64),
    "wave5-glossy-area-mesh": lambda: sampling_glossy_area(triangle=True, res=(8, 4), spp=64),
}
