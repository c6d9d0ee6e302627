"""The device's fused length and normalisation (dt_math.h vnorm_fused: sqrt's own refinement restated, the
division's reciprocal taken from it instead of a second transcendental; plain sqrt and divisions in a branch
out of range) against plain sqrt and three plain divisions on the device, bit for bit (dt_debug_vnorm), and
both against numpy's correctly rounded float64 results. Then the product path against the oracle on one
shape of each BRDF model and on a rectangle light of a shifted, scaled scene (DLight's edge vectors), at 64
spp: the 5-wave room and mesh builds, which have DT_VNORM on.

The in-range test of vnorm_fused is 2^-600 <= d < 2^600 for d = (x*x + y*y) + z*z and 2^-600 <= |n| for each
component; the compiler's sqrt scales below d = 2^-767. The inputs put sums and components on both sides of
each of these."""
import ctypes

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
import scene_gen as sg
from parity_check import assert_parity

pytestmark = pytest.mark.gpu

INF, NAN = np.inf, np.nan
SUB = 5e-324          # the smallest subnormal
LO, HI, SQRT_SCALE = 2.0 ** -600, 2.0 ** 600, 2.0 ** -767
HAND = [
    (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, 1.0, 2.0), (-0.0, 1.0, 2.0), (3.0, 4.0, 0.0),
    (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 0.1), (-7.5, 0.0, -0.0), (1e-160, 0.0, 0.0), (0.0, 1e200, 0.0),
    (SUB, SUB, SUB), (1e-310, -2e-320, SUB), (SUB, 1.0, 2.0), (1e-162, 1e-162, 1e-162), (3e-162, -1e-162, 2e-162),
    (1e-160, 1e-161, 1e-162), (1e-155, 1e-155, 1e-155),
    (1e300, 1e300, 1e300), (1e154, 1e154, 1e154), (1e300, 1.0, 1.0), (2.0 ** 1000, 2.0 ** -1000, 1.0),
    (1e-300, 1e-300, 1e-300), (1.0, 1e-300, 1.0), (1.0, 1.0, 1e-300),
    (INF, 1.0, 2.0), (-INF, 1.0, 2.0), (1.0, INF, -INF), (NAN, 1.0, 2.0), (1.0, 2.0, NAN), (INF, NAN, 0.0),
    (LO, 1.0, 1.0), (np.nextafter(LO, 0.0), 1.0, 1.0), (1.0, -LO, 1.0), (1.0, -np.nextafter(LO, 0.0), 1.0),
    (1.0, 1.0, LO), (1.0, 1.0, np.nextafter(LO, 0.0)), (LO, LO, LO), (2.0 ** -300, LO, LO),
]
N_ROOM, N_WILD, N_MIXED = 4096, 16384, 24576


def _random_doubles(rng, shape):
    """sign, exponent field (1..2046: every normal binade) and fraction drawn independently"""
    bits = (rng.integers(0, 2, size=shape, dtype=np.uint64) << np.uint64(63)
            | rng.integers(1, 2047, size=shape, dtype=np.uint64) << np.uint64(52)
            | rng.integers(0, 1 << 52, size=shape, dtype=np.uint64))
    return bits.view(np.float64)


def _dot(v):
    with np.errstate(all="ignore"):
        return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def _around(rng, threshold, n):
    """n vectors of random direction (no component below a thousandth of the length) whose sum of squares
    lies within a few ulps of threshold, on both sides"""
    d = rng.uniform(0.2, 1.0, size=(n, 3)) * rng.choice([-1.0, 1.0], size=(n, 3))
    v = d * (np.sqrt(threshold) / np.sqrt(_dot(d)))[:, None]
    for _ in range(4):                                    # pull the rounded sum onto the threshold
        v *= np.sqrt(threshold / _dot(v))[:, None]
    steps = rng.integers(-3, 4, size=n)
    x = v[:, 0].copy()
    for k in range(1, 4):
        x = np.where(steps >= k, np.nextafter(x, np.sign(x) * INF), x)
        x = np.where(steps <= -k, np.nextafter(x, 0.0), x)
    v[:, 0] = x
    return v


def _room(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    return d * 10.0 ** rng.uniform(-3, np.log10(30.0), size=(n, 1))


def _inputs():
    rng = np.random.default_rng(21)
    room = _room(rng, N_ROOM)
    wild = _random_doubles(rng, (N_WILD, 3))
    mixed = _room(rng, N_MIXED) * 10.0 ** rng.uniform(-3, 3, size=(N_MIXED, 1))
    sub = _room(rng, 1024) * 2.0 ** rng.integers(-536, -514, size=(1024, 1)).astype(np.float64)   # subnormal sums
    edges = np.concatenate([_around(rng, t, 1024) for t in (LO, HI, SQRT_SCALE)])
    hand = np.array(HAND * 5)   # (5 copies: the shuffle below drops them into several waves)
    v = np.concatenate([wild, mixed, sub, edges, hand])
    v = np.concatenate([room, v[rng.permutation(len(v))]])   # the room's vectors first, in waves of their own
    assert len(v) <= 1 << 16 and len(v) % 64 != 0
    return np.ascontiguousarray(v)


def _debug_vnorm(v):
    out = np.empty((2, len(v), 4), dtype=np.float64)
    fb = (ctypes.c_uint64 * 1)()
    PD = ctypes.POINTER(ctypes.c_double)
    dt.check(dt.lib.dt_debug_vnorm(v.ctypes.data_as(PD), out.ctypes.data_as(PD), fb, len(v)), "dt_debug_vnorm")
    return out[0], out[1], int(fb[0])


@pytest.fixture(scope="module")
def run(cuda):
    v = _inputs()
    d = _dot(v)
    with np.errstate(all="ignore"):
        ref = np.empty((len(v), 4))
        ref[:, 0] = np.sqrt(d)
        ref[:, 1:] = v
        pos = d > 0
        ref[pos, 1:] = v[pos] / ref[pos, :1]
    fused, plain, fb = _debug_vnorm(v)
    _, _, fb_room = _debug_vnorm(np.ascontiguousarray(v[:N_ROOM]))
    for a in (v, d, ref, fused, plain):
        a.setflags(write=False)
    return {"v": v, "d": d, "ref": ref, "fused": fused, "plain": plain, "fallback": fb, "fallback_room": fb_room}


def _first(bad, run, a, b):
    i = int(np.argmax(bad.any(axis=1)))
    return "%d differ; first: %r (d = %r) -> %r vs %r" % (bad.any(axis=1).sum(), run["v"][i], run["d"][i], a[i], b[i])


def test_inputs_straddle_the_thresholds(run):
    """sums of squares just below and just above each bound; components below and on theirs; subnormal sums"""
    v, d = run["v"], run["d"]
    for t in (LO, HI, SQRT_SCALE):
        near = (d > t * (1 - 1e-12)) & (d < t * (1 + 1e-12))
        assert (d[near] < t).any() and (d[near] > t).any(), t
    assert ((d > 0) & (d < 2.0 ** -1022)).sum() > 50
    a = np.abs(v)
    assert (a == LO).any() and (a == np.nextafter(LO, 0.0)).any()


def test_fused_equals_plain_bit_for_bit(run):
    """the length and the three quotients, NaNs by payload"""
    a, b = run["fused"], run["plain"]
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), _first(bad, run, a, b)


@pytest.mark.parametrize("path", ["fused", "plain"])
def test_equals_numpy(run, path):
    """correctly rounded: numpy's float64 sqrt and quotients bit for bit (a NaN for a NaN)"""
    a, b = run[path], run["ref"]
    bad = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), _first(bad, run, a, b)


def test_fallback_share(run):
    """no vector of the room's scale (lengths 1e-3 to 30) leaves the fused path; of the whole set exactly the
    vectors outside the bounds do, and the fused path runs"""
    v, d, n = run["v"], run["d"], len(run["v"])
    in_range = (d >= LO) & (d < HI) & (np.abs(v) >= LO).all(axis=1)
    print("fallback: %d of %d vectors (expected %d); room scale: %d of %d" % (
        run["fallback"], n, int((~in_range).sum()), run["fallback_room"], N_ROOM))
    assert run["fallback_room"] == 0
    assert 0 < run["fallback"] < n
    assert run["fallback"] == int((~in_range).sum())


# ---- the product path against the oracle -----------------------------------------------------------------

def _scene(model, s, t):
    """A floor, a back wall and one standing cylinder of the given BRDF model under a rectangle light and a
    point light: shapes of the room builds, or with Oren-Nayar of the mesh builds"""
    b = sg._Builder(s, t)
    sg._rect(b, (-4, 0, 4), (4, 0, 4), (4, 0, -4), (-4, 0, -4), (0.58, 0.82, 1.0))
    sg._rect(b, (-4, 0, -4), (4, 0, -4), (4, 4, -4), (-4, 4, -4), (0.0, 0.81, 0.99))
    kw = {sg.PHONG: {}, sg.COOK_TORRANCE: dict(roughness=0.4, refr=(2.75, 3.79)), sg.OREN_NAYAR: dict(roughness=0.3)}[model]
    sg._cylinder(b, (0.25, 0, 0.5), (0.25, 2.0, 0.5), 1.0, (0.95, 0.64, 0.54), model=model, **kw)
    ra, rb, rc, rd = (1.5, 3.75, 2.5), (2.5, 3.75, 2.5), (2.5, 3.75, 1.25), (1.5, 3.75, 1.25)
    rl = b.shape(sg.RECTANGLE, v=[ra, rb, rc, rd], color=(0.8, 0.8, 0.8), emit=2, flags=sg.F_LIGHT, length=1.0,
                 width=1.25, center=(2.0, 3.75, 1.875))
    b.light(sg.RECT_LIGHT, rl, center=(2.0, 3.75, 1.875), color=(0.7, 0.7, 0.7), A=ra, B=rb, D=rd)
    b.light(sg.POINT_LIGHT, center=(-3.0, 3.0, 3.0), color=(0.6, 0.6, 0.6))
    g = b.globals((0.5, 1.25, 6.5), (0.0, 0.75, 0.0), 0.0625, 6.0)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth, g.brdf_samples = 32, 18, 64, 4, 2
    desc, keep = b.desc()
    return desc, g, keep


@pytest.mark.parametrize("name,model,case", [("phong", sg.PHONG, "unit"), ("cook-torrance", sg.COOK_TORRANCE, "unit"),
                                             ("oren-nayar", sg.OREN_NAYAR, "unit"),
                                             ("rect-light-tiny-shifted", sg.PHONG, "tiny-shifted")])
def test_product_path_matches_the_oracle(cuda, name, model, case):
    """32x18 at 64 spp: the largest channel difference 0, the same rays and shadow rays"""
    desc, g, keep = _scene(model, *sg.CASES[case])
    scene = dt.Scene(desc, g)
    try:
        out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        st = dt.render(scene, g, 0, out, dt.tiles())
        gpu = out.cpu().numpy()
    finally:
        scene.close()
    ref, rst = oracle.render(desc, g, 0, dt.tiles())
    print("%s: rays %d/%d shadow %d/%d" % (name, st.rays, rst.rays, st.shadow_rays, rst.shadow_rays))
    assert st.rays == rst.rays and st.shadow_rays == rst.shadow_rays and st.shadow_rays > 0
    assert assert_parity("vnorm %s 32x18 64 spp vs oracle" % name, gpu, ref) == 0.0
