"""The numpy restatement of the ray-ordering key (include/dt.h dt_ray_order, csrc/dt_order.h): void rays, the
box, the origin and direction cells, the Morton packing, and the order as argsort(kind="stable"). Every
operation is one rounded f64 operation in the parenthesisation the header writes, so the keys equal the
library's by bit pattern. Shared by tests/test_rayorder_host.py and tests/test_gpu_rayorder.py, with the
inputs both use."""
import numpy as np


def void_rays(start, dir):
    return ~(np.isfinite(start).all(axis=1) & np.isfinite(dir).all(axis=1)) | (dir == 0).all(axis=1)


def box_of(start, dir):
    """(lo, hi): min and max of the non-void starts, a -0 reported as +0; no such ray: zeros"""
    live = ~void_rays(start, dir)
    if not live.any():
        return np.zeros(3), np.zeros(3)
    return start[live].min(axis=0) + 0.0, start[live].max(axis=0) + 0.0


def _cell(f, bits):
    with np.errstate(invalid="ignore"):
        scaled = np.where((f > 0) & (f < 1), f, 0.0) * float(1 << bits)
        c = scaled.astype(np.uint32)
        c = np.where(f >= 1, np.uint32((1 << bits) - 1), c)
        return np.where(f > 0, c, np.uint32(0)).astype(np.uint32)


def _spread(c, bits, stride, k):
    m = np.zeros(c.shape, np.uint32)
    for i in range(bits):
        m |= ((c >> np.uint32(i)) & np.uint32(1)) << np.uint32(stride * i + k)
    return m


def keys_of(start, dir, origin_bits, dir_bits, dir_major, lo, hi):
    start, dir = np.asarray(start, np.float64).reshape(-1, 3), np.asarray(dir, np.float64).reshape(-1, 3)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ob, db = int(origin_bits), int(dir_bits)
    with np.errstate(all="ignore"):
        M3 = np.zeros(len(start), np.uint32)
        for k in range(3):
            e = hi[k] - lo[k]
            f = (start[:, k] - lo[k]) / e if e > 0 else np.zeros(len(start))
            M3 |= _spread(_cell(f, ob), ob, 3, k)
        s = (np.abs(dir[:, 0]) + np.abs(dir[:, 1])) + np.abs(dir[:, 2])
        u, v = dir[:, 0] / s, dir[:, 1] / s
        fu = (1.0 - np.abs(v)) * np.where(u >= 0, 1.0, -1.0)
        fv = (1.0 - np.abs(u)) * np.where(v >= 0, 1.0, -1.0)
        neg = dir[:, 2] < 0
        u, v = np.where(neg, fu, u), np.where(neg, fv, v)
        gu, gv = u * 0.5 + 0.5, v * 0.5 + 0.5
        M2 = _spread(_cell(gu, db), db, 2, 0) | _spread(_cell(gv, db), db, 2, 1)
    key = (M2 << np.uint32(3 * ob)) | M3 if dir_major else (M3 << np.uint32(2 * db)) | M2
    return np.where(void_rays(start, dir), np.uint32(1 << (3 * ob + 2 * db)), key).astype(np.uint32)


def order_of(keys):
    return np.argsort(keys, kind="stable").astype(np.uint32)


# the bit configurations of the tests: (origin_bits, dir_bits, dir_major)
CONFIGS = [(5, 6, 0), (0, 8, 0), (0, 8, 1), (10, 0, 0), (10, 0, 1), (1, 0, 0), (1, 0, 1), (5, 6, 1), (2, 3, 1)]


def hand_made_rays():
    """(start, dir, tags): the hand-made vectors of the issue, tags naming what each row is there for"""
    S, D, T = [], [], []

    def add(tag, s, d):
        S.append(s)
        D.append(d)
        T.append(tag)

    inf, nan, big = np.inf, np.nan, 1.5e308
    add("void nan start", (nan, 0.0, 0.0), (1.0, 0.0, 0.0))
    add("void inf start", (0.0, -inf, 0.0), (1.0, 2.0, 3.0))
    add("void nan dir", (1.0, 2.0, 3.0), (0.0, nan, 1.0))
    add("void inf dir", (1.0, 2.0, 3.0), (0.0, 1.0, inf))
    add("void zero dir", (1.0, 2.0, 3.0), (0.0, -0.0, 0.0))
    for d in ((0.3, -0.2, -0.9), (-0.5, 0.5, -0.1), (-0.0, 0.25, -4.0), (1e-300, -1e-300, -1e-300)):
        add("dz < 0", (0.5, 1.5, -2.5), d)
    for axis in range(3):
        for sign in (1.0, -1.0):
            d = [0.0, 0.0, 0.0]
            d[axis] = sign * 2.5
            add("axis-aligned", (-3.0, 0.25, 7.0), tuple(d))
    add("u = 1", (0.0, 0.0, 0.0), (3.0, 0.0, 0.0))
    add("u = -1", (0.0, 0.0, 0.0), (-3.0, 0.0, -0.0))
    add("v = 1", (0.0, 0.0, 0.0), (0.0, 0.125, 0.0))
    add("v = -1", (0.0, 0.0, 0.0), (-0.0, -7.0, 0.0))
    add("huge s", (1.0, 1.0, 1.0), (big, big, -big))
    add("huge s", (1.0, 1.0, 1.0), (-big, 1.0, big))
    add("huge o - lo", (big, -big, big), (0.1, 0.2, 0.3))
    add("huge o - lo", (-big, big, -big), (0.1, -0.2, -0.3))
    add("plain", (9.75, 0.3, -5.0), (1.0, 1.0, 1.0))
    add("plain", (-10.0, 10.3, 8.0), (-1.0, -1.0, 1.0))
    return np.array(S, np.float64), np.array(D, np.float64), np.array(T)


def scattered_rays():
    """the 4096 + 37 scattered rays of tests/test_gpu_rayquery.py's recipe, rebuilt from or_primary_ray: rays of
    seven cameras in and around the room of final(240), in one fixed permutation"""
    import distraytracer_amd as dt
    from oracle import geom as G
    from test_gpu_features import MIXED_AT, MIXED_EYE
    cameras = [(MIXED_EYE, MIXED_AT), (None, None), ((0.0, 4.0, 6.0), (0.75, 1.0, 0.65)),
               ((-8.0, 2.0, 6.0), (5.0, 3.0, -4.0)), ((5.0, 9.0, 0.0), (0.0, 0.3, 2.0)),
               ((0.0, 1.0, -3.0), (2.3, 10.25, 3.8)), ((15.0, 5.0, 20.0), (0.0, 5.0, 0.0))]
    n = 4096 + 37
    g = dt.globals_default()
    g.use_model = 0
    g.xRes, g.yRes = 1920, 1080
    starts, dirs = [], []
    per = -(-n // len(cameras))
    for eye, at in cameras:
        gc = g.copy()
        gc.xRes, gc.yRes = 40, 24
        if eye is not None:
            for a in range(3):
                gc.eye[a], gc.lookingAt[a] = eye[a], at[a]
        s, d = G.or_primary_ray(gc, 240, 0, 40 * 24 * 8)
        pick = np.linspace(0, len(s) - 1, per).astype(int)
        starts.append(s[pick])
        dirs.append(d[pick])
    perm = np.random.default_rng(20240).permutation(per * len(cameras))[:n]
    return np.ascontiguousarray(np.concatenate(starts)[perm]), np.ascontiguousarray(np.concatenate(dirs)[perm])


def key_inputs():
    """(name, start, dir, given box or None) for the key tests: the scattered rays, the hand-made vectors with the
    box from the rays (huge starts: e overflows) and inside a given box (starts outside on either side), the
    hand-made vectors without the huge starts, all starts equal, and void rays only"""
    ss, sd = scattered_rays()
    hs, hd, tags = hand_made_rays()
    small = np.array([not t.startswith("huge o") for t in tags])
    eq_s = np.tile(np.array([[1.25, -2.5, 3.0]]), (len(hd), 1))
    room = (np.array([-10.0, 0.3, -5.0]), np.array([10.0, 10.3, 8.0]))
    return [("scattered", ss, sd, None), ("scattered in the room's box", ss, sd, room),
            ("hand-made", hs, hd, None), ("hand-made in the room's box", hs, hd, room),
            ("hand-made, moderate starts", np.ascontiguousarray(hs[small]), np.ascontiguousarray(hd[small]), None),
            ("all starts equal", eq_s, hd.copy(), None),
            ("void only", np.ascontiguousarray(hs[:5]), np.ascontiguousarray(hd[:5]), None)]
