"""Restatements for dt_camera_rays and dt_rays_resolve (include/dt.h), in numpy and plain Python.

resolve_ref: per owned pixel and component a sequential f64 sum in a Python loop over samples (Python floats are
IEEE doubles, one rounded operation per +), one f64 division, one cast to float32.
owned_slots: which output slots a tile share owns, from dt_tiles' rule restated (dt_scene_dev.h tile_of).
ray_numbers: the number, in dt_intersect_primary's (or_primary_ray's) numbering, of every row of dt_camera_rays."""
import numpy as np


def _tile_rot(slot, world):
    h = (slot * 2654435761) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2c1b3c6d) & 0xFFFFFFFF
    h ^= h >> 12
    return h % world


def tile_of(slot, rank, world):
    return slot * world + (rank + _tile_rot(slot, world)) % world


def slot_pixels(g, tile=None):
    """(x, y, owned) per output slot: int arrays of accum_doubles // 3 entries. x, y are -1 where a slab slot
    holds no pixel of the window."""
    W, H = g.xRes, g.yRes
    if tile is None:
        x0, y0, x1, y1, tw, th, rank, world, layout = 0, 0, W, H, 32, 32, 0, 1, 0
    else:
        x0, y0 = max(tile.x0, 0), max(tile.y0, 0)
        x1 = min(tile.x1, W) if tile.x1 > 0 else W
        y1 = min(tile.y1, H) if tile.y1 > 0 else H
        tw, th = tile.tile_w or 32, tile.tile_h or 32
        rank, world, layout = tile.rank, max(tile.world, 1), tile.layout
    tiles_x = (x1 - x0 + tw - 1) // tw
    tiles_y = (y1 - y0 + th - 1) // th
    n_tiles = tiles_x * tiles_y
    n_owned = (n_tiles + world - 1) // world
    if layout:   # slab: tile slots in turn, row-major inside the tile
        xs, ys, own = [], [], []
        for slot in range(n_owned):
            t = tile_of(slot, rank, world)
            ty, tx = divmod(t, tiles_x)
            for py in range(th):
                for px in range(tw):
                    x, y = x0 + tx * tw + px, y0 + ty * th + py
                    ok = t < n_tiles and x < x1 and y < y1
                    xs.append(x if ok else -1)
                    ys.append(y if ok else -1)
                    own.append(ok)
        return np.array(xs), np.array(ys), np.array(own, bool)
    q = np.arange(W * H)
    x, y = q % W, H - 1 - q // W
    own = np.zeros(W * H, bool)
    for i in range(W * H):
        if x0 <= x[i] < x1 and y0 <= y[i] < y1:
            t = ((y[i] - y0) // th) * tiles_x + (x[i] - x0) // tw
            own[i] = tile_of(t // world, rank, world) == t
    return x, y, own


def ray_numbers(g, samples, tile=None):
    """(numbers, owned): per row (slots, ns) of dt_camera_rays the ray's number ((i/8)*W*H + y*W + x)*8 + i%8,
    and which rows are written"""
    x, y, own = slot_pixels(g, tile)
    W, H = g.xRes, g.yRes
    i = np.arange(samples[0], samples[1])[None, :]
    num = ((i // 8) * W * H + y[:, None] * W + x[:, None]) * 8 + i % 8
    return np.where(own[:, None], num, 0), np.repeat(own[:, None], i.shape[1], axis=1)


def resolve_ref(values, n, width, shape=None, mode="mean", owned=None, out=None, coverage=None):
    """(plane (slots, width) float32, coverage (slots,) float32); unowned slots keep out's / coverage's values
    (zeros without them)"""
    v = np.asarray(values, np.float64).reshape(-1, n, width)
    slots = v.shape[0]
    sh = None if shape is None else np.asarray(shape, np.int32).reshape(slots, n)
    plane = np.zeros((slots, width), np.float32) if out is None else np.array(out, np.float32).reshape(slots, width)
    cov = np.zeros(slots, np.float32) if coverage is None else np.array(coverage, np.float32).reshape(slots)
    for q in range(slots):
        if owned is not None and not owned[q]:
            continue
        H = 0
        S = [0.0] * width
        for i in range(n):
            if sh is not None and sh[q, i] < 0:
                continue
            for k in range(width):
                S[k] = S[k] + float(v[q, i, k])
            H += 1
        for k in range(width):
            if mode == "mean":
                plane[q, k] = np.float32(S[k] / float(n))
            else:
                plane[q, k] = np.float32(S[k] / float(H)) if H > 0 else np.float32(0)
        cov[q] = np.float32(float(H) / float(n))
    return plane, cov
