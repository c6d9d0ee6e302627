"""Object mattes restated in numpy (include/dt.h dt_render_mattes and dt_matte_mask; a plain helper module,
imported by tests/test_mattes_host.py and tests/test_gpu_mattes.py).

The input is ids[pixel, sample]: the shape every sample's primary ray hit (-1: a miss), and optionally a group
per shape. Everything is integer work but the weight, one f64 division rounded to f32, and the mask, f32
additions in layer order, so the host loop, the kernel and this file must agree in every bit."""
import numpy as np

TABLE = 64        # DT_MATTE_TABLE
MAX_LAYERS = 8    # DT_MATTE_MAX_LAYERS


def pixel_table(groups, table=TABLE):
    """The histogram rule, one sample after the other: ([group, count] in insertion order, overflowed?).
    groups: the pixel's samples in ascending sample order, -1 a miss."""
    entries, where, over = [], {}, False
    for gid in groups:
        gid = int(gid)
        if gid < 0:
            continue
        if gid in where:
            entries[where[gid]][1] += 1
        elif len(entries) < table:
            where[gid] = len(entries)
            entries.append([gid, 1])
        else:
            over = True   # dropped
    return entries, over


def rank(entries):
    """count descending, ties by group ascending"""
    return sorted(entries, key=lambda e: (-e[1], e[0]))


def mattes(ids, n_samples, layers, group_of_shape=None, table=TABLE):
    """ids: (n_pixels, >= n_samples) integers. Returns {"id": (n_pixels, layers) int32, "weight": the same
    shape float32, "distinct": (n_pixels,) int32, "overflow": (n_pixels,) bool}."""
    ids = np.asarray(ids)[:, :n_samples]
    assert ids.shape[1] == n_samples and 1 <= layers <= MAX_LAYERS
    if group_of_shape is not None:
        gm = np.asarray(group_of_shape)
        assert (gm >= 0).all()
        ids = np.where(ids >= 0, gm[np.maximum(ids, 0)], -1)
    n_px = ids.shape[0]
    out = {"id": np.full((n_px, layers), -1, np.int32), "weight": np.zeros((n_px, layers), np.float32),
           "distinct": np.zeros(n_px, np.int32), "overflow": np.zeros(n_px, bool)}
    for p in range(n_px):
        entries, over = pixel_table(ids[p], table)
        out["distinct"][p] = len(entries)
        out["overflow"][p] = over
        for j, (gid, c) in enumerate(rank(entries)[:layers]):
            out["id"][p, j] = gid
            out["weight"][p, j] = np.float32(np.float64(c) / np.float64(n_samples))
    return out


def matte_mask(ids, weight, groups):
    """mask[q]: the f32 sum, from 0, in layer order, of the weights of the layers whose id is in groups"""
    ids, weight = np.asarray(ids), np.asarray(weight, np.float32)
    groups = np.atleast_1d(np.asarray(groups))
    assert ids.shape == weight.shape and ids.ndim == 2 and (groups >= 0).all()
    m = np.zeros(ids.shape[0], np.float32)
    for j in range(ids.shape[1]):
        sel = (ids[:, j] >= 0) & np.isin(ids[:, j], groups)
        m = np.where(sel, m + weight[:, j], m).astype(np.float32)
    return m


def pixel_ids(hit_shape, W, H, n_samples):
    """dt_intersect_primary's (or or_primary_hit's) hit shapes of rays 0 .. ceil(n/8)*W*H*8 - 1, regrouped per
    pixel: sample i of pixel (x, y) is ray ((i/8)*W*H + y*W + x)*8 + i%8. Returns (H*W, n_samples), pixel
    (x, y) in row y*W + x."""
    nb = (n_samples + 7) // 8
    a = np.asarray(hit_shape).reshape(nb, H, W, 8).transpose(1, 2, 0, 3).reshape(H * W, nb * 8)
    return a[:, :n_samples]


def defocus(g):
    """The renders' primary rays of one pixel differ only in their lens sample: in a sharp image every sample
    of a pixel hits the same shape. A wide lens focused well in front of tests/scene_gen.py's scenes blurs the
    silhouettes over several pixels, so that a pixel holds up to four shapes."""
    g.aperture, g.focal_length = 0.6, 2.0
    return g
