"""First-hit feature buffers (include/dt.h dt_render_features; dt_features_kernel) against a prediction
made on the CPU from the oracle's exports alone, bit for bit.

The prediction (predict below): the call's samples are primary rays of dt_intersect_primary's numbering
(sample i of pixel (x, y) is ray ((i/8)*W*H + y*W + x)*8 + i%8), so or_primary_ray gives their start and
direction and or_primary_hit their closest shape and t. For a hit, or_shape_intersect (the hole),
or_shape_color_after_hit (the colour intersect() leaves behind), or_shape_norm at p = start + t * ray,
or_fix_norm with the normalised ray, and for textured shapes or_shape_uv and the texel lookup of
oracle.c's light loop restated in numpy float32. The sums are Python floats (f64) added left to right
in sample order; a miss adds nothing.

All comparisons are by bit pattern (oracle.geom.differs); shape ids as integers."""
import ctypes
import math
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
from oracle import geom as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTRENDER = os.path.join(os.path.dirname(HERE), "distraytracer_amd", "dtrender")
F_TEXTURE = 1 << 2
PLANES = ("albedo", "normal", "depth", "coverage", "shape")


def _desc(built):
    return built.desc if hasattr(built, "desc") else built


def _texel(desc, sh, u, v):
    """oracle.c's light loop: float products, truncation, the clamped index, byte / 255.0"""
    T = desc.textures[sh.tex_frame]
    f32 = np.float32
    x_tex = int(f32(T.width - 1) * f32(u))
    y_tex = int(f32(T.height - 1) * f32(v))
    ind = int(y_tex * float(T.width) + x_tex)
    ind = min(max(ind, 0), T.width * T.height - 1)
    return [T.pixels[ind * T.channels + k] / 255.0 for k in range(3)]


def predict(built, g, frame, n):
    """{plane: array in image order (pixel (x, y) at entry y*W + x)} plus the counts and kinds of hits seen"""
    desc = _desc(built)
    W, H = g.xRes, g.yRes
    nb = (n + 7) // 8
    start, ray = G.or_primary_ray(g, frame, 0, nb * W * H * 8)
    shape, t = oracle.primary_hit(built, g, frame, 0, nb * W * H * 8)
    start, ray = start.reshape(nb, H, W, 8, 3), ray.reshape(nb, H, W, 8, 3)
    shape, t = shape.reshape(nb, H, W, 8), t.reshape(nb, H, W, 8)
    rec, hrec = G.records_from_desc(desc)
    orc = G.Oracle(rec, hrec)
    out = {"albedo": np.zeros((H, W, 3), np.float32), "normal": np.zeros((H, W, 3), np.float32),
           "depth": np.zeros((H, W), np.float32), "coverage": np.zeros((H, W), np.float32),
           "shape": np.full((H, W), -1, np.int32)}
    seen = {"tex_fetches": 0, "uv_out_of_range": 0, "textured": 0, "checker": 0, "emissive": 0, "border": 0,
            "prism_norm_fallback": 0}
    for y in range(H):
        for x in range(W):
            A, N, D, hits = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0.0, 0
            out["shape"][y, x] = shape[0, y, x, 0]
            for i in range(n):
                b, s = i // 8, i % 8
                si = int(shape[b, y, x, s])
                if si < 0:
                    continue
                r, o, tt = ray[b, y, x, s], start[b, y, x, s], float(t[b, y, x, s])
                sh = desc.shapes[si]
                hit, t1, _, col = orc.intersect(si, r, o)
                assert hit and np.float32(t1) == t[b, y, x, s]
                p = o + tt * r
                nrm = np.zeros(3)
                seen["prism_norm_fallback"] += orc.o.or_shape_norm(orc.dp, si, G._d(p)[1], orc.last_hole,
                                                                   nrm.ctypes.data_as(G._D))
                rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
                rn = math.sqrt(rr)
                nrm = orc.fix_norm(r / rn if rr > 0 else r, nrm)
                c = [float(col[0]), float(col[1]), float(col[2])]
                if c != list(sh.color):
                    seen["checker"] += 1
                if sh.emit:
                    seen["emissive"] += 1
                if sh.flags & F_TEXTURE:
                    uv, kind = orc.uv(si, p)
                    if kind == 2:
                        c = list(sh.bordercolor)
                        seen["border"] += 1
                    elif kind == 1 and sh.tex_frame >= 0:
                        c = _texel(desc, sh, uv[0], uv[1])
                        seen["tex_fetches"] += 1
                        seen["textured"] += 1
                    if kind != 0 and (uv[0] < 0 or uv[1] < 0 or uv[0] > 1 or uv[1] > 1):
                        seen["uv_out_of_range"] += 1
                for k in range(3):
                    A[k] = A[k] + c[k]
                    N[k] = N[k] + float(nrm[k])
                D = D + tt * rn
                hits += 1
            for k in range(3):
                out["albedo"][y, x, k] = np.float32(A[k] / float(n))
                out["normal"][y, x, k] = np.float32(N[k] / float(n))
            out["coverage"][y, x] = np.float32(float(hits) / float(n))
            out["depth"][y, x] = np.float32(D / float(hits)) if hits else np.float32(0)
    return out, seen


def image_order(g, feats):
    """full-frame image-layout planes (torch or numpy) -> arrays indexed [y, x] like predict's"""
    W, H = g.xRes, g.yRes
    out = {}
    for k, v in feats.items():
        a = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        a = a.reshape(H, W, 3) if k in ("albedo", "normal") else a.reshape(H, W)
        out[k] = a[::-1].copy()   # ppmOut rows run from the top: entry (yRes-1-y)*xRes + x
    return out


def compare(got, want, what):
    for k in want:
        bad = np.nonzero(G.differs(got[k].reshape(-1), want[k].reshape(-1)))[0]
        print("%s %s: %d of %d entries differ" % (what, k, bad.size, want[k].size))
        assert bad.size == 0, "%s %s entry %d: device %r, prediction %r" % (
            what, k, bad[0], got[k].reshape(-1)[bad[0]], want[k].reshape(-1)[bad[0]])


def _final(frame, W, H, aa, **kw):
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", frame, g)
    g.xRes, g.yRes, g.antialias_samples = W, H, aa
    for k, v in kw.items():
        setattr(g, k, v)
    return g, built


# The room of final(240) is closed: from inside no primary ray misses, from outside the walls hide what
# is in it. This eye is 0.074 outside the wall x = 10 and looks along it, so the lens (aperture 0.2, the
# default) straddles the wall: the few samples whose eye point falls inside see the room (the textured
# floor, the checker squares, the ceiling lights), the others the wall's outer face or, for pixels aimed
# past the wall, nothing. Found with the oracle alone; the test asserts it of its own prediction.
MIXED_EYE = (10.074, 8.7, 7.5)
MIXED_AT = (6.2, 7.0, -4.8)


def _mixed_camera():
    """final(240), 40x24, 64 spp, default aperture, every kind of pixel case 1 asks for"""
    g, built = _final(240, 40, 24, 64)
    for a in range(3):
        g.eye[a], g.lookingAt[a] = MIXED_EYE[a], MIXED_AT[a]
    return g, built




def test_final_frame_all_planes_and_counts():
    g, built = _mixed_camera()
    want, seen = predict(built, g, 240, 64)
    cov = want["coverage"]
    print("prediction:", seen, "partial pixels", int(((cov > 0) & (cov < 1)).sum()), "missed pixels",
          int((cov == 0).sum()))
    assert seen["textured"] > 0 and seen["checker"] > 0 and seen["emissive"] > 0
    assert ((cov > 0) & (cov < 1)).any() and (cov == 0).any()
    scene = dt.Scene(built, g)
    try:
        st = dt.Stats()
        got = image_order(g, dt.render_features(scene, g, 240, stats=st))
    finally:
        scene.close()
    compare(got, want, "final(240)")
    assert st.tex_fetches == seen["tex_fetches"] and st.uv_out_of_range == seen["uv_out_of_range"]
    assert st.prism_norm_fallback == seen["prism_norm_fallback"]
    assert st.pixels == 40 * 24 and st.samples == st.rays == 40 * 24 * 64 and st.kernel_ms > 0
    assert st.shadow_rays == st.sky_pixels == st.nan_pixels == st.stack_overflows == 0


@pytest.mark.parametrize("aa,n", [(16, 16), (121, 121), (121, 64)])
def test_wave_layouts(aa, n):
    """16 spp: four pixels per wave; 121 = 64 + 57: a partial last chunk; its leading chunk alone"""
    g, built = _final(240, 16, 12, aa)
    want, seen = predict(built, g, 240, n)
    scene = dt.Scene(built, g)
    try:
        st = dt.Stats()
        got = image_order(g, dt.render_features(scene, g, 240, n_samples=n, stats=st))
        if aa == 121:
            with pytest.raises(dt.DTError, match="multiple of 64 or spp"):
                dt.render_features(scene, g, 240, n_samples=100)
    finally:
        scene.close()
    compare(got, want, "%d of %d spp" % (n, aa))
    assert st.samples == 16 * 12 * n and st.tex_fetches == seen["tex_fetches"]


@pytest.mark.parametrize("layout", [dt.DT_OUT_IMAGE, dt.DT_OUT_SLAB], ids=["image", "slab"])
def test_tile_shares(layout):
    """world = 3: each rank writes its own pixels' entries, the full-frame call's values, and nothing
    else; the ranks' pixels partition the frame"""
    W, H, n = 40, 24, 64
    g, built = _final(240, W, H, n)
    scene = dt.Scene(built, g)
    try:
        full = {k: v.cpu().numpy() for k, v in dt.render_features(scene, g, 240).items()}
        owner = np.full(W * H, -1)
        for rank in range(3):
            tile = dt.tiles(tile_w=8, tile_h=8, rank=rank, world=3, layout=layout)
            n3 = dt.accum_doubles(g, tile)
            out = {k: (torch.full((n3 // 3,), -77, dtype=torch.int32, device="cuda") if k == "shape" else
                       torch.full((n3 if k in ("albedo", "normal") else n3 // 3,), -77.0, device="cuda"))
                   for k in PLANES}
            st = dt.Stats()
            dt.render_features(scene, g, 240, tile=tile, out=out, stats=st)
            out = {k: v.cpu().numpy() for k, v in out.items()}
            # the pixel of every slot q this rank owns, as the image-layout entry (yRes-1-y)*xRes + x
            tiles_x, n_tiles = (W + 7) // 8, ((W + 7) // 8) * ((H + 7) // 8)
            own_q, own_px = [], []
            for slot in range((n_tiles + 2) // 3):
                # dt_scene_dev.h tile_of
                h = (slot * 2654435761) & 0xFFFFFFFF
                h ^= h >> 15
                h = (h * 0x2c1b3c6d) & 0xFFFFFFFF
                h ^= h >> 12
                t = slot * 3 + (rank + h % 3) % 3
                if t >= n_tiles:
                    continue
                ty, tx = divmod(t, tiles_x)
                for py in range(8):
                    for px in range(8):
                        x, y = tx * 8 + px, ty * 8 + py
                        if x < W and y < H:
                            e = (H - 1 - y) * W + x
                            own_px.append(e)
                            own_q.append(e if layout == dt.DT_OUT_IMAGE else slot * 64 + py * 8 + px)
            own_q, own_px = np.array(own_q), np.array(own_px)
            assert st.pixels == own_q.size
            assert (owner[own_px] == -1).all()
            owner[own_px] = rank
            for k in PLANES:
                three = k in ("albedo", "normal")
                a = out[k].reshape(-1, 3) if three else out[k]
                f = full[k].reshape(-1, 3) if three else full[k]
                assert not G.differs(a[own_q], f[own_px]).any(), (rank, k)
                rest = np.ones(len(a), bool)
                rest[own_q] = False
                assert (a[rest] == -77).all(), (rank, k)
        assert (owner >= 0).all()
    finally:
        scene.close()


_gold = np.load(os.path.join(HERE, "golden", "geom_ref.npz"))
_SCENES = [k for k in range(len(_gold["cam.shape"])) if _gold["cam.on_device"][k]]


@pytest.mark.parametrize("k", _SCENES, ids=["%d-%s" % (k, _gold["shape_names"][_gold["cam.shape"][k]])
                                            for k in _SCENES])
def test_one_shape_scenes(k):
    """tests/golden/geom_ref.npz's one-shape camera scenes (grazing hits, the eye inside a sphere and a
    prism, zero ray components; every device shape type), their stored globals at 4 spp"""
    g = G.globals_from_record(_gold["cam.globals"][k])
    g.antialias_samples = 4
    desc, keep = G.one_shape_scene(_gold["shapes"][_gold["cam.shape"][k]], _gold["holes"])
    want, seen = predict(desc, g, 0, 4)
    scene = dt.Scene(desc, g)
    try:
        st = dt.Stats()
        got = image_order(g, dt.render_features(scene, g, 0, stats=st))
    finally:
        scene.close()
    print("scene %d: coverage %.3f, %s" % (k, float(want["coverage"].mean()), seen))
    compare(got, want, "scene %d" % k)
    assert st.prism_norm_fallback == seen["prism_norm_fallback"]
    assert st.tex_fetches == seen["tex_fetches"] and st.uv_out_of_range == seen["uv_out_of_range"]


def test_tunnel_frame_is_the_unshifted_hit():
    """a frame at or after frame_prism: the planes are the shift-0 primary hit's"""
    g0 = dt.globals_default()
    frame = max(int(g0.frame_prism), 150 * 8)
    g, built = _final(frame, 16, 12, 64)
    assert frame >= g.frame_prism
    want, seen = predict(built, g, frame, 64)
    scene = dt.Scene(built, g)
    try:
        got = image_order(g, dt.render_features(scene, g, frame))
    finally:
        scene.close()
    compare(got, want, "final(%d)" % frame)


def test_a_render_afterwards_is_unaffected():
    g, built = _final(240, 40, 24, 4)
    scene = dt.Scene(built, g)
    try:
        a = torch.zeros(3 * 40 * 24, device="cuda")
        b = torch.zeros_like(a)
        dt.render(scene, g, 240, a)
        dt.render_features(scene, g, 240)
        st = dt.render(scene, g, 240, b)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert st.pixels == 40 * 24
    finally:
        scene.close()


def test_prismcyl_scene_is_unsupported():
    g = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, g)
    g.xRes, g.yRes, g.antialias_samples = 16, 12, 4
    scene = dt.Scene(built, g)
    try:
        with pytest.raises(dt.DTError, match=r"\(-4\).*RectPrismWithCylinder"):
            dt.render_features(scene, g, 30)
    finally:
        scene.close()


def test_progressive_features_are_the_leading_samples():
    g, built = _final(240, 16, 12, 128)
    scene = dt.Scene(built, g)
    try:
        p = dt.Progressive(scene, g, 240)
        with pytest.raises(dt.DTError, match="no window rendered"):
            p.features()
        p.step()
        got = p.features()
        want = dt.render_features(scene, g, 240, n_samples=64)
        assert set(got) == set(PLANES)
        for k in PLANES:
            assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
        only = p.features(planes=("depth",))
        assert list(only) == ["depth"] and torch.equal(only["depth"].view(torch.int32), want["depth"].view(torch.int32))
    finally:
        scene.close()


def _read_png(path):
    """8-bit RGB, filter type none (dt_write_png): (H, W, 3) uint8"""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, W, H = 8, b"", 0, 0
    while pos < len(raw):
        n = int.from_bytes(raw[pos:pos + 4], "big")
        kind, body = raw[pos + 4:pos + 8], raw[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            W, H = int.from_bytes(body[:4], "big"), int.from_bytes(body[4:8], "big")
            assert body[8] == 8 and body[9] == 2
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, 3)


def test_cli_feature_images(tmp_path):
    """dtrender final 30 --features P at 40x24, 16 spp: the four PNGs are the Python planes through the
    CLI's formulas (distraytracer_amd.feature_images), and the frame is the file written without the flag"""
    common = [DTRENDER, "final", "30", "--res", "40x24", "--spp", "16", "--depth", "2"]
    plain, with_f, prefix = str(tmp_path / "plain.png"), str(tmp_path / "feat.png"), str(tmp_path / "P")
    subprocess.run(common + ["--out", plain], check=True, timeout=120, stdout=subprocess.DEVNULL)
    subprocess.run(common + ["--out", with_f, "--features", prefix], check=True, timeout=120,
                   stdout=subprocess.DEVNULL)
    assert open(plain, "rb").read() == open(with_f, "rb").read()
    # the CLI's globals: defaults, no models, buildFinal(240), then the options
    g = dt.globals_default()
    g.use_model = 0
    built = dt.build_scene("final", 240, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = 40, 24, 16, 2
    scene = dt.Scene(built, g)
    try:
        feats = dt.render_features(scene, g, 240, planes=("albedo", "normal", "depth", "coverage"))
    finally:
        scene.close()
    imgs = dt.feature_images(g, {k: v.cpu().numpy() for k, v in feats.items()})
    for name, v in imgs.items():
        png = _read_png("%s.%s.png" % (prefix, name))
        assert png.shape == (24, 40, 3)
        assert np.array_equal(png.reshape(-1), v.astype(np.uint8)), name
    assert imgs["coverage"].max() == 255 and imgs["depth"].max() == 255
