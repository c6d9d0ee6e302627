"""Object mattes on the device (include/dt.h dt_render_mattes, dt_matte_mask; dt_mattes_kernel) against
tests/mattes_ref.py, in every bit.

The reference: dt_intersect_primary's hit shapes (pinned to the oracle by tests/test_gpu_isect.py) of the rays
the call's samples are (sample i of pixel (x, y) is ray ((i/8)*W*H + y*W + x)*8 + i%8), regrouped per pixel and
fed to the numpy restatement. id, weight and distinct are compared as integers and bit patterns, the overflow
count as a number. All frames lie below frame_prism."""
import ctypes

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import mattes_ref as R
import scene_gen as sg

pytestmark = pytest.mark.gpu


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


class Case:
    """A scene on the device, its globals and the per-pixel hit shapes of its first n samples"""

    def __init__(self, desc, g, keep, W, H, aa):
        self.desc, self.g, self.keep, self.W, self.H = desc, g, keep, W, H
        g.xRes, g.yRes, g.antialias_samples = W, H, aa
        self.spp = dt._spp(g)
        self.scene = dt.Scene(desc, g)
        nb = (self.spp + 7) // 8
        shape = torch.empty(nb * W * H * 8, dtype=torch.int32, device="cuda")
        t = torch.empty(nb * W * H * 8, dtype=torch.float32, device="cuda")
        dt.intersect_primary(self.scene, g, 0, 0, shape, t)
        self.hits = shape.cpu().numpy()

    def ids(self, n):
        return R.pixel_ids(self.hits[:((n + 7) // 8) * self.W * self.H * 8], self.W, self.H, n)

    def want(self, n, layers, gmap=None):
        return R.mattes(self.ids(n), n, layers, gmap)

    def got(self, m, layers):
        """a whole image's planes, rows flipped to the reference's order (entry (yRes-1-y)*xRes + x)"""
        out = {}
        for k in ("id", "weight", "distinct"):
            if k in m:
                a = _bits(m[k]).reshape((self.H, self.W) + ((layers,) if k != "distinct" else ()))
                out[k] = a[::-1].reshape((self.H * self.W,) + a.shape[2:])
        return out

    def check(self, m, want, layers, what):
        got = self.got(m, layers)
        for k, a in got.items():
            bad = np.nonzero((a != _bits(want[k])).reshape(self.H * self.W, -1).any(axis=1))[0]
            print("%s %s: %d of %d pixels differ" % (what, k, bad.size, self.H * self.W))
            assert bad.size == 0, "%s %s pixel %d: device %r, reference %r" % (what, k, bad[0], a[bad[0]], want[k][bad[0]])
        assert m["overflow_pixels"] == int(want["overflow"].sum()), what

    def close(self):
        self.scene.close()


def _features_case(W, H, aa):
    desc, g, keep = sg.features()
    return Case(desc, R.defocus(g), keep, W, H, aa)


@pytest.fixture(scope="module")
def c64():
    c = _features_case(48, 32, 64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def c256():
    c = _features_case(24, 16, 256)
    yield c
    c.close()


@pytest.mark.parametrize("layers", [1, 4, 8])
def test_identity_groups_64_spp(c64, layers):
    want = c64.want(64, layers)
    print("distinct per pixel:", np.bincount(want["distinct"]).tolist())
    assert want["distinct"].max() >= 3 and (want["distinct"] == 0).any()
    st = dt.Stats()
    m = dt.render_mattes(c64.scene, c64.g, 0, layers=layers, planes=dt.MATTE_PLANES, stats=st)
    assert m["id"].shape == (32, 48, layers) and m["weight"].shape == (32, 48, layers) and m["distinct"].shape == (32, 48)
    c64.check(m, want, layers, "64 spp, %d layers" % layers)
    assert st.pixels == 48 * 32 and st.samples == st.rays == 48 * 32 * 64 and st.kernel_ms > 0
    assert st.shadow_rays == st.tex_fetches == st.sky_pixels == st.nan_pixels == st.uv_out_of_range == 0


@pytest.mark.parametrize("n", [64, 256])
def test_counts_carry_across_chunks(c256, n):
    """256 spp: four chunks of one wave; the first chunk alone"""
    want = c256.want(n, 4)
    if n == 256:   # some group of some pixel is met again in a later chunk
        ids = c256.ids(256)
        assert any(set(r[:64][r[:64] >= 0]) & set(r[64:][r[64:] >= 0]) and len(set(r[r >= 0])) >= 2 for r in ids)
    m = dt.render_mattes(c256.scene, c256.g, 0, n_samples=n, planes=dt.MATTE_PLANES)
    c256.check(m, want, 4, "%d of 256 spp" % n)


@pytest.mark.parametrize("aa", [16, 9, 49])
def test_several_pixels_per_wave(aa):
    """spp < 64: 4, 7 and 1 pixels per wave in segments of 16, 9 and 49 lanes; 24x16 = 384 pixels is no
    multiple of 7, so the last wave of the 9-spp case is partly empty"""
    c = _features_case(24, 16, aa)
    try:
        want = c.want(aa, 4)
        assert want["distinct"].max() >= (3 if aa > 9 else 2)
        c.check(dt.render_mattes(c.scene, c.g, 0, planes=dt.MATTE_PLANES), want, 4, "%d spp" % aa)
        with pytest.raises(dt.DTError, match="dt_render_mattes: n_samples"):
            dt.render_mattes(c.scene, c.g, 0, n_samples=aa - 1)
    finally:
        c.close()


def test_a_many_to_one_map_changes_the_ranking(c64):
    """the floor one group, everything that stands on it another: where the floor led two spheres, it now
    trails their sum"""
    desc = c64.desc
    gmap = np.array([0 if desc.shapes[i].type == sg.CHECKER else 1 for i in range(desc.n_shapes)], np.int32)
    ident, want = c64.want(64, 4), c64.want(64, 4, gmap)
    top = ident["id"][:, 0]
    changed = (top >= 0) & (gmap[np.maximum(top, 0)] != want["id"][:, 0])
    print("pixels whose leading group changes: %d" % changed.sum())
    assert changed.any()
    c64.check(dt.render_mattes(c64.scene, c64.g, 0, groups=gmap, planes=dt.MATTE_PLANES), want, 4, "merged")
    m = dt.render_mattes(c64.scene, c64.g, 0, groups=dt.shape_groups(desc), planes=dt.MATTE_PLANES)
    c64.check(m, c64.want(64, 4, dt.shape_groups(desc)), 4, "material groups")


def _tile_of(slot, rank, world):
    """dt_scene_dev.h tile_of"""
    h = (slot * 2654435761) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2c1b3c6d) & 0xFFFFFFFF
    h ^= h >> 12
    return slot * world + (rank + h % world) % world


@pytest.mark.parametrize("layout", [dt.DT_OUT_IMAGE, dt.DT_OUT_SLAB], ids=["image", "slab"])
def test_tile_shares(c64, layout):
    """world = 2, 16x16 tiles: each rank writes its own pixels' entries, the whole frame's values, and nothing
    else; the ranks' pixels partition the frame"""
    W, H, L, T = 48, 32, 4, 16
    full = dt.render_mattes(c64.scene, c64.g, 0, planes=dt.MATTE_PLANES)
    c64.check(full, c64.want(64, L), L, "whole frame")
    full = {k: _bits(full[k]).reshape(W * H, -1) for k in dt.MATTE_PLANES}
    owner = np.full(W * H, -1)
    tiles_x, n_tiles = W // T, (W // T) * (H // T)
    for rank in range(2):
        tile = dt.tiles(tile_w=T, tile_h=T, rank=rank, world=2, layout=layout)
        n1 = dt.accum_doubles(c64.g, tile) // 3
        out = {"id": torch.full((n1 * L,), -77, dtype=torch.int32, device="cuda"),
               "weight": torch.full((n1 * L,), -77.0, device="cuda"),
               "distinct": torch.full((n1,), -77, dtype=torch.int32, device="cuda")}
        st = dt.Stats()
        m = dt.render_mattes(c64.scene, c64.g, 0, layers=L, tiles=tile, out=out, stats=st)
        assert m["overflow_pixels"] == 0
        own_q, own_px = [], []
        for slot in range((n_tiles + 1) // 2):
            t = _tile_of(slot, rank, 2)
            if t >= n_tiles:
                continue
            ty, tx = divmod(t, tiles_x)
            for py in range(T):
                for px in range(T):
                    e = (H - 1 - (ty * T + py)) * W + tx * T + px
                    own_px.append(e)
                    own_q.append(e if layout == dt.DT_OUT_IMAGE else slot * T * T + py * T + px)
        own_q, own_px = np.array(own_q), np.array(own_px)
        assert st.pixels == own_q.size and (owner[own_px] == -1).all()
        owner[own_px] = rank
        for k in dt.MATTE_PLANES:
            a = out[k].cpu().numpy().reshape(n1, -1)
            assert np.array_equal(_bits(a[own_q]), full[k][own_px]), (rank, k)
            rest = np.ones(n1, bool)
            rest[own_q] = False
            assert (a[rest] == -77).all(), (rank, k)
    assert (owner >= 0).all()


def test_host_planes_and_plane_subsets(c64):
    L, n1 = 4, 48 * 32
    dev = dt.render_mattes(c64.scene, c64.g, 0, planes=dt.MATTE_PLANES)
    host = {"id": np.full(n1 * L, -5, np.int32), "weight": np.full(n1 * L, -5, np.float32),
            "distinct": np.full(n1, -5, np.int32)}
    m = dt.render_mattes(c64.scene, c64.g, 0, out=host)
    assert m["overflow_pixels"] == dev["overflow_pixels"]
    for k in dt.MATTE_PLANES:
        assert np.array_equal(_bits(host[k]), _bits(dev[k]).reshape(-1)), k
    only = dt.render_mattes(c64.scene, c64.g, 0, planes=("id",))
    assert set(only) == {"id", "layers", "overflow_pixels"} and torch.equal(only["id"], dev["id"])
    only = dt.render_mattes(c64.scene, c64.g, 0, out={"distinct": np.zeros(n1, np.int32)})
    assert np.array_equal(only["distinct"], _bits(dev["distinct"]).reshape(-1))
    only = dt.render_mattes(c64.scene, c64.g, 0, planes=("weight",), layers=2)
    assert torch.equal(only["weight"].view(torch.int32), dev["weight"][:, :, :2].contiguous().view(torch.int32))


def _lattice():
    """4x4 pixels, 256 spp, a lens of 2 focused at 10: halfway to the focus the pixel that looks along the axis
    sees a disc of diameter 1, filled by a 12x12 lattice of small spheres in front of a backdrop"""
    b = sg._Builder(1.0, (0, 0, 0))
    k, sp = 12, 0.08
    for j in range(k):
        for i in range(k):
            c = ((i - (k - 1) / 2) * sp, (j - (k - 1) / 2) * sp, 5.0)
            b.shape(sg.SPHERE, v=[c], radius=0.038, color=(0.1 + 0.05 * i, 0.1 + 0.05 * j, 0.5), center=c)
    A, B, C, D = (-20, -20, -2), (20, -20, -2), (20, 20, -2), (-20, 20, -2)
    sg._rect(b, A, B, C, D, (0.5, 0.5, 0.5))
    b.light(sg.POINT_LIGHT, center=(0, 5, 10), color=(1, 1, 1))
    g = b.globals((0, 0, 10.0), (0, 0, 0), 2.0, 10.0)
    desc, keep = b.desc()
    return desc, g, keep


def test_overflow_pixels_drop_new_groups_and_count_once():
    desc, g, keep = _lattice()
    c = Case(desc, g, keep, 4, 4, 256)
    try:
        ids = c.ids(256)
        distinct = [len(set(r[r >= 0].tolist())) for r in ids]
        print("distinct shapes per pixel:", distinct)
        assert max(distinct) > R.TABLE and min(distinct) >= 1
        want = c.want(256, 8)
        assert want["overflow"].sum() >= 1 and want["distinct"].max() == R.TABLE
        # the dropped samples are gone from the weights: they no longer add up to the coverage
        p = int(np.argmax(want["overflow"]))
        full = R.mattes(ids[p:p + 1], 256, 8, table=1 << 20)
        assert full["distinct"][0] > R.TABLE
        m = dt.render_mattes(c.scene, c.g, 0, layers=8, planes=dt.MATTE_PLANES)
        c.check(m, want, 8, "lattice")
        assert m["overflow_pixels"] == int(want["overflow"].sum()) >= 1
        # the lattice in three groups: nothing overflows
        gmap = np.array([i % 3 for i in range(144)] + [3], np.int32)
        want3 = c.want(256, 8, gmap)
        assert not want3["overflow"].any() and want3["distinct"].max() == 4
        m3 = dt.render_mattes(c.scene, c.g, 0, groups=gmap, layers=8, planes=dt.MATTE_PLANES)
        c.check(m3, want3, 8, "lattice in three groups")
        assert m3["overflow_pixels"] == 0
    finally:
        c.close()


def test_the_layers_add_up_to_the_coverage_plane(c64, c256):
    for c, n in ((c64, 64), (c256, 256)):
        m = dt.render_mattes(c.scene, c.g, 0, layers=8, planes=dt.MATTE_PLANES)
        assert int(m["distinct"].max()) <= 8 and m["overflow_pixels"] == 0
        counts = m["weight"].cpu().numpy().astype(np.float64) * n   # exact: count <= 1024, n a power of two
        assert (counts == np.round(counts)).all()
        cov = np.float32(counts.sum(axis=-1) / np.float64(n))
        f = dt.render_features(c.scene, c.g, 0, planes=("coverage",))["coverage"].cpu().numpy()
        assert np.array_equal(cov.reshape(-1).view(np.int32), f.view(np.int32))
        assert ((cov > 0) & (cov < 1)).any()


def test_a_render_afterwards_is_unaffected():
    desc, g, keep = sg.features()
    g.xRes, g.yRes, g.antialias_samples = 40, 24, 4
    scene = dt.Scene(desc, g)
    try:
        a = torch.zeros(3 * 40 * 24, device="cuda")
        b = torch.zeros_like(a)
        dt.render(scene, g, 0, a)
        dt.render_mattes(scene, g, 0)
        st = dt.render(scene, g, 0, b)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and st.pixels == 40 * 24
    finally:
        scene.close()


def test_matte_mask_on_the_device_is_the_host_loop(c64):
    m = dt.render_mattes(c64.scene, c64.g, 0, layers=4)
    host = {"id": m["id"].cpu().numpy(), "weight": m["weight"].cpu().numpy()}
    for groups in ([0], [1, 2, 3], [2, 2, 0, 5], list(range(64))):
        dev = dt.matte_mask(m, groups)
        torch.cuda.synchronize()
        want = dt.matte_mask(host, groups)
        assert dev.is_cuda and dev.shape == (32, 48) and want.shape == (32, 48)
        assert np.array_equal(_bits(dev), _bits(want)), groups
        assert np.array_equal(_bits(want).reshape(-1),
                              _bits(R.matte_mask(host["id"].reshape(-1, 4), host["weight"].reshape(-1, 4), groups)))
    frac = dt.matte_mask(m, [1, 2, 3]).cpu().numpy()
    assert ((frac > 0) & (frac < 1)).any()   # an antialiased edge
    empty = {"id": torch.empty(0, dtype=torch.int32, device="cuda"), "weight": torch.empty(0, device="cuda"), "layers": 4}
    assert dt.matte_mask(empty, [1]).numel() == 0


def test_progressive_mattes_are_the_leading_samples(c256):
    p = dt.Progressive(c256.scene, c256.g, 0)
    with pytest.raises(dt.DTError, match="no window rendered"):
        p.mattes()
    p.step()
    p.step()
    got, want = p.mattes(), dt.render_mattes(c256.scene, c256.g, 0, n_samples=128)
    assert torch.equal(got["id"], want["id"]) and got["overflow_pixels"] == want["overflow_pixels"]
    assert torch.equal(got["weight"].view(torch.int32), want["weight"].view(torch.int32))
    c256.check(got, c256.want(128, 4), 4, "two windows")


def test_checks_that_read_the_scene(c64):
    """a shape count that is not the scene's, with and without a map; a RectPrismWithCylinder"""
    n1, n_shapes = 48 * 32, c64.desc.n_shapes
    ids = np.zeros(n1 * 4, np.int32)
    from distraytracer_amd._lib import Mattes
    m = Mattes(ids.ctypes.data, None, None)
    gmap = np.zeros(n_shapes + 1, np.int32)
    for n, gp in ((n_shapes + 1, None), (n_shapes - 1, None), (n_shapes + 1, ctypes.c_void_p(gmap.ctypes.data))):
        rc = dt.lib.dt_render_mattes(c64.scene.handle, ctypes.byref(c64.g), 0, None, 64, gp, n, 4, ctypes.byref(m), 0,
                                     None, None, None)
        err = dt.lib.dt_last_error().decode()
        assert rc == -1 and err.startswith("dt_render_mattes: n_shapes %d" % n), err
    g = dt.globals_default()
    built = dt.build_scene("prismcyl", 30, g)
    g.xRes, g.yRes, g.antialias_samples = 16, 12, 4
    scene = dt.Scene(built, g)
    try:
        with pytest.raises(dt.DTError, match=r"\(-4\): dt_render_mattes: .*RectPrismWithCylinder"):
            dt.render_mattes(scene, g, 30)
    finally:
        scene.close()


def test_cli_writes_a_matte_image_and_the_same_frame(tmp_path):
    """dtrender final 30 --mattes P at 40x24, 16 spp: P.matte.png is written, an image of the frame's size with
    colour in it, and the frame is the file written without the flag"""
    import os
    import subprocess
    dtrender = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "distraytracer_amd", "dtrender")
    common = [dtrender, "final", "30", "--res", "40x24", "--spp", "16", "--depth", "2"]
    plain, with_m, prefix = str(tmp_path / "plain.png"), str(tmp_path / "m.png"), str(tmp_path / "P")
    subprocess.run(common + ["--out", plain], check=True, timeout=120, stdout=subprocess.DEVNULL)
    res = subprocess.run(common + ["--out", with_m, "--mattes", prefix, "--matte-layers", "3"], check=True, timeout=120,
                         stdout=subprocess.PIPE)
    assert open(plain, "rb").read() == open(with_m, "rb").read()
    assert b"mattes: 960 pixels" in res.stdout and b"3 layers, 0 overflow pixels" in res.stdout
    raw = open(prefix + ".matte.png", "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[16:24] == (40).to_bytes(4, "big") + (24).to_bytes(4, "big")
    assert len(raw) > 200
