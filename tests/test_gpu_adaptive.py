"""Adaptive sampling: converged pixels stop between sample windows (include/dt.h
dt_render_window_adaptive and dt_resolve_adaptive, dt_kernels.hip dt_adapt_*_kernel and the accum2
branches of the *_win builds, distraytracer_amd.AdaptiveProgressive).

The state is three buffers: accum (sums of sample colours), accum2 (sums of their squares) and count
(samples per pixel). A pixel is live at a window [begin, end) iff count == begin, and a live pixel is
traced unless the rule of dt_adapt.h says it has converged. A sample's colour depends only on (seed,
frame, pixel, sample index), so which pixels stop when follows from the sums of a run that never
stops: the tests take that run's (accum, accum2) after every window, compute in numpy the window at
which every pixel stops, and ask the adaptive run for exactly that, bit for bit.
"""
import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
from parity_check import assert_parity, log_equal

pytestmark = pytest.mark.gpu

# Test 3's tolerance, in grey levels. Chosen on the CPU from the oracle's per-sample colours of the
# 40x24, 256-spp spheres frame (the GPU's sums are the oracle's bits): see test_stopping's docstring.
T_SPHERES = 0.02


def _n_out(g, tile):
    return dt.slab_floats(g, tile) if tile.layout == dt.DT_OUT_SLAB else 3 * g.xRes * g.yRes


def _spheres(aa, w=40, h=24, depth=3, cloud=1):
    g = dt.globals_default()
    built = dt.build_scene("spheres", 0, g)
    g.perlin_cloud = cloud
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = w, h, aa, depth
    return g, built


def _final(frame, models, w, h, aa, depth):
    g = dt.globals_default()
    g.use_model = models
    built = dt.build_scene("final", frame, g)
    g.xRes, g.yRes, g.antialias_samples, g.max_depth = w, h, aa, depth
    return g, built


def _rule(s1, s2, n, tol):
    """the convergence rule (dt_adapt.h) on arrays [..., 3], in numpy f64, operation for operation"""
    thr2 = (np.float64(tol) / np.float64(255.0)) * (np.float64(tol) / np.float64(255.0))
    n = np.float64(n)
    with np.errstate(invalid="ignore", over="ignore"):
        d = s2 - (s1 * s1) / n
        v = d / (n * (n - np.float64(1.0)))
        return np.all(v <= thr2, axis=-1)


def _resolve_np(acc, cnt):
    """numpy's per-pixel resolve: clamp01(float32(accum / count)) * 255, 0 without samples"""
    c3 = np.repeat(cnt.astype(np.float64), 3)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(c3 > 0, acc / c3, 0.0)
    return np.clip(np.float32(mean), np.float32(0), np.float32(1)) * np.float32(255)


class _Full:
    """A run that never stops (min_samples = spp) in one-chunk windows: the sums after every window."""

    def __init__(self, scene, g, frame, tile=None):
        p = dt.AdaptiveProgressive(scene, g, frame, tol=1e9, min_samples=dt._spp(g), tile=tile)
        self.ends, self.acc, self.acc2, self.stats = [], [], [], []
        while not p.done:
            self.stats.append(p.step())
            self.ends.append(p.samples_done)
            self.acc.append(p.accum.cpu().numpy())
            self.acc2.append(p.accum2.cpu().numpy())
        self.p, self.spp = p, p.spp
        self.count = p.count.cpu().numpy()
        self.owned = self.count == p.spp          # pixels this share renders
        assert set(np.unique(self.count)) <= {0, p.spp}
        for a in self.acc + self.acc2:
            a.setflags(write=False)

    def predict(self, tol, min_samples=64):
        """per pixel the sample count at which it stops, and the pixels traced in every window"""
        stop = np.where(self.owned, self.spp, 0)
        live = self.owned.copy()
        traced = []
        for k, e in enumerate(self.ends):
            traced.append(int(live.sum()))
            if not traced[-1]:
                break
            if e < self.spp and e >= 64 and e >= min_samples:
                conv = live & _rule(self.acc[k].reshape(-1, 3)[:live.size], self.acc2[k].reshape(-1, 3)[:live.size], e, tol)
                stop[conv] = e
                live &= ~conv
        return stop, traced


def _check_adaptive(label, scene, g, frame, tile, tol, full, min_samples=64):
    """the adaptive run at `tol` against the prediction from `full`, bit for bit. Returns (the
    AdaptiveProgressive, the predicted stop counts)."""
    stop, traced = full.predict(tol, min_samples)
    p = dt.AdaptiveProgressive(scene, g, frame, tol=tol, min_samples=min_samples, tile=tile)
    got = []
    while not p.done:
        begin = p.samples_done
        st = p.step()
        got.append(int(st.pixels))
        assert st.samples == st.pixels * (p.samples_done - begin), label
        assert p.active_pixels == st.pixels and st.stack_overflows == 0
    hist = {int(e): int((stop[full.owned] == e).sum()) for e in full.ends}
    print("%s tol=%g: pixels per window %s (predicted %s), stop histogram %s" % (label, tol, got, traced, hist))
    assert got == traced, label
    cnt = p.count.cpu().numpy()
    assert np.array_equal(cnt, stop), label
    assert p.samples_taken == int(stop.sum())
    acc, acc2 = p.accum.cpu().numpy(), p.accum2.cpu().numpy()
    want = np.zeros_like(acc)
    want2 = np.zeros_like(acc2)
    for k, e in enumerate(full.ends):
        m = np.repeat(stop == e, 3)
        want[:m.size][m] = full.acc[k][:m.size][m]
        want2[:m.size][m] = full.acc2[k][:m.size][m]
    log_equal("%s accum vs the trajectory at each pixel's stop (bits)" % label, acc.view(np.uint64), want.view(np.uint64))
    log_equal("%s accum2 vs the trajectory (bits)" % label, acc2.view(np.uint64), want2.view(np.uint64))
    img = p.image().cpu().numpy()
    n3 = 3 * cnt.size
    log_equal("%s image vs numpy's per-pixel resolve (bits)" % label, img[:n3].view(np.uint32),
              _resolve_np(acc[:n3], cnt).view(np.uint32))
    assert p.nan_pixels == 0
    return p, stop


@pytest.fixture(scope="module")
def spheres256(cuda):
    """The spheres scene with clouds, 40x24, 256 spp, depth 3: the one-shot render, the oracle image,
    a plain Progressive's accumulator and the never-stopping adaptive run, shared (never modified)."""
    g, built = _spheres(256)
    tile = dt.tiles()
    scene = dt.Scene(built, g)
    try:
        out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        st = dt.render(scene, g, 0, out, tile)
        one = out.cpu().numpy()
        plain = dt.Progressive(scene, g, 0, tile).run().accum.cpu().numpy()
        full = _Full(scene, g, 0, tile)
    finally:
        scene.close()
    ref, rst = oracle.render(built, g, 0, tile, out=np.zeros(one.size, dtype=np.float32))
    for a in (one, ref, plain):
        a.setflags(write=False)
    return g, built, tile, one, st, ref, plain, full


def test_never_stopping_is_the_one_shot_render(spheres256):
    """min_samples = spp: nothing stops. image() is dt.render's and the oracle's, accum a plain
    Progressive's, every count 256, every window traces all 960 pixels (the sky-item relaunch is on
    this path: the frame has sky pixels)."""
    g, built, tile, one, st, ref, plain, full = spheres256
    assert full.ends == [64, 128, 192, 256]
    assert [int(s.pixels) for s in full.stats] == [960] * 4
    assert [int(s.samples) for s in full.stats] == [960 * 64] * 4
    assert all(s.sky_pixels > 0 for s in full.stats)
    for k in ("rays", "shadow_rays", "tex_fetches"):
        assert sum(getattr(s, k) for s in full.stats) == getattr(st, k), k
    assert np.all(full.count == 256) and full.p.samples_taken == 960 * 256 and full.p.done
    img = full.p.image().cpu().numpy()
    log_equal("never-stopping adaptive image vs one-shot (bits)", img.view(np.uint32), one.view(np.uint32))
    assert_parity("never-stopping adaptive image vs oracle", img, ref, tol=0)
    log_equal("never-stopping adaptive accum vs Progressive (bits)", full.acc[-1].view(np.uint64), plain.view(np.uint64))


def test_second_moment_pinned_to_oracle(cuda):
    """The window [0,64) of the 16x12, 144-spp, depth-2 frame: for 24 pixels (hits and misses) accum2
    is the left-to-right f64 sum of col*col of the oracle's sample colours, exactly, and accum their
    sum."""
    g, built = _spheres(144, 16, 12, 2)
    scene = dt.Scene(built, g)
    try:
        p = dt.AdaptiveProgressive(scene, g, 0, tol=0.5)
        st = p.step()
        assert p.samples_done == 64 and st.pixels == 16 * 12
        acc, acc2, cnt = p.accum.cpu().numpy(), p.accum2.cpu().numpy(), p.count.cpu().numpy()
    finally:
        scene.close()
    assert np.all(cnt == 64)
    kind = {(x, y): oracle.sample_color(built, g, 0, x, y, 0)[1] for y in range(12) for x in range(16)}
    hits = [q for q in sorted(kind) if kind[q]]
    misses = [q for q in sorted(kind) if not kind[q]]
    assert hits and misses
    n_miss = min(12, len(misses))
    n_hit = min(24 - n_miss, len(hits))
    n_miss = min(24 - n_hit, len(misses))
    pixels = [hits[(i * len(hits)) // n_hit] for i in range(n_hit)]
    pixels += [misses[(i * len(misses)) // n_miss] for i in range(n_miss)]
    assert len(pixels) == 24 and len(set(pixels)) == 24
    for (x, y) in pixels:
        s1 = np.zeros(3, dtype=np.float64)
        s2 = np.zeros(3, dtype=np.float64)
        for i in range(64):
            col = np.array(oracle.sample_color(built, g, 0, x, y, i)[0], dtype=np.float64)
            s1 = s1 + col
            s2 = s2 + col * col      # one product and one add per sample, in sample order
        off = 3 * ((g.yRes - 1 - y) * g.xRes + x)
        print("pixel (%d,%d): accum2 %s oracle %s" % (x, y, acc2[off:off + 3], s2))
        assert np.array_equal(acc[off:off + 3].view(np.uint64), s1.view(np.uint64)), (x, y)
        assert np.array_equal(acc2[off:off + 3].view(np.uint64), s2.view(np.uint64)), (x, y, acc2[off:off + 3], s2)


def test_stopping(spheres256):
    """The 40x24, 256-spp frame at tol = T_SPHERES: every pixel's count, sums and resolved value are
    what the never-stopping run's trajectory and the rule predict, each window traces the predicted
    number of pixels, and fewer than 960 * 256 samples are taken. Fails without the feature.

    Measured split (CPU oracle's per-sample colours, the rule in numpy), pixels stopping at
    64 / 128 / 192 / running to 256 of 960 -- T = 0.02: 603 / 62 / 30 / 265 (72.4% stop early,
    27.6% run to the end). For comparison T = 0.01: 582 / 0 / 2 / 376, T = 0.03: 671 / 48 / 56 / 185,
    T = 0.05: 763 / 120 / 53 / 24, and 0.1 <= T <= 0.3: 938 / 0 / 0 / 22. Half of the frame (sphere
    interiors under point lights, much of the sky) has no variance at all and stops at 64 for any T;
    only a small T separates the rest."""
    g, built, tile, one, st, ref, plain, full = spheres256
    scene = dt.Scene(built, g)
    try:
        p, stop = _check_adaptive("spheres aa=256", scene, g, 0, tile, T_SPHERES, full)
    finally:
        scene.close()
    early = int((stop < 256).sum())
    late = int((stop == 256).sum())
    print("stopped before the last window: %d, ran to 256: %d of 960" % (early, late))
    assert early >= 96 and late >= 96, "the split is vacuous"
    assert p.samples_taken < 960 * 256


def test_partial_last_chunk(cuda):
    """100 spp: windows [0,64) and [64,100)."""
    g, built = _spheres(100)
    scene = dt.Scene(built, g)
    try:
        full = _Full(scene, g, 0)
        assert full.ends == [64, 100] and [int(s.samples) for s in full.stats] == [960 * 64, 960 * 36]
        out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        dt.render(scene, g, 0, out)
        log_equal("aa=100 never-stopping vs one-shot (bits)", full.p.image().cpu().numpy().view(np.uint32),
                  out.cpu().numpy().view(np.uint32))
        p, stop = _check_adaptive("spheres aa=100", scene, g, 0, None, T_SPHERES, full)
        assert 0 < int((stop == 64).sum()) < 960
    finally:
        scene.close()


def test_two_slab_shares(spheres256):
    """world = 2 in 16x16 tiles (DT_OUT_SLAB): each share's prediction check, and the shares' counts
    and images unpacked are the single-share run's."""
    g, built, tile, one, st, ref, plain, full1 = spheres256
    scene = dt.Scene(built, g)
    try:
        whole, _ = _check_adaptive("spheres aa=256 whole", scene, g, 0, tile, T_SPHERES, full1)
        whole_img = whole.image().cpu().numpy()
        whole_cnt = whole.count.cpu().numpy()
        t0 = dt.tiles(tile_w=16, tile_h=16, rank=0, world=2, layout=dt.DT_OUT_SLAB)
        per = dt.slab_floats_max(g, t0)
        slabs = torch.zeros(2 * per, dtype=torch.float32, device="cuda")
        cslabs = torch.zeros(2 * per, dtype=torch.float32, device="cuda")
        for r in range(2):
            t = dt.tiles(tile_w=16, tile_h=16, rank=r, world=2, layout=dt.DT_OUT_SLAB)
            full = _Full(scene, g, 0, t)
            p, _ = _check_adaptive("spheres aa=256 share %d/2" % r, scene, g, 0, t, T_SPHERES, full)
            n = dt.slab_floats(g, t)
            p.image(out=slabs[r * per:r * per + p.accum.numel()])
            cslabs[r * per:r * per + n] = p.count[:n // 3].to(torch.float32).repeat_interleave(3)   # (<= 256: exact)
        image = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        cimage = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        dt.unpack_slabs(g, t0, 2, slabs, image)
        dt.unpack_slabs(g, t0, 2, cslabs, cimage)
        log_equal("two slab shares' images vs the whole frame's (bits)", image.cpu().numpy().view(np.uint32),
                  whole_img.view(np.uint32))
        assert np.array_equal(cimage.cpu().numpy()[::3].astype(np.int32), whole_cnt)
    finally:
        scene.close()


def test_tunnel_blur_frame(cuda):
    """buildFinal(1200) (motion-blur passes, the tunnel build), 96x54 at 128 spp, depth 4
    (antialias_samples = 128 samples int(sqrt(128))^2 = 121: windows [0,64) and [64,121))."""
    g, built = _final(1200, 0, 96, 54, 128, 4)
    scene = dt.Scene(built, g)
    try:
        full = _Full(scene, g, 1200)
        assert full.ends == [64, 121] and full.stats[0].pixels == 96 * 54
        out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        dt.render(scene, g, 1200, out)
        log_equal("tunnel never-stopping vs one-shot (bits)", full.p.image().cpu().numpy().view(np.uint32),
                  out.cpu().numpy().view(np.uint32))
        _check_adaptive("tunnel 1200 96x54 aa=128", scene, g, 1200, None, 0.5, full)
    finally:
        scene.close()


def test_mesh_build_slab_share(cuda):
    """buildFinal(240) with the OBJ models (the mesh build, 5 waves), 1920x1080, 256 spp, depth 4,
    rank 1's slab of a 1024-way split in 16x16 tiles."""
    g, built = _final(240, 1, 1920, 1080, 256, 4)
    tile = dt.tiles(tile_w=16, tile_h=16, rank=1, world=1024, layout=dt.DT_OUT_SLAB)
    scene = dt.Scene(built, g)
    try:
        full = _Full(scene, g, 240, tile)
        n = dt.slab_floats(g, tile)
        out = torch.zeros(n, dtype=torch.float32, device="cuda")
        dt.render(scene, g, 240, out, tile)
        log_equal("mesh share never-stopping vs one-shot (bits)", full.p.image().cpu().numpy()[:n].view(np.uint32),
                  out.cpu().numpy().view(np.uint32))
        _check_adaptive("final(240) models aa=256 1/1024", scene, g, 240, tile, 0.5, full)
    finally:
        scene.close()


def test_16_spp_single_window(cuda):
    """16 spp: the single window [0,16), four pixels per wave. Nothing stops, the bits are dt.render's."""
    g, built = _spheres(16)
    scene = dt.Scene(built, g)
    try:
        out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        st = dt.render(scene, g, 0, out)
        p = dt.AdaptiveProgressive(scene, g, 0, tol=100.0, min_samples=0)
        ws = p.step()
        assert p.done and ws.pixels == st.pixels == 960 and ws.samples == st.samples and ws.rays == st.rays
        assert np.all(p.count.cpu().numpy() == 16) and p.samples_taken == 960 * 16
        log_equal("aa=16 adaptive single window vs one-shot (bits)", p.image().cpu().numpy().view(np.uint32),
                  out.cpu().numpy().view(np.uint32))
        plain = dt.Progressive(scene, g, 0).run()
        log_equal("aa=16 accum vs Progressive (bits)", p.accum.cpu().numpy().view(np.uint64),
                  plain.accum.cpu().numpy().view(np.uint64))
        with pytest.raises(dt.DTError):
            p.step()
    finally:
        scene.close()


def test_state_and_restore(spheres256):
    """state() after two windows, restore() on a second scene object, run to the end: counts, sums
    and image are the uninterrupted run's."""
    g, built, tile, one, st, ref, plain, full = spheres256
    scene = dt.Scene(built, g)
    try:
        whole, _ = _check_adaptive("spheres aa=256 uninterrupted", scene, g, 0, tile, T_SPHERES, full)
        p = dt.AdaptiveProgressive(scene, g, 0, tol=T_SPHERES)
        p.step()
        p.step()
        state = p.state()
    finally:
        scene.close()
    assert state["samples_done"] == 128 and state["tol"] == T_SPHERES and state["min_samples"] == 64
    assert state["accum2"].dtype == np.float64 and state["count"].size == 960
    scene2 = dt.Scene(built, g)
    try:
        q = dt.AdaptiveProgressive.restore(scene2, g, state)
        assert isinstance(q, dt.AdaptiveProgressive) and q.samples_done == 128 and not q.done
        q.run()
        assert q.done
        for name in ("accum", "accum2"):
            log_equal("restored %s vs uninterrupted (bits)" % name, getattr(q, name).cpu().numpy().view(np.uint64),
                      getattr(whole, name).cpu().numpy().view(np.uint64))
        assert np.array_equal(q.count.cpu().numpy(), whole.count.cpu().numpy())
        assert q.samples_taken == whole.samples_taken
        log_equal("restored image vs uninterrupted (bits)", q.image().cpu().numpy().view(np.uint32),
                  whole.image().cpu().numpy().view(np.uint32))
    finally:
        scene2.close()


def test_device_resolve_matches_host_resolve(spheres256):
    """dt_resolve_adaptive_kernel against the host loop on the final buffers of the stopping run, and
    on a copy with a zero count, a NaN pixel and out-of-range sums."""
    g, built, tile, one, st, ref, plain, full = spheres256
    scene = dt.Scene(built, g)
    try:
        p = dt.AdaptiveProgressive(scene, g, 0, tol=T_SPHERES).run()
    finally:
        scene.close()
    acc, cnt = p.accum.cpu().numpy(), p.count.cpu().numpy()
    assert len(np.unique(cnt)) > 1
    dev = torch.empty(acc.size, dtype=torch.float32, device="cuda")
    host = np.empty(acc.size, dtype=np.float32)
    assert dt.resolve_adaptive(g, p.accum, p.count, dev) == dt.resolve_adaptive(g, acc, cnt, host) == 0
    log_equal("adaptive resolve device vs host (bits)", dev.cpu().numpy().view(np.uint32), host.view(np.uint32))
    log_equal("adaptive resolve host vs numpy (bits)", host.view(np.uint32), _resolve_np(acc, cnt).view(np.uint32))
    bad, bcnt = acc.copy(), cnt.copy()
    bcnt[1] = 0
    bad[3] = np.nan              # a pixel without samples: 0, not counted
    bad[3 * 70] = np.nan         # pixel 70 (the second wave)
    bad[-1] = np.nan
    bad[7], bad[10] = -7.0, 1e9
    n_dev = dt.resolve_adaptive(g, torch.from_numpy(bad).cuda(), torch.from_numpy(bcnt).cuda(), dev)
    n_host = dt.resolve_adaptive(g, bad, bcnt, host)
    assert n_dev == n_host == 2
    log_equal("adaptive resolve with NaN pixels device vs host (bits)", dev.cpu().numpy().view(np.uint32),
              host.view(np.uint32))
