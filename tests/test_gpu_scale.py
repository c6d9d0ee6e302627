"""The culling structures on scaled and shifted synthetic scenes (tests/scene_gen.py): the shadow grid,
the primary-ray lists, the fast tree and the bump tree are full of absolute margins chosen at room scale
(host_shadowgrid.cpp m1, m2, mplane, the umbra margin, the start-side rule; the reach and padding terms of
host_primlists.cpp and host_fasttree.cpp), and so are the reference's own constants (shadow rays start
1e-3 along the ray). Every family under every transform of scene_gen.CASES must still be bit-identical
to the oracle, and to the same render with every structure off and with each structure alone.
tests/test_scale_host.py checks on the host that the structures are really built for these scenes.

Frames are 96x64 at 4 spp (the 4-wave builds; the room kernel has DT_UMBRA_EARLY=0) and 48x32 at 64 spp
(the 5-wave builds, where the early point-light umbra decision is compiled in: ADVICE.md's second finding,
on the tiny room), brdf_samples 2, depth 4, a small scaled aperture.
"""
import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
import scene_gen as sg
from parity_check import assert_parity, log_equal

pytestmark = pytest.mark.gpu

FAMILIES, CASES = list(sg.FAMILIES), list(sg.CASES)
STRUCTURES = ("DT_SHADOW_GRID", "DT_PRIM_LISTS", "DT_FAST_TREE", "DT_BUMP_TREE")
KNOBS = STRUCTURES + ("DT_SG_UMBRA", "DT_SG_START", "DT_SG_REACH", "DT_PL_BLOCK", "DT_SG_PASS0", "DT_BUMP_PAD_SCALE",
                      "DT_PL_BUMP")
ALL_OFF = {k: "0" for k in STRUCTURES}


def _render(desc, g, frame):
    scene = dt.Scene(desc, g)
    try:
        out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        st = dt.render(scene, g, frame, out, dt.tiles())
        return out.cpu().numpy(), st
    finally:
        scene.close()


def _setenv(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("spp,res", [(4, (96, 64)), (64, (48, 32))], ids=["4spp", "64spp"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_product_path_matches_the_oracle(cuda, monkeypatch, family, case, spp, res):
    """The product path (every structure on) against the oracle: the largest channel difference within
    1e-4 (0 today, logged), the NaN pixels of the glass sphere (Q25) coinciding, the same rays and shadow
    rays."""
    _setenv(monkeypatch, {})
    desc, g, keep, frame = sg.build(family, case)
    g.xRes, g.yRes = res
    g.antialias_samples = spp
    gpu, st = _render(desc, g, frame)
    ref, rst = oracle.render(desc, g, frame, dt.tiles())
    print("%s %s %d spp: rays %d/%d shadow %d/%d nan %d/%d" % (family, case, spp, st.rays, rst.rays, st.shadow_rays,
                                                               rst.shadow_rays, st.nan_pixels, rst.nan_pixels))
    assert_parity("scale %s %s %d spp vs oracle" % (family, case, spp), gpu, ref, nan_ok=True)
    assert st.nan_pixels == rst.nan_pixels
    assert st.rays == rst.rays and st.shadow_rays == rst.shadow_rays
    assert st.shadow_rays > 0
    if family.startswith("motion"):
        assert st.rays > st.samples   # the blur re-traces ran


def _variants(family):
    on = lambda k: {s: v for s, v in ALL_OFF.items() if s != k}
    v = [("everything off + " + k, on(k)) for k in STRUCTURES]   # one structure at a time: a failure names its culprit
    v += [("DT_SG_UMBRA=" + m, {"DT_SG_UMBRA": m}) for m in ("0", "2")]
    v += [("DT_SG_START=" + m, {"DT_SG_START": m}) for m in ("0", "2")]
    v += [("DT_SG_REACH=0.05", {"DT_SG_REACH": "0.05"}), ("DT_PL_BLOCK=3", {"DT_PL_BLOCK": "3"})]
    if family.startswith("motion"):
        v += [("DT_SG_PASS0=" + m, {"DT_SG_PASS0": m}) for m in ("0", "1")]
        v += [("DT_BUMP_PAD_SCALE=0.5", {"DT_BUMP_PAD_SCALE": "0.5"}), ("DT_PL_BUMP=0", {"DT_PL_BUMP": "0"})]
    return v


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_structures_match_plain_walks(cuda, monkeypatch, family, case):
    """Everything off (DT_SHADOW_GRID=0 DT_PRIM_LISTS=0 DT_FAST_TREE=0 DT_BUMP_TREE=0: reference-tree walks)
    against the product path, each structure switched on alone, and the grid's, the lists' and the bump
    tree's build variants: bit for bit, with equal rays and shadow rays. 96x64, 4 spp; a fresh scene per
    variant (the switches are read when the scene is built)."""
    desc, g, keep, frame = sg.build(family, case)
    _setenv(monkeypatch, ALL_OFF)
    ref, rst = _render(desc, g, frame)
    assert rst.shadow_rays > 0
    if family.startswith("motion"):
        assert rst.rays > rst.samples
    failed = []
    for label, env in [("product path", {})] + _variants(family):
        _setenv(monkeypatch, env)
        img, st = _render(desc, g, frame)
        same = np.array_equal(img, ref, equal_nan=True)
        try:
            log_equal("scale %s %s: %s vs everything off" % (family, case, label), img, ref)
        except AssertionError:
            pass
        if not (same and st.rays == rst.rays and st.shadow_rays == rst.shadow_rays):
            failed.append("%s (%d channels differ, rays %d/%d, shadow rays %d/%d)" % (
                label, int((~((img == ref) | (np.isnan(img) & np.isnan(ref)))).sum()), st.rays, rst.rays,
                st.shadow_rays, rst.shadow_rays))
    assert not failed, failed
