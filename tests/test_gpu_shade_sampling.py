"""The device's glossy, rectangle-light and sphere-light sampling against the REFERENCE's own rayColor.

tests/golden/shade_sampling_ref.npz (tools/gen_golden_shade_sampling.py, tests/test_oracle_shade_sampling.py)
holds the classes of tests/scene_gen.py SAMPLING_SCENES: the rays are the project's, the colours those of the
reference's draw-tape build when handed the project's own Philox draws in the order it consumes them. The
colour it gives a ray is the colour the kernel must produce for that pixel and sample. Per class, as
tests/test_gpu_shade.py: render with the build the scene selects (AUTO, asserted), with the all-features build
(DT_FULL_KERNEL=1) and with the work-sharing build, and compare with the image made from the stored colours in
renderImage's order: assert_parity's project-wide TOL. oracle.render is compared in the same message, so that
a failure says which side left the reference. The in-motion class is also rendered with blur_samples > 0: a
wrong in_motion changes the number of blur passes, so the device's stats.rays must equal the oracle's.
Reads the fixture only, never oracle/_ref."""
import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
from oracle import geom as G
from oracle import shade as S
from parity_check import TOL, assert_parity

pytestmark = pytest.mark.gpu

_gold = np.load(S.GOLD_SAMPLING)
CLASSES = [str(c) for c in _gold["classes"]]
# class -> the build its scene selects (dt_trace_build), asserted below
AUTO = {"rect-light": "dt_trace_kernel", "sphere-light": "dt_trace_kernel_full", "glossy": "dt_trace_kernel",
        "glossy-area": "dt_trace_kernel", "in-motion": "dt_trace_kernel", "wave5-glossy-area": "dt_trace_kernel_w5",
        "wave5-glossy-area-mesh": "dt_trace_kernel_w5_mesh"}
CASES = [(c, b) for c in CLASSES for b in ("auto", "full", "donate") if not (b == "full" and AUTO[c].endswith("_full"))]
BUILDS = ("auto", "full", "donate")


def _scene(name):
    desc, keep = S.desc_from_records(_gold[name + ".shapes"], _gold[name + ".lights"], None)
    return desc, G.globals_from_record(_gold[name + ".globals"]), keep


def _render(monkeypatch, name, desc, g, build):
    """(image, stats, kernel name) of one render with the named build"""
    monkeypatch.setenv("DT_FULL_KERNEL", "1" if build == "full" else "0")
    monkeypatch.delenv("DT_DONATE", raising=False)
    monkeypatch.delenv("DT_W5", raising=False)
    kernel = dt.trace_build(desc, g, 0)[0]
    if build == "auto":
        assert kernel == AUTO[name], kernel
    elif build == "full":
        assert kernel.endswith("_full") and ("_w5" in kernel) == name.startswith("wave5"), kernel
    else:
        kernel = "dt_trace_kernel_dn"    # dt_scene_set_kernel's choice: dt_trace_build does not know of it
    assert g.xRes * g.yRes * S.spp(g) <= 2048 and g.max_depth <= 4
    scene = dt.Scene(desc, g)
    try:
        scene.set_kernel(dt.DT_KERNEL_DONATE if build == "donate" else dt.DT_KERNEL_PRODUCT)
        out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        st = dt.render(scene, g, 0, out, dt.tiles())
        return out.cpu().numpy(), st, kernel
    finally:
        scene.close()


def test_the_five_wave_builds_see_a_class():
    assert set(AUTO) == set(CLASSES)
    assert {"dt_trace_kernel", "dt_trace_kernel_full", "dt_trace_kernel_w5", "dt_trace_kernel_w5_mesh"} <= set(AUTO.values())


@pytest.mark.parametrize("name,build", CASES, ids=["%s-%s" % c for c in CASES])
def test_render_against_reference(cuda, monkeypatch, name, build):
    desc, g, keep = _scene(name)
    gpu, _, kernel = _render(monkeypatch, name, desc, g, build)
    orc, _ = oracle.render(desc, g, 0, dt.tiles())
    ref = S.image_from_colors(g, _gold[name + ".color"])
    d_or = float(np.abs(orc.astype(np.float64) - ref).max())
    side = "the oracle agrees with the reference (largest difference %.3g)" % d_or if d_or <= TOL else \
        "the oracle leaves the reference too (largest difference %.3g)" % d_or
    try:
        assert_parity("shade sampling %s %s (%s) vs reference" % (name, build, kernel), gpu, ref)
    except AssertionError as e:
        raise AssertionError("%s; %s" % (e, side)) from None
    assert d_or <= TOL, side


@pytest.mark.parametrize("build", BUILDS)
def test_in_motion_decides_the_blur_passes(cuda, monkeypatch, build):
    """blur_samples = 2: every sample whose primary rayColor call left in_motion set is traced twice more. The
    reference's per-vector flag gives the number of samples that do; the device's ray count equals the oracle's"""
    desc, g, keep = _scene("in-motion")
    g.blur_samples = 2
    gpu, st, kernel = _render(monkeypatch, "in-motion", desc, g, build)
    orc, ost = oracle.render(desc, g, 0, dt.tiles())
    moving = int((_gold["in-motion.in_motion"] != 0).sum())
    g.blur_samples = 0
    still = oracle.render(desc, g, 0, dt.tiles())[1]
    print("in-motion %s (%s): %d samples in motion, rays %d (device) %d (oracle) %d (without blur passes)" % (
        build, kernel, moving, st.rays, ost.rays, still.rays))
    assert moving > 0 and ost.rays > still.rays
    assert st.rays == ost.rays and st.shadow_rays == ost.shadow_rays
    assert_parity("shade sampling in-motion %s (%s) with blur passes vs oracle" % (build, kernel), gpu, orc)
