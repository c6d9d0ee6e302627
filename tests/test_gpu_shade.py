"""The device's shading loop against the REFERENCE's own rayColor, ray by ray.

tests/golden/shade_ref.npz (tools/gen_golden_shade.py, tests/test_oracle_shade.py) holds scene classes whose
rays are the project's and whose colours are the reference's alone. Per class: build the SceneDesc from the
stored records, render it with the trace build the scene selects, with the all-features build
(DT_FULL_KERNEL=1) and with the work-sharing build (dt_scene_set_kernel). A room-featured scene cannot be sent
to a mesh build by any switch, so the classes come in room- and mesh-featured twins (mirror / mirror-mesh,
wave5-phong / wave5-phong-mesh, ...): every product build renders the loops it was compiled with. Then
compare with the image made from the stored reference colours in renderImage's order: assert_parity's 1e-4,
NaN channels coinciding, the pixels of `skip` rays left out. oracle.render is compared in the same message,
so that a failure says which side left the reference. AUTO below lists the build each class selects. Reads the fixture only, never oracle/_ref."""
import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
from oracle import geom as G
from oracle import shade as S
from parity_check import TOL, assert_parity

pytestmark = pytest.mark.gpu

_gold = np.load(S.GOLD)
CLASSES = [str(c) for c in _gold["classes"]]
# class -> the build its scene selects (dt_trace_build), asserted below
AUTO = {"phong": "dt_trace_kernel_mesh", "oren-nayar": "dt_trace_kernel_mesh", "cook-torrance": "dt_trace_kernel_mesh",
        "raw": "dt_trace_kernel_mesh", "mirror": "dt_trace_kernel", "mirror-mesh": "dt_trace_kernel_mesh",
        "grazing": "dt_trace_kernel", "glass": "dt_trace_kernel_full", "emitters": "dt_trace_kernel_full",
        "textured": "dt_trace_kernel_mesh", "area": "dt_trace_kernel_full", "own-shape": "dt_trace_kernel",
        "wave5-phong": "dt_trace_kernel_w5", "wave5-cook-torrance": "dt_trace_kernel_w5",
        "wave5-oren-nayar": "dt_trace_kernel_w5_mesh", "wave5-phong-mesh": "dt_trace_kernel_w5_mesh",
        "wave5-cook-torrance-mesh": "dt_trace_kernel_w5_mesh", "averaged": "dt_trace_kernel_mesh"}
# every (class, build) pair that is a render of its own: where the scene's own build is the all-features one,
# "full" would repeat "auto"
CASES = [(c, b) for c in CLASSES for b in ("auto", "full", "donate") if not (b == "full" and AUTO[c].endswith("_full"))]


def test_every_product_build_sees_a_class():
    """room, mesh and full at 4 waves and at 5; the mesh builds get the mirror, Phong and Cook-Torrance loops"""
    assert {"dt_trace_kernel", "dt_trace_kernel_mesh", "dt_trace_kernel_full", "dt_trace_kernel_w5",
            "dt_trace_kernel_w5_mesh"} <= set(AUTO.values())
    assert AUTO["mirror-mesh"] == AUTO["phong"] == AUTO["cook-torrance"] == "dt_trace_kernel_mesh"
    assert AUTO["wave5-phong-mesh"] == AUTO["wave5-cook-torrance-mesh"] == "dt_trace_kernel_w5_mesh"


@pytest.mark.parametrize("name,build", CASES, ids=["%s-%s" % c for c in CASES])
def test_render_against_reference(cuda, monkeypatch, name, build):
    tex = str(_gold[name + ".texture"])
    desc, keep = S.desc_from_records(_gold[name + ".shapes"], _gold[name + ".lights"], tex or None)
    g = G.globals_from_record(_gold[name + ".globals"])
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
    scene = dt.Scene(desc, g)
    try:
        scene.set_kernel(dt.DT_KERNEL_DONATE if build == "donate" else dt.DT_KERNEL_PRODUCT)
        out = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device="cuda")
        dt.render(scene, g, 0, out, dt.tiles())
        gpu = out.cpu().numpy()
    finally:
        scene.close()
    orc, _ = oracle.render(desc, g, 0, dt.tiles())
    ref = S.image_from_colors(g, _gold[name + ".color"])
    ok = S.pixel_mask_to_channels(g, (_gold[name + ".skip"] == 0).all(axis=1))
    with np.errstate(invalid="ignore"):
        d_or = np.nanmax(np.abs(orc[ok].astype(np.float64) - ref[ok]), initial=0.0)
    side = "the oracle agrees with the reference (largest difference %.3g)" % d_or if d_or <= TOL else \
        "the oracle leaves the reference too (largest difference %.3g)" % d_or
    try:
        assert_parity("shade %s %s (%s) vs reference" % (name, build, kernel), gpu[ok], ref[ok], nan_ok=(name == "glass"))
    except AssertionError as e:
        raise AssertionError("%s; %s" % (e, side)) from None
    assert d_or <= TOL, side
