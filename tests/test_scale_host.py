"""Host half of the scale tests (no GPU): what dt_accel_info_build, dt_bvh_build, dt_trace_build and the
oracle say about tests/scene_gen.py's scenes under every transform, so that tests/test_gpu_scale.py
cannot pass vacuously -- the structures are built, few cells fall back to the tree, the room's plate
leaves umbra cells, the tiny room is past the bound the advisor named, the kernels are the intended
builds and the plate's shadow is in the picture.
"""
import ctypes

import numpy as np
import pytest

import distraytracer_amd as dt
import oracle
import scene_gen as sg

FAMILIES, CASES = list(sg.FAMILIES), list(sg.CASES)
KERNELS = {"room": ("dt_trace_kernel", "dt_trace_kernel_w5"),
           "features": ("dt_trace_kernel_full", "dt_trace_kernel_w5_full"),
           "motion-small": ("dt_trace_kernel_blur", "dt_trace_kernel_w5_blur"),
           "motion-large": ("dt_trace_kernel_blur", "dt_trace_kernel_w5_blur")}


def _root_box(desc, g):
    nn, ni = ctypes.c_int32(), ctypes.c_int32()
    dt.check(dt.lib.dt_bvh_build(ctypes.byref(desc), ctypes.byref(g), None, 0, None, 0, ctypes.byref(nn),
                                 ctypes.byref(ni)), "dt_bvh_build")
    nodes = (dt.BVHNode * max(nn.value, 1))()
    idx = (ctypes.c_int32 * max(ni.value, 1))()
    dt.check(dt.lib.dt_bvh_build(ctypes.byref(desc), ctypes.byref(g), nodes, nn.value, idx, ni.value, ctypes.byref(nn),
                                 ctypes.byref(ni)), "dt_bvh_build")
    return list(nodes[0].lbound), list(nodes[0].ubound)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_structures_are_built(family, case):
    """The host build succeeds, the shadow grid serves every point and rectangle light, at most half of its
    cells walk the tree, and the trace kernels at 4 and at 64 spp are the builds the GPU tests mean."""
    desc, g, keep, frame = sg.build(family, case)
    info = dt.accel_info(desc, g)
    # sg_lights counts light slots up to the last light the grid serves (a sphere light keeps its slot,
    # without lists): the number of point and rectangle lights, plus the sphere lights listed before the last
    grid = [i for i in range(desc.n_lights) if desc.lights[i].type in (sg.POINT_LIGHT, sg.RECT_LIGHT)]
    n_grid_lights = len(grid) + sum(1 for i in range(grid[-1]) if desc.lights[i].type == sg.SPHERE_LIGHT)
    assert len(grid) == (2 if family == "features" else 3)
    print(family, case, {k: info[k] for k in ("sg_lights", "sg_dim", "sg_cells", "sg_tree_cells", "sg_umbra_cells",
                                              "n_fnodes", "n_bnodes", "bump_pad")})
    assert info["n_nodes"] > 0 and info["n_fnodes"] > 0 and info["boxes_ordered"] == 1
    assert info["sg_lights"] == n_grid_lights
    assert info["sg_cells"] > 0
    assert 2 * info["sg_tree_cells"] <= info["sg_cells"]
    if family.startswith("motion"):
        assert info["n_bnodes"] > 0 and info["bump_pad"] > 0   # the blur passes have their bump tree
    for spp, want in zip((4, 64), KERNELS[family]):
        g.antialias_samples = spp
        assert dt.trace_build(desc, g, frame)[0] == want


@pytest.mark.parametrize("case", CASES)
def test_room_plate_leaves_umbra_cells(case):
    """room: whole blocks of grid cells under the plate are umbra cells of the point light above it, under
    every transform: about 25600 (light, cell) records at s = 1 and 2^8, 10250 at s = 2^-8.
    The shifted cases had none before host_shadowgrid.cpp took them into account: every leaf box of the
    reference's BVH ends at 0.01 or above (its running maximum starts at FLT_MIN), so at t_y = -2048 (-8)
    the grid box made from the leaves was 2048 (8) tall and the grid 6 x 256 x 6 cells, one layer of which
    held the room; and the f32 coordinate slack 1e-4 (1 + scale) of m1 and m2, 0.82 at 8192, swallowed the
    plate. The grid box now follows the shapes on an axis where they all lie below zero, and the slack is
    capped at 5 % of a cell (never below 1e-6 (1 + scale)): test_shifted_grid_is_the_unshifted_grid."""
    desc, g, keep, frame = sg.build("room", case)
    info = dt.accel_info(desc, g)
    print("room", case, "sg_dim", info["sg_dim"], "sg_umbra_cells", info["sg_umbra_cells"])
    assert info["sg_umbra_cells"] > 0


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shifted,plain", [("shifted", "unit"), ("tiny-shifted", "tiny")])
def test_shifted_grid_is_the_unshifted_grid(family, shifted, plain):
    """A translation leaves the shadow grid's dimensions alone, although on the y axis every shape then
    lies below zero and the reference's leaf boxes all reach up to 0.01 (host_shadowgrid.cpp, grid box)."""
    dims = []
    for case in (shifted, plain):
        desc, g, keep, frame = sg.build(family, case)
        dims.append(dt.accel_info(desc, g)["sg_dim"])
    assert dims[0] == dims[1]


def test_tiny_room_is_past_the_early_umbra_bound():
    """ADVICE.md's second finding: the early point-light umbra decision (DT_UMBRA_EARLY, dt_kernels.hip)
    looks up the cell of p where the shadow test looks up the cell of o = p + 1e-3 sn, which the advisor
    judges exact only while m1 > 1e-3. This is that situation: at s = 2^-8 an upper bound of
    m1 = (reach + 0.05) h + 1e-4 (1 + scale) (host_shadowgrid.cpp; h at most the root box's extent over the
    grid's dimension, scale at most the root box's largest coordinate) is below 1e-3, and the room has umbra
    cells (test_room_plate_leaves_umbra_cells). tests/test_gpu_scale.py renders it on the 5-wave build."""
    desc, g, keep, frame = sg.build("room", "tiny")
    info = dt.accel_info(desc, g)
    lo, hi = _root_box(desc, g)
    h = max((hi[a] - lo[a]) / info["sg_dim"][a] for a in range(3))
    scale = max(abs(v) for v in lo + hi)
    m1 = (info["sg_reach"] + 0.05) * h + 1e-4 * (1 + scale)
    print("room tiny: root box", lo, hi, "sg_dim", info["sg_dim"], "m1 <=", m1)
    assert m1 < 1e-3
    assert info["sg_umbra_cells"] > 0


@pytest.fixture(scope="module")
def plate_frames():
    """oracle frames of the room with and without the plate, per case (96x64, 4 spp, depth 4)"""
    out = {}
    for case, (s, t) in sg.CASES.items():
        pair = []
        for plate in (True, False):
            desc, g, keep = sg.room(s, t, plate=plate)
            assert (g.xRes, g.yRes, g.antialias_samples, g.max_depth) == (96, 64, 4, 4)
            img, st = oracle.render(desc, g, 0, dt.tiles())
            pair.append((img.reshape(-1, 3), st))
        out[case] = pair
    return out


@pytest.mark.parametrize("case", CASES)
def test_plate_shadow_is_in_view(plate_frames, case):
    """The plate changes at least 2 % of the pixels (its shadow and itself are in view), the frame is not
    constant and shadow rays are traced."""
    (a, st), (b, _) = plate_frames[case]
    differ = np.any(a != b, axis=1).mean()
    print("room %s: %.1f %% of the pixels differ with the plate; values %.1f .. %.1f" % (case, 100 * differ, a.min(), a.max()))
    assert differ >= 0.02
    assert a.max() > a.min()
    assert st.shadow_rays > 0 and st.nan_pixels == 0
