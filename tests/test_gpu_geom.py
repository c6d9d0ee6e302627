"""The device's intersection code against the reference's geometry.cpp, one primitive at a time.

tests/golden/geom_ref.npz holds one-shape camera scenes (tools/gen_golden_geom.py): every dt_shape_type
dt_intersect_primary accepts, the camera placed so that the 4096 primary rays (32 x 16 pixels x 8
samples) hit, graze and miss; the eye inside a sphere and inside a RectPrismV2; rays with an exactly-zero
component (the centre column and row of an axis-aligned camera); aperture 0 and the default aperture.
The rays are the project's (or_primary_ray); the stored answers are the reference's alone: its
BoundingVolume::intersect for a leaf of the shape, then the shape's intersect.

For each scene: build the SceneDesc from the stored record, one dt.intersect_primary launch, compare the
shape index (0 or -1) as an integer and t by bit pattern with the stored answer. oracle.primary_hit is
compared in the same message, so that a failure says which of the two left the reference. Reads the
fixture only, never oracle/_ref."""
import os

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
import oracle
from oracle import geom as G

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "geom_ref.npz")
_gold = np.load(GOLD)
_SCENES = [k for k in range(len(_gold["cam.shape"])) if _gold["cam.on_device"][k]]


@pytest.mark.parametrize("k", _SCENES, ids=["%d-%s" % (k, _gold["shape_names"][_gold["cam.shape"][k]])
                                            for k in _SCENES])
def test_one_shape_scene_against_reference(k):
    gold = _gold
    g = G.globals_from_record(gold["cam.globals"][k])
    want_s, want_t = gold["cam.hit"][k], gold["cam.t"][k]
    n = len(want_s)
    desc, keep = G.one_shape_scene(gold["shapes"][gold["cam.shape"][k]], gold["holes"])
    scene = dt.Scene(desc, g)
    try:
        shape = torch.empty(n, dtype=torch.int32, device="cuda")
        t = torch.empty(n, dtype=torch.float32, device="cuda")
        dt.intersect_primary(scene, g, 0, 0, shape, t)
        gs, gt = shape.cpu().numpy(), t.cpu().numpy()
    finally:
        scene.close()
    os_, ot = oracle.primary_hit(desc, g, 0, 0, n)
    bad_gpu = np.nonzero((gs != want_s) | G.differs(gt, want_t))[0]
    bad_or = np.nonzero((os_ != want_s) | G.differs(ot, want_t))[0]
    print("scene %d: hits %d of %d, device mismatches %d, oracle mismatches %d" % (
        k, int((want_s >= 0).sum()), n, bad_gpu.size, bad_or.size))
    i = bad_gpu[0] if bad_gpu.size else (bad_or[0] if bad_or.size else 0)
    assert bad_gpu.size == 0 and bad_or.size == 0, (
        "%d rays differ on the device, %d in the oracle; ray %d start %s dir %s: reference (%d, %r) "
        "device (%d, %r) oracle (%d, %r)" % (bad_gpu.size, bad_or.size, i, gold["cam.start"][k][i].tolist(),
                                             gold["cam.dir"][k][i].tolist(), want_s[i], want_t[i], gs[i], gt[i],
                                             os_[i], ot[i]))
