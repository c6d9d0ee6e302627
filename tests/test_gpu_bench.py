"""bench.py as a command: a plain run times --steps frames and prints one JSON line without the
--full measurements, and --dump-outputs writes the frame its last timed step rendered. That frame
must be the image dt.render gives for the same configuration, bit for bit (the bench renders the
same frame with the same seed every step, so the dump is the same from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distraytracer_amd as dt
from parity_check import log_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_frame(cuda, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "Mpixel-samples/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    # value and ms_per_step say the same thing: 800x600 pixels x 16 spp per step
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(800 * 600 * 16 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert 0 < line["roofline"]["kernel_ms"] <= line["ms_per_step"] * 1.001
    # what --full measures is not run
    assert line["cpu_baseline"] is None and line["parity"] is None and line["end_to_end_ms_per_frame"] is None
    assert "counts_per_sample" not in line["roofline"]
    assert line["work"]["nan_pixels"] == 0

    assert sorted(os.listdir(out)) == ["image.npy"]
    got = np.load(out / "image.npy")
    assert got.dtype == np.float32 and got.shape == (600, 800, 3)
    import bench
    g, built = bench.build_globals(dt, "c2")
    scene = dt.Scene(built, g)
    ref = torch.zeros(3 * g.xRes * g.yRes, dtype=torch.float32, device=cuda)
    dt.render(scene, g, 240, ref, dt.tiles())
    scene.close()
    log_equal("bench.py --dump-outputs image = dt.render of the same config", got.ravel(), ref.cpu().numpy())
