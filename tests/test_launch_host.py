"""The device-free half of the render launch path (csrc/host_launch.h): the grow-only
device buffer that every lazily grown buffer of a scene is (a failed allocation must leave it empty,
never a null pointer behind a capacity that lets the next launch skip the allocation), and the launch
policy (chunk items, items per queue atomic, queue segments, priority steps) as a pure function of the
render's parameters, the grid and the environment. tests/launch_host_check.cpp holds the checks; it
includes only that header, makes no HIP call and runs under ASan and UBSan (leak check included)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_host_check(tmp_path):
    exe = str(tmp_path / "launch_host_check")
    # (the sanitizer runtimes linked into the program itself: it needs nothing from its environment)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "distraytracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "launch_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
