"""phd_map_error through the C++ host mirror (tests/map_error_check.cpp): PHDNavigator.hpp compiles with the new method against
the header; without a GPU the program fails loudly, with one it compares the device's series with the host's own metric."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp):
    from monorfs_amd import _lib
    so = _lib.build()
    exe = os.path.join(tmp, "map_error_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "map_error_check.cpp"),
                           so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_error_check_fails_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    r = subprocess.run([build(str(tmp_path))], capture_output=True, text=True)
    assert r.returncode == 3, r.stdout + r.stderr
    assert "no HIP device" in r.stdout


@pytest.mark.gpu
def test_map_error_check_runs_on_gpu(tmp_path):
    r = subprocess.run([build(str(tmp_path))], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "estimate sizes:" in r.stdout and r.stdout.rstrip().endswith("map error ok"), r.stdout
