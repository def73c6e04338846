"""Loopy.hpp::LeaveOneOutMaps through the C++ host mirror (tests/leave_one_out_check.cpp): without a GPU it fails loudly, with
one it gives the maps of monorfs_amd/loopy.py on the same scene, digit for digit of the 17 printed (which is bit for bit)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp):
    from monorfs_amd import _lib
    so = _lib.build()
    exe = os.path.join(tmp, "leave_one_out_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "leave_one_out_check.cpp"),
                           so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_scene(path, trajectory, factors, maxparticles):
    num = lambda a: " ".join("%.17g" % v for v in np.asarray(a, float).ravel())
    with open(path, "w") as fh:
        fh.write("%d %d\n" % (len(trajectory), maxparticles))
        for (t, pose), (_, zt) in zip(trajectory, factors):
            fh.write("%.17g %s %d %s\n" % (t, num(pose), len(zt), num(zt)))


def parse(stdout):
    """{(kind, index): (w, mean, cov)} of the printed maps"""
    out, key, rows, left = {}, None, [], 0
    for ln in stdout.splitlines():
        tok = ln.split()
        if tok and tok[0] in ("map", "full", "some"):
            key, left, rows = (tok[0], int(tok[1])), int(tok[2]), []
            out[key] = (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3)))
        elif tok and tok[0] == "component":
            rows.append([float(v) for v in tok[1:]])
            left -= 1
            if left == 0:
                a = np.array(rows)
                out[key] = (a[:, 0].copy(), a[:, 1:4].copy(), a[:, 4:].reshape(-1, 3, 3).copy())
    return out


def test_leave_one_out_check_fails_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    from test_gpu_leave_one_out import make_scene
    path = str(tmp_path / "scene.txt")
    write_scene(path, *make_scene(), maxparticles=4)
    r = subprocess.run([build(str(tmp_path)), path], capture_output=True, text=True)
    assert r.returncode == 3, r.stdout + r.stderr
    assert "no HIP device" in r.stdout


@pytest.mark.gpu
def test_leave_one_out_check_matches_python(tmp_path):
    from monorfs_amd import loopy, navigator
    from monorfs_amd.abi import prm3d_defaults
    from test_gpu_leave_one_out import T, make_scene
    trajectory, factors = make_scene()
    path = str(tmp_path / "scene.txt")
    write_scene(path, trajectory, factors, maxparticles=4)       # (three left-out frames per pass: the C++ chunking runs too)
    r = subprocess.run([build(str(tmp_path)), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("leave one out ok"), r.stdout
    got = parse(r.stdout)
    nav = navigator.PHDNavigator(prm3d_defaults(max_particles=16, max_components=600, max_measurements=16), particlecount=1)
    try:
        maps, full = loopy.LeaveOneOutMaps(nav, trajectory, factors)
    finally:
        nav.close()
    same = lambda a, b: all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))
    assert len(full[0]) > 0 and same(got[("full", -1)], full)
    for i in range(T):
        assert same(got[("map", i)], maps[i]), i
    assert same(got[("some", 0)], maps[1]) and same(got[("some", 1)], maps[1])
    assert same(got[("some", 2)], full) and same(got[("some", 3)], full)
