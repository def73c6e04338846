"""phd_pose_error through the C++ host mirror (tests/pose_error_check.cpp) and the host's own metric alone
(tests/pose_error_host.cpp over monorfs_amd/host/PoseError.hpp): PHDNavigator.hpp compiles with the new method against the
header; without a GPU the device program fails loudly, with one it compares the device's series with PoseError.hpp. The
host-only program runs its hand-checkable cases and is held against the numpy statement of tests/pose_error_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pose_error_ref as ref
from pose_error_tools import MODES, build_host, host_series, same_kind


def build(tmp):
    from monorfs_amd import _lib
    so = _lib.build()
    exe = os.path.join(tmp, "pose_error_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "pose_error_check.cpp"),
                           so, "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def random_log(rng, L, noise=1e-2):
    """poses with rotations of 0.05 to 1 rad, and a truth 1e-2 away in location and in rotation"""
    def quats(angle):
        v = rng.normal(size=(L, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        return np.concatenate([np.cos(angle / 2)[:, None], np.sin(angle / 2)[:, None] * v], axis=1)
    est = np.concatenate([rng.uniform(-2, 2, size=(L, 3)), quats(rng.uniform(0.05, 1.0, L))], axis=1)
    dq = quats(np.full(L, noise))
    q = est[:, 3:]
    turned = np.stack([q[:, 0] * dq[:, 0] - (q[:, 1:] * dq[:, 1:]).sum(1),
                       q[:, 0] * dq[:, 1] + q[:, 1] * dq[:, 0] + q[:, 2] * dq[:, 3] - q[:, 3] * dq[:, 2],
                       q[:, 0] * dq[:, 2] + q[:, 2] * dq[:, 0] + q[:, 3] * dq[:, 1] - q[:, 1] * dq[:, 3],
                       q[:, 0] * dq[:, 3] + q[:, 3] * dq[:, 0] + q[:, 1] * dq[:, 2] - q[:, 2] * dq[:, 1]], axis=1)
    truth = np.concatenate([est[:, :3] + noise * rng.normal(size=(L, 3)), turned], axis=1)
    return est, truth


def test_host_cases(tmp_path):
    r = subprocess.run([build_host(str(tmp_path)), "cases"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("estimate equals truth", "rigid offset", "turned by 0.01", "turned by 1", "turned by 3", "short odometry series", "timed division: NaN and -0"):
        assert "case " + name in r.stdout, name
    assert r.stdout.rstrip().endswith("cases ok")


def test_host_metric_against_the_numpy_statement(tmp_path):
    """PoseError.hpp and pose_error_ref.py on the same random log: paths that are no prefixes of one another, every mode,
    first_entry 0 and 1, ref_entry inside and behind the log, slam_time before, inside and behind it. The two differ in libm
    and in how a quaternion is scaled (q / n against (1 / n) q): locations to 5e-14 (a few hundred ulp of coordinates below 5),
    rotations (>= 1e-3 here, so the acos magnifies by 1 / sin(angle / 2) <= 2e3) to 1e-11; -0 and NaN by kind."""
    exe = build_host(str(tmp_path))
    rng = np.random.default_rng(5)
    for L in (1, 2, 11, 23):
        est, truth = random_log(rng, L)
        times = np.arange(L) / 30.0
        paths = [est[:i + 1] + (1e-3 * i if i % 5 == 3 else 0.0) * np.array([1, 1, 1, 0, 0, 0, 0]) for i in range(L)]
        queries = [(m, f, r, s) for m in range(3) for f in sorted({0, min(1, L - 1)}) for r in (0, 5, L + 3) for s in (-1.0, times[L // 2] + 1e-3, 100.0)
                   if m == 0 or s == -1.0]
        got = host_series(exe, times, truth, paths, queries)
        for q, series in zip(queries, got):
            trajectory, estimate = ref.histories(times, truth, paths, q[1])
            want = ref.all_series(MODES[q[0]], trajectory, estimate, q[2], q[3])
            for name, (gt, gv), (wt, wv), tol in zip(("location", "rotation", "odolocation", "odorotation"), series, want, (5e-14, 1e-11, 5e-14, 1e-11)):
                assert np.array_equal(gt, wt), (L, q, name)
                assert same_kind(gv, wv), (L, q, name, gv, wv)
                ok = ~np.isnan(wv)
                assert np.all(np.abs(gv[ok] - wv[ok]) <= tol), (L, q, name, np.abs(gv[ok] - wv[ok]).max())


def test_pose_error_check_fails_loudly_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    r = subprocess.run([build(str(tmp_path))], capture_output=True, text=True)
    assert r.returncode == 3, r.stdout + r.stderr
    assert "no HIP device" in r.stdout


@pytest.mark.gpu
def test_pose_error_check_runs_on_gpu(tmp_path):
    r = subprocess.run([build(str(tmp_path))], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "best slots:" in r.stdout and r.stdout.rstrip().endswith("pose error ok"), r.stdout
