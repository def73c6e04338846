"""What the pose-error tests and scripts/pose_error_cost.py share beside the numpy statement of pose_error_ref.py: the host-only
program over monorfs_amd/host/PoseError.hpp (tests/pose_error_host.cpp), built and run on a log, and the comparison by kind."""
import os
import subprocess

import numpy as np

import pose_error_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (ref.TIMED, ref.SMOOTH, ref.FILTER)   # in the order of PHD_POSE_ERROR_*


def build_host(tmp, optimise="-O1"):
    """the host-only program: no library, no device"""
    exe = os.path.join(tmp, "pose_error_host")
    subprocess.check_call(["g++", "-std=c++17", optimise, "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "pose_error_host.cpp")])
    return exe


def host_series(exe, times, truth, paths, queries, clock=False):
    """PoseError.hpp on a log: paths[i] = the estimate as of entry i ([i + 1][7]), queries = (mode index, first_entry, ref_entry,
    slam_time). Returns per query the four series as (times, values); with `clock` also the ms the program's own clock counted
    around the metric (without reading its input), summed over the queries."""
    L = len(times)
    buf = np.concatenate([[float(L), float(len(queries))], np.asarray(times, float), np.asarray(truth, float).ravel()] +
                         [np.asarray(paths[i], float)[:i + 1].ravel() for i in range(L)] + [np.asarray(q, float) for q in queries])
    r = subprocess.run([exe, "series"], input=buf.astype(np.float64).tobytes(), capture_output=True)
    assert r.returncode == 0, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]
    lines = r.stdout.decode().split("\n")
    out, ms, i = [], None, 0
    while i < len(lines):
        if lines[i].startswith("query"):
            out.append([])
            i += 1
        elif lines[i].startswith("series"):
            n = int(lines[i].split()[2])
            v = np.array([[float(x) for x in l.split()] for l in lines[i + 1:i + 1 + n]], float).reshape(n, 2)
            out[-1].append((v[:, 0], v[:, 1]))
            i += 1 + n
        else:
            if lines[i].startswith("clock"):
                ms = (ms or 0.0) + float(lines[i].split()[1])
            i += 1
    assert len(out) == len(queries) and all(len(s) == 4 for s in out)
    return (out, ms) if clock else out


def same_kind(a, b):
    """NaN where NaN, -0 where -0 (the quirk values are compared by kind)"""
    a, b = np.asarray(a), np.asarray(b)
    zero = (b == 0)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.signbit(a[zero]), np.signbit(b[zero])) and np.all(a[zero] == 0))
