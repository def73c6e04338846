"""What the pose-error series costs on the device against the route a host had before it.

  device  phd_pose_error in Timed mode over a trajectory log of L entries at 2048 particles: the whole call, which uploads the
          truth and the slots, launches one workgroup per estimate, waits for the device and copies 4 L doubles back.
  host    the same four series the way a host got them before: phd_trajectories_at per entry (a device wait and a copy of a
          path of growing length each), then monorfs_amd/host/PoseError.hpp on one core (tests/pose_error_host.cpp, built
          with -O2; its time is the program's own clock around the metric, without reading its input).
Both legs read the same log, alternated in one process; the first round warms up and is not counted. The log is made without
steps: random poses per particle (set_poses) and an append per entry, a random slot per entry, the truth the newest estimate's
path plus noise of 1e-2.

Prints one JSON line.   python scripts/pose_error_cost.py [--entries 256,2048] [--repeats 3] [--particles 2048] [--host-up-to 2048]

The host route is quadratic in copies (28 L^2 bytes) and in arithmetic; beyond --host-up-to entries only its waits and copies
are measured, over every 16th entry, and the sum over all entries is extrapolated from them (said so in the output)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pose_error_tools import build_host, host_series   # (the host-only program over PoseError.hpp, as the tests build and run it)


def quats(rng, shape):
    v = rng.normal(size=shape + (3,))
    v /= np.linalg.norm(v, axis=-1)[..., None]
    a = rng.uniform(0.05, 1.0, shape)
    return np.concatenate([np.cos(a / 2)[..., None], np.sin(a / 2)[..., None] * v], axis=-1)


def cost(navigator, prm3d_defaults, exe, L, P, repeats, host_up_to):
    rng = np.random.default_rng(L)
    p = prm3d_defaults(max_particles=P, max_components=600, max_measurements=8)
    nav = navigator.PHDNavigator(p, particlecount=P)
    nav.timing_reset(False)
    nav.enable_history(L)
    times = np.arange(L) / 30.0
    slots = rng.integers(0, P, L).astype(np.int32)
    newest = np.zeros((L, 7))
    for k in range(L):
        poses = np.concatenate([rng.uniform(-2, 2, (P, 3)), quats(rng, (P,))], axis=1)
        newest[k] = poses[slots[L - 1]]
        nav.set_poses(poses)
        nav.append_history(times[k])
    nav.sync()
    truth = newest.copy()
    truth[:, :3] += 1e-2 * rng.normal(size=(L, 3))
    truth[:, 3:] += 1e-2 * rng.normal(size=(L, 4))           # (FromState scales the quaternion)
    full = L <= host_up_to
    ms = {"device": [], "host_copies": [], "host_metric": []}
    worst = 0.0
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        dev = nav.PoseError(truth, mode="timed", slots=slots, first_entry=0, ref_entry=0, slam_time=0.0)
        t1 = time.perf_counter()
        entries = range(L) if full else range(0, L, 16)
        paths = [nav.WayPointsAt(i, [slots[i]])[1][0] for i in entries]
        t2 = time.perf_counter()
        if rep:
            ms["device"].append((t1 - t0) * 1e3)
            ms["host_copies"].append((t2 - t1) * 1e3 * (1 if full else 16))
        if full:
            series, clock = host_series(exe, times, truth, paths, [(0, 0, 0, 0.0)], clock=True)   # (Timed, first_entry 0, ref_entry 0)
            host = [v for _, v in series[0]]
            if rep:
                ms["host_metric"].append(clock)
            for d, h in zip((dev[1], dev[2], dev[4], dev[5]), host):
                ok = ~np.isnan(h)
                assert len(d) == len(h) and np.array_equal(np.isnan(d), np.isnan(h))
                worst = max(worst, float(np.max(np.abs(d[ok] - h[ok]), initial=0.0)))
    nav.close()
    out = {"entries": L, "particles": P, "host_route": "measured" if full else "waits and copies of every 16th entry, times 16; no arithmetic",
           "max_abs_difference": worst if full else None, "bytes_copied_by_the_host_route": 28 * L * (L + 1)}
    for leg in ms:
        out["ms_" + leg] = ms[leg]
        out["median_" + leg] = float(np.median(ms[leg])) if ms[leg] else None
    if full:
        out["host_over_device"] = (out["median_host_copies"] + out["median_host_metric"]) / out["median_device"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="256,2048")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--particles", type=int, default=2048)
    ap.add_argument("--host-up-to", type=int, default=2048)
    args = ap.parse_args()
    from monorfs_amd import navigator
    from monorfs_amd.abi import prm3d_defaults
    out = {"metric": "pose error of a whole log, Timed mode: ms of phd_pose_error against phd_trajectories_at per entry + PoseError.hpp on one core", "log": {}}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_host(tmp, "-O2")
        for n in [int(e) for e in args.entries.split(",") if e]:
            out["log"][str(n)] = cost(navigator, prm3d_defaults, exe, n, args.particles, args.repeats, args.host_up_to)
            print(json.dumps({str(n): out["log"][str(n)]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
