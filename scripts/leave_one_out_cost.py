"""What the leave-one-out maps of the smoother's UpdateMessagesFromMap cost in one pass of held steps against one filter per
left-out frame.

  sequential  T calls of monorfs_amd/loopy.py::FilterMissing as they always ran: each resets the handle to one particle and runs
              T - 1 blocking SlamUpdates (a copy in, the step of one particle, a stream wait): T (T - 1) blocking steps.
  one pass    loopy.LeaveOneOutMaps: the handle reset to T + 1 particles, T held steps (PHDNavigator.StepHold,
              phd_step_hold_async) posted without waiting, one sync, one download of the maps.
Both run on the same handle (the same parameters: --max-particles, 600 components, 16 measurements), alternated in one process,
and every round asserts that both give the same maps bit for bit. Wall time of the host clock around calls that end in a device
synchronise; --warmup rounds are not counted; median, minimum and maximum of --repeats rounds.

Shapes: T = 16, 64 and 192 frames of the generator of tests/test_gpu_loopy.py::test_filter_missing_against_oracle (one landmark
set of 40 seen from jittered poses, 12 measurements a frame).

Prints one JSON line.   python scripts/leave_one_out_cost.py [--frames 16,64,192] [--repeats 5] [--warmup 1] [--max-particles 256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)}


def scene(T):
    from monorfs_amd.navigator import pose3d_add
    from monorfs_amd.synth import Frame
    rng = np.random.default_rng(41)
    f = Frame(1, 40, 12, 41, weight_profile="steady")
    trajectory, factors = [], []
    for t in range(T):
        pose = pose3d_add(f.poses[0], rng.normal(0, 1, 6) * [3e-3, 3e-3, 3e-3, 1e-3, 1e-3, 1e-3])
        zt = f.z + rng.normal(0, 1, f.z.shape) * [0.5, 0.5, 0.01]
        trajectory.append((0.1 * t, pose))
        factors.append((0.1 * t, zt))
    return trajectory, factors


def cost(nav, loopy, T, repeats, warmup):
    trajectory, factors = scene(T)
    ms = {"sequential": [], "one_pass": []}
    sizes = None
    for rep in range(warmup + repeats):
        t0 = time.perf_counter()
        want = [loopy.FilterMissing(nav, trajectory, factors, i, T) for i in range(T)]
        t1 = time.perf_counter()
        got, full = loopy.LeaveOneOutMaps(nav, trajectory, factors)
        t2 = time.perf_counter()
        if rep >= warmup:
            ms["sequential"].append((t1 - t0) * 1e3)
            ms["one_pass"].append((t2 - t1) * 1e3)
        assert len(got) == T and all(all(np.array_equal(x, y) for x, y in zip(g, w)) for g, w in zip(got, want)), "the two routes give different maps"
        sizes = [len(g[0]) for g in got] + [len(full[0])]
        print("T = %d, round %d: %.1f ms sequential, %.1f ms one pass" % (T, rep, (t1 - t0) * 1e3, (t2 - t1) * 1e3), file=sys.stderr, flush=True)
    out = {"frames": T, "blocking_steps_sequential": T * (T - 1), "held_steps_one_pass": T, "particles_one_pass": T + 1,
           "map_components": [min(sizes), max(sizes)]}
    out.update({k: stats(v) for k, v in ms.items()})
    out["sequential_over_one_pass"] = round(out["sequential"]["median_ms"] / out["one_pass"]["median_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="16,64,192")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-particles", type=int, default=256, help="of the handle both routes use; at least frames + 1 for a single pass")
    args = ap.parse_args()
    from monorfs_amd import loopy, navigator
    from monorfs_amd.abi import prm3d_defaults
    p = prm3d_defaults(max_particles=args.max_particles, max_components=600, max_measurements=16)
    nav = navigator.PHDNavigator(p, particlecount=1)
    nav.timing_reset(False)
    cases = [cost(nav, loopy, int(T), args.repeats, args.warmup) for T in args.frames.split(",")]
    nav.close()
    print(json.dumps({"clock": "host wall time around synchronous calls", "repeats": args.repeats, "warmup": args.warmup,
                      "max_particles": args.max_particles, "cases": cases}))


if __name__ == "__main__":
    main()
