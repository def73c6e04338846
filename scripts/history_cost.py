"""What the trajectory log costs (phd_history_enable / phd_history_append / phd_trajectories).

  frame   host time per frame of phd_update_motion (+ phd_history_append) + phd_step_async, posted back to back and ended
          by one phd_sync, with the log off and on, alternated in one process on the `steady` frame of configs A and B.
          Every leg starts from the same uploaded state and posts the same inputs, so both do the same work (the steps are
          not frozen: a frozen step composes nothing into the log).
  trace   phd_trajectories for the best particle and for all particles at 2048 particles and 1 000 / 10 000 entries, a
          resampling roughly every third frame (weights concentrated on a few particles on those frames), and the longest log
          once more with no resampling at all; the number of entries at which the ancestry really changed is counted from
          the returned slots and reported with the times.
  memory  bytes per entry, and the capacity ten minutes at 30 Hz need.

Prints one JSON line.   python scripts/history_cost.py [--frames 300] [--repeats 5] [--entries 1000,10000] [--configs A,B]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_cost(navigator, prm3d_defaults, cfg, frames, repeats):
    from monorfs_amd.synth import CONFIGS, Frame
    P, C, M, seed = CONFIGS[cfg]
    f = Frame(P, C, M, seed, weight_profile="steady")
    maxq = max(600, C)
    p = prm3d_defaults(max_particles=P, max_components=maxq, max_measurements=M)
    p.max_quantity = maxq
    nav = navigator.PHDNavigator(p, particlecount=P)
    nav.timing_reset(False)
    planes = f.planes()
    rng = np.random.default_rng(seed)
    noise = (1.0 / 30) * rng.normal(size=(frames, P, 6)) * np.sqrt([5e-3] * 3 + [2e-4] * 3)
    us = rng.uniform(0.05, 0.95, frames)
    reading = np.array([1e-3, 0, 0, 0, 0, 0])
    ms = {"off": [], "on": []}
    for rep in range(repeats + 1):              # (the first pair warms up and is not counted)
        for leg in ("off", "on"):
            nav.enable_history(frames if leg == "on" else 0)
            nav.upload_state(planes, f.counts, f.poses, f.weights)
            nav.set_measurements(f.z)
            nav.sync()
            t0 = time.perf_counter()
            for k in range(frames):
                nav.UpdateOdometry(k / 30.0, reading, noise[k])   # (appends when the log is on)
                nav.step_async(float(us[k]))
            nav.sync()
            if rep:
                ms[leg].append((time.perf_counter() - t0) * 1e3 / frames)
    nav.close()
    return {"P": P, "C": C, "M": M, "frames": frames, "ms_per_frame_off": ms["off"], "ms_per_frame_on": ms["on"],
            "median_off": float(np.median(ms["off"])), "median_on": float(np.median(ms["on"])),
            "spread_off": float(max(ms["off"]) - min(ms["off"]))}


def trace_cost(navigator, prm3d_defaults, entries, repeats, P=2048):
    from monorfs_amd import _lib
    from monorfs_amd.synth import Frame
    f = Frame(P, 8, 4, 77, weight_profile="steady")          # small maps: the log does not care what a step costs
    p = prm3d_defaults(max_particles=P, max_components=600, max_measurements=8)
    nav = navigator.PHDNavigator(p, particlecount=P)
    nav.timing_reset(False)
    rng = np.random.default_rng(5)
    uniform = np.full(P, 1.0 / P)
    out = {}
    for L, every in [(L, 3) for L in entries] + [(max(entries), 0)]:   # (the longest log once more with no resampling at all)
        nav.enable_history(L)
        nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
        nav.set_measurements(f.z)
        for k in range(L):
            nav.UpdateOdometry(k / 30.0, [1e-3, 0, 0, 0, 0, 0])
            if every and k % every == every - 1:               # concentrated weights: the step resamples
                w = rng.random(P) ** 40
                nav.set_weights(w / w.sum())
            else:
                nav.set_weights(uniform)
            nav.step_async(float(rng.uniform(0.05, 0.95)))
        nav.sync()
        best = nav.BestParticle
        res = {}
        for name, q in (("best", np.array([best], np.int32)), ("all", np.arange(P, dtype=np.int32))):
            times = []
            n, pt, px, ps = C.c_int(0), _lib.dp(), _lib.dp(), _lib.ip()
            for _ in range(repeats + 1):                       # (the library call alone: the paths are then in its pinned buffers)
                t0 = time.perf_counter()
                rc = nav._lib.phd_trajectories(nav._h, q.ctypes.data_as(_lib.ip), len(q), C.byref(n), C.byref(pt), C.byref(px), C.byref(ps))
                times.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0 and n.value == L
            t, x, s = nav.WayPoints(q)
            res[name + "_ms"] = times[1:]                       # (the first call allocates the result buffers)
            res[name + "_first_call_ms"] = times[0]
            if name == "all":
                res["entries_with_a_resampling"] = int(np.count_nonzero(np.any(s[:, 1:] != s[:, :-1], axis=0)))
                res["distinct_ancestors_at_entry_0"] = int(len(np.unique(s[:, 0])))
            del t, x, s
        out[str(L) if every else "%d_no_resampling" % L] = res
    nav.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--entries", default="1000,10000")
    ap.add_argument("--configs", default="A,B")
    args = ap.parse_args()
    from monorfs_amd import navigator
    from monorfs_amd.abi import prm3d_defaults
    out = {"metric": "trajectory log: host ms per posted frame with the log off / on; ms per phd_trajectories call", "frame": {}, "trace": {}}
    for cfg in [c for c in args.configs.split(",") if c]:
        out["frame"][cfg] = frame_cost(navigator, prm3d_defaults, cfg, args.frames, args.repeats)
    entries = [int(e) for e in args.entries.split(",") if e]
    if entries:
        out["trace"] = trace_cost(navigator, prm3d_defaults, entries, args.repeats)
    out["memory"] = {"bytes_per_entry_per_particle": 60, "bytes_per_entry_at_2048": 2048 * 60 + 4,
                     "entries_for_10_min_at_30_Hz": 18000, "bytes_for_10_min_at_30_Hz_at_2048": 18000 * (2048 * 60 + 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
