"""What the map log costs (phd_map_history_enable / phd_map_history_append / phd_map_history).

  frame   host time per frame of phd_update_motion + phd_step_async (+ phd_map_history_append, + phd_history_append), posted
          back to back and ended by one phd_sync, three ways alternated in one process on the `steady` frame of configs A
          and B: both logs off, a map entry behind every step, map entries and the trajectory log. Every leg starts from the
          same uploaded state and posts the same inputs. The steps are bench.py's timed steps but for frozen mode, in which
          the append is refused.
  read    phd_map_history of the log the last leg left: the call, the entries and the components it copied.

Prints one JSON line.   python scripts/map_history_cost.py [--frames 300] [--repeats 5] [--configs A,B]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("off", "maps", "maps_and_paths")


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
    ms = {leg: [] for leg in LEGS}
    read = {}
    for rep in range(repeats + 1):              # (the first round warms up and is not counted)
        for leg in LEGS:
            nav.enable_history(frames if leg == "maps_and_paths" else 0)
            nav.enable_map_history(frames if leg != "off" else 0, frames * maxq)
            nav.upload_state(planes, f.counts, f.poses, f.weights)
            nav.set_measurements(f.z)
            nav.sync()
            t0 = time.perf_counter()
            for k in range(frames):
                nav.UpdateOdometry(k / 30.0, reading, noise[k])   # (appends when the trajectory log is on)
                nav.step_async(float(us[k]))
                if leg != "off":
                    nav.append_map_history(k / 30.0)
            nav.sync()
            if rep:
                ms[leg].append((time.perf_counter() - t0) * 1e3 / frames)
            if rep == repeats and leg == "maps":
                t0 = time.perf_counter()
                way = nav.WayMaps()
                read = {"ms": (time.perf_counter() - t0) * 1e3, "entries": len(way), "components": int(sum(len(e[3][0]) for e in way)),
                        "distinct_best": len(set(e[1] for e in way))}
    nav.close()
    out = {"P": P, "C": C, "M": M, "frames": frames, "read": read}
    for leg in LEGS:
        out["ms_per_frame_" + leg] = ms[leg]
        out["median_" + leg] = float(np.median(ms[leg]))
    out["spread_off"] = float(max(ms["off"]) - min(ms["off"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="A,B")
    args = ap.parse_args()
    from monorfs_amd import navigator
    from monorfs_amd.abi import prm3d_defaults
    out = {"metric": "map log: host ms per posted frame with both logs off / a map entry per step / map entries and the trajectory log", "frame": {}}
    for cfg in [c for c in args.configs.split(",") if c]:
        out["frame"][cfg] = frame_cost(navigator, prm3d_defaults, cfg, args.frames, args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
