"""What the pose searches of T frames cost as ONE call over many problems against a loop of single calls.

  loop   T times PHDNavigator.QuasiAscent (phd_quasi_ascent), one frame's starting guesses each: what a host had before
         phd_quasi_ascent_multi.
  multi  one PHDNavigator.QuasiAscentMulti (phd_quasi_ascent_multi) over the starting guesses of all T frames.
Both run the same searches on the same handle (the results are compared in every round: equal bits), alternated in one process.
Wall time of the host clock around calls that end in a device synchronise, the wrappers' packing included; --warmup rounds are
not counted; median, minimum and maximum of --repeats rounds.

Shapes: --frames frames of one scene of tests/loopy_stub.py (--landmarks landmarks, --measurements measurements; every frame has
the scene's landmark and measurement set as a problem of its own and its own starting guesses), --starts guesses per frame. The
handle holds the largest case in one call (max_particles = 16 x guesses x frames).

Prints one JSON line.
  python scripts/ascent_multi_cost.py [--frames 8,64,256] [--starts 1,4] [--scene-seed 1064] [--landmarks 40] [--measurements 20] [--repeats 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def cost(nav, scene, seed, T, g, J, M, mode, repeats, warmup):
    lin, lm, z = scene(np.random.default_rng(seed), nav.params, J, M)
    rng = np.random.default_rng(1000 + 7 * T + g)
    starts = rng.normal(0, 1, (T, g, 6)) * [4e-3, 4e-3, 4e-3, 2e-3, 2e-3, 2e-3]
    problems = [(lm, z, lin)] * T
    problem = np.repeat(np.arange(T), g)
    ms = {"loop": [], "multi": []}
    iters = None
    for rep in range(warmup + repeats):
        t0 = time.perf_counter()
        single = [nav.QuasiAscent(starts[t], z, lm, lin, mode) for t in range(T)]
        t1 = time.perf_counter()
        poses, values, iters, capped = nav.QuasiAscentMulti(problems, starts.reshape(-1, 6), problem, mode)
        t2 = time.perf_counter()
        if rep >= warmup:
            ms["loop"].append((t1 - t0) * 1e3)
            ms["multi"].append((t2 - t1) * 1e3)
        assert not capped and not any(s[3] for s in single)
        assert np.array_equal(poses, np.concatenate([s[0] for s in single])) and np.array_equal(values, np.concatenate([s[1] for s in single]))
        assert np.array_equal(iters, np.concatenate([s[2] for s in single]))
    out = {"scene_seed": seed, "frames": T, "starts_per_frame": g, "estimates": T * g, "landmarks": J, "measurements": M, "average_mode": mode,
           "iterations_min": int(iters.min()), "iterations_max": int(iters.max())}
    out.update({k: stats(v) for k, v in ms.items()})
    out["loop_over_multi"] = round(out["loop"]["median_ms"] / out["multi"]["median_ms"], 2)
    out["loop_per_frame_ms"] = round(out["loop"]["median_ms"] / T, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="8,64,256")
    ap.add_argument("--starts", default="1,4")
    ap.add_argument("--landmarks", type=int, default=40)
    ap.add_argument("--measurements", type=int, default=20)
    ap.add_argument("--average-mode", type=int, default=1)
    ap.add_argument("--scene-seed", type=int, default=1064, help="1064: an evaluation is tens of microseconds, 1016: about a millisecond (profiles/ascent_cost.md)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from loopy_stub import scene
    from monorfs_amd import navigator
    from monorfs_amd.abi import prm3d_defaults
    frames = [int(s) for s in args.frames.split(",")]
    starts = [int(s) for s in args.starts.split(",")]
    p = prm3d_defaults(max_particles=16 * max(starts) * max(frames), max_components=600, max_measurements=max(16, args.measurements))
    nav = navigator.PHDNavigator(p, particlecount=1)
    nav.timing_reset(False)
    cases = [cost(nav, scene, args.scene_seed, T, g, args.landmarks, args.measurements, args.average_mode, args.repeats, args.warmup)
             for T in frames for g in starts]
    nav.close()
    print(json.dumps({"clock": "host wall time around synchronous calls", "repeats": args.repeats, "warmup": args.warmup, "max_particles": p.max_particles, "cases": cases}))


if __name__ == "__main__":
    main()
