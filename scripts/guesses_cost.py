"""What the starting guesses of the pose searches of T frames cost on the host and as ONE device call.

  fit_host     loopy.GuidedFitMixtures: the whole fit with the guesses made on the host (what a host had before
               phd_quasi_guesses_multi; unchanged by it, so it can be timed from another tree: --tree)
  fit_device   loopy.GuidedFitMixturesRouted(..., device_guesses=True): the whole fit with the guess stage as one call
  loop_host    loopy.HostGuessLists: the host guess loop alone (numpy), no device call
  stage_host   loopy.HostGuesses: that loop and the batch call for the first values
  call         PHDNavigator.QuasiGuessesMulti (phd_quasi_guesses_multi): the guesses and their first values
  cpp_loop / cpp_stage / cpp_call   the same three from the C++ host (scripts/guesses_cost.cpp, built here with g++)
Wall time of the host clock around calls that end in a device synchronise, the wrappers' packing included; --warmup rounds are not
counted; median, minimum and maximum of --repeats rounds for the host routes (those of 256 frames take tens of seconds a round: few
rounds, and their first round is like the others: --warmup 0 is fair), of at least 5 (1 warm-up) for fit_device and 20 (3) for the calls.

Frames: T scenes of tests/loopy_stub.py (--landmarks x --measurements, seeds 3000 + t), each with a moved and rotated linearisation
pose and a small pose0 of its own. A tree without QuasiGuessesMulti runs fit_host, loop_host alone.

Prints one JSON line.
  python scripts/guesses_cost.py [--frames 8,64,256] [--landmarks 40] [--measurements 20] [--repeats 5] [--warmup 1] [--tree DIR] [--no-cpp] [--no-fits] [--no-fit-host]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)}


def make_frames(scene, pose3d_add, params, T, J, M):
    pose0s, zs, models, lins = [], [], [], []
    for t in range(T):
        rng = np.random.default_rng(3000 + t)
        lin, lm, z = scene(rng, params, J, M)
        lins.append(pose3d_add(lin, rng.normal(0, 1, 6) * [0.02, 0.02, 0.02, 0.4, 0.4, 0.4]))
        pose0s.append(rng.normal(0, 1, 6) * [4e-3, 4e-3, 4e-3, 2e-3, 2e-3, 2e-3])
        zs.append(z)
        models.append((np.full(len(lm), 1.0001), lm, np.broadcast_to(1e-4 * np.eye(3), (len(lm), 3, 3))))
    return pose0s, zs, models, lins


def timed(fn, repeats, warmup):
    ms, last = [], None
    for rep in range(warmup + repeats):
        t0 = time.perf_counter()
        last = fn()
        if rep >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms), last


def cpp_cost(so, frames, repeats, warmup):
    """scripts/guesses_cost.cpp on the same frames: {cpp_loop, cpp_stage, cpp_call}"""
    pose0s, zs, models, lins = frames
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "guesses_cost")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(HERE, "scripts", "guesses_cost.cpp"), so,
                               "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
        path = os.path.join(tmp, "scene.txt")
        num = lambda a: " ".join("%.17g" % v for v in np.asarray(a, float).ravel())
        with open(path, "w") as fh:
            fh.write("%d\n" % len(pose0s))
            for pose0, z, model, lin in zip(pose0s, zs, models, lins):
                fh.write("%d %d\n%s\n%s\n%s\n%s\n" % (len(model[1]), len(z), num(model[1]), num(z), num(lin), num(pose0)))
        out = subprocess.check_output([exe, path, str(repeats), str(warmup)], text=True)
    got = json.loads(out)
    return {k: stats(v) for k, v in got["ms"].items()}, got["guesses"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="8,64,256")
    ap.add_argument("--landmarks", type=int, default=40)
    ap.add_argument("--measurements", type=int, default=20)
    ap.add_argument("--average-mode", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tree", default=HERE, help="the repository whose monorfs_amd is timed (its library built)")
    ap.add_argument("--no-cpp", action="store_true")
    ap.add_argument("--no-fits", action="store_true", help="the guess stage alone")
    ap.add_argument("--no-fit-host", action="store_true", help="skip fit_host (it is timed from another tree)")
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    sys.path.insert(0, os.path.join(args.tree, "tests"))
    from loopy_stub import scene
    from monorfs_amd import _lib, loopy, navigator
    from monorfs_amd.abi import prm3d_defaults
    from monorfs_amd.navigator import pose3d_add
    p = prm3d_defaults(max_particles=4096, max_components=600, max_measurements=max(16, args.measurements))
    nav = navigator.PHDNavigator(p, particlecount=1)
    nav.timing_reset(False)
    device = hasattr(nav, "QuasiGuessesMulti")
    cases = []
    for T in [int(s) for s in args.frames.split(",")]:
        frames = make_frames(scene, pose3d_add, p, T, args.landmarks, args.measurements)
        pose0s, zs, models, lins = frames
        out = {"frames": T, "landmarks": args.landmarks, "measurements": args.measurements, "pairs": T * args.landmarks * args.measurements}
        if not args.no_fits and not args.no_fit_host:
            out["fit_host"], host = timed(lambda: loopy.GuidedFitMixtures(nav, pose0s, zs, models, lins, args.average_mode), args.repeats, args.warmup)
            out["components_host"] = sum(len(c) for _, c in host)
        if device:
            problems, starts = loopy._problems_of(pose0s, zs, models, lins)
            out["loop_host"], (hg, hp) = timed(lambda: loopy.HostGuessLists(p, problems, starts), args.repeats, args.warmup)
            out["stage_host"], _ = timed(lambda: loopy.HostGuesses(nav, problems, starts), args.repeats, args.warmup)
            out["call"], got = timed(lambda: nav.QuasiGuessesMulti(problems, starts), max(args.repeats, 20), max(args.warmup, 3))
            out["guesses"] = int(got[0][-1])
            assert [tuple(int(v) for v in q) for q in got[1]] == [q for f in hp for q in f], "the device's lists are not the host's"
            if not args.no_fits:
                out["fit_device"], dev = timed(lambda: loopy.GuidedFitMixturesRouted(nav, pose0s, zs, models, lins, args.average_mode, device_guesses=True),
                                               max(args.repeats, 5), max(args.warmup, 1))
                out["components_device"] = sum(len(c) for _, c in dev)
                if "fit_host" in out:
                    out["fit_host_over_fit_device"] = round(out["fit_host"]["median_ms"] / out["fit_device"]["median_ms"], 2)
            out["stage_host_over_call"] = round(out["stage_host"]["median_ms"] / out["call"]["median_ms"], 1)
            if not args.no_cpp:
                cpp, n = cpp_cost(_lib.SO_PATH, frames, max(args.repeats, 20), max(args.warmup, 3))
                assert n == out["guesses"], "the C++ host counts other guesses"
                out.update(cpp)
                out["cpp_stage_over_cpp_call"] = round(cpp["cpp_stage"]["median_ms"] / cpp["cpp_call"]["median_ms"], 2)
        cases.append(out)
        print(json.dumps(out), file=sys.stderr, flush=True)
    nav.close()
    print(json.dumps({"clock": "host wall time around synchronous calls", "repeats": args.repeats, "warmup": args.warmup, "tree_has_device_guesses": device,
                      "max_particles": p.max_particles, "cases": cases}))


if __name__ == "__main__":
    main()
