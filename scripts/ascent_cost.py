"""What one pose search of the smoother costs resident on the device against the host-driven loop.

  host      monorfs_amd/loopy.py::LogLikeGradientAscent as it always ran: per iteration one gradient batch and one batch of 16
            line-search candidates per active estimate (phd_quasi_set_loglik_grad, phd_quasi_set_loglik), each a staged copy in
            and out and a stream wait, and the pose compositions in numpy between them.
  resident  PHDNavigator.QuasiAscent (phd_quasi_ascent): one copy in, the chain of kernels, one copy out; between rounds of
            `round_iterations` iterations the host reads one word. Measured for rounds of 1, 2, 4 and 8 and the library's default.
Both run the same searches on the same handle (the results are compared: iteration counts equal, values and poses within the
tolerances of tests/test_gpu_ascent.py), alternated in one process. Wall time of the host clock around calls that end in a
device synchronise; --warmup rounds are not counted; median, minimum and maximum of --repeats rounds.

Shapes: 1, 16 and 64 starting guesses (GuidedFitMixture's guesses climb side by side) against --landmarks landmarks and
--measurements measurements, the scene of tests/loopy_stub.py.

Prints one JSON line.   python scripts/ascent_cost.py [--starts 1,16,64] [--scene-seeds 1064,1016] [--landmarks 40] [--measurements 20] [--repeats 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS = (1, 2, 4, 8, 0)   # 0: the library's default


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def cost(nav, loopy, scene, seed, n, J, M, mode, repeats, warmup):
    lin, lm, z = scene(np.random.default_rng(seed), nav.params, J, M)
    rng = np.random.default_rng(1000 + n)
    starts = rng.normal(0, 1, (n, 6)) * [4e-3, 4e-3, 4e-3, 2e-3, 2e-3, 2e-3]
    ms = {"host": []}
    ms.update({"resident_round_%d" % r if r else "resident_default": [] for r in ROUNDS})
    iters = None
    for rep in range(warmup + repeats):
        t0 = time.perf_counter()
        want, wantv = loopy.LogLikeGradientAscent(nav, starts, z, lm, lin, mode)
        t1 = time.perf_counter()
        if rep >= warmup:
            ms["host"].append((t1 - t0) * 1e3)
        for r in ROUNDS:
            t0 = time.perf_counter()
            got, gotv, iters, capped = nav.QuasiAscent(starts, z, lm, lin, mode, round_iterations=r)
            t1 = time.perf_counter()
            if rep >= warmup:
                ms["resident_round_%d" % r if r else "resident_default"].append((t1 - t0) * 1e3)
            assert not capped and np.allclose(gotv, wantv, rtol=1e-9, atol=1e-8) and np.allclose(got, want, rtol=0, atol=1e-9)
    out = {"scene_seed": seed, "starts": n, "landmarks": J, "measurements": M, "average_mode": mode, "iterations_per_estimate": [int(i) for i in iters],
           "device_calls_of_the_host_loop": 1 + 2 * int(max(iters))}
    out.update({k: stats(v) for k, v in ms.items()})
    out["host_over_resident_default"] = round(out["host"]["median_ms"] / out["resident_default"]["median_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--starts", default="1,16,64")
    ap.add_argument("--landmarks", type=int, default=40)
    ap.add_argument("--measurements", type=int, default=20)
    ap.add_argument("--average-mode", type=int, default=1)
    ap.add_argument("--scene-seeds", default="1064,1016", help="one table per scene: the cost of an evaluation depends on how the landmarks cluster")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from loopy_stub import scene
    from monorfs_amd import loopy, navigator
    from monorfs_amd.abi import prm3d_defaults
    starts = [int(s) for s in args.starts.split(",")]
    p = prm3d_defaults(max_particles=16 * max(starts), max_components=600, max_measurements=max(16, args.measurements))
    nav = navigator.PHDNavigator(p, particlecount=1)
    nav.timing_reset(False)
    cases = [cost(nav, loopy, scene, int(seed), n, args.landmarks, args.measurements, args.average_mode, args.repeats, args.warmup)
             for seed in args.scene_seeds.split(",") for n in starts]
    nav.close()
    print(json.dumps({"clock": "host wall time around synchronous calls", "repeats": args.repeats, "warmup": args.warmup, "cases": cases}))


if __name__ == "__main__":
    main()
