"""What the Kinect depth map costs a step (phd_set_depth_map): configs A, A64 and B in bench.py's timed mode
(phd_set_frozen(1) + phd_set_all_pairs(1), the same P x C x M input every step), device time per step from events on the
handle's stream, with no map, an all-+inf map and an occluding map (piecewise-constant occluders at 0.5 - 1.5 m with NaN
holes, tests/kinect_ref.py). Two image sizes: 640 x 480 with the default PRM3D camera, and 160 x 120 with the camera of
KinectDelta 4 (focal / 4, film / 4, the frame's pixel coordinates / 4), each against its own no-map time. The all-+inf
map is the same workload as no map (the cost of the map itself); the occluding one changes the workload — occluded
components keep (1 - PD) w = w and survive the MinWeight cut — so its ratio is not the map's price alone.
Prints one JSON line.   python scripts/depth_map_cost.py [--steps 300] [--warmup 30] [--repeats 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="A,A64,B")
    args = ap.parse_args()
    import torch
    import kinect_ref
    from monorfs_amd import navigator
    from monorfs_amd.abi import prm3d_defaults
    from monorfs_amd.synth import CONFIGS, Frame

    out = {"metric": "device ms per step (timed mode) with / without a depth map", "steps": args.steps, "repeats": args.repeats,
           "statistic": "median over repeats of (event time / steps)", "configs": {}}
    for cfg in args.configs.split(","):
        P, C, M, seed = CONFIGS[cfg]
        res = {}
        for w, h, scale in ((640, 480, 1), (160, 120, 4)):
            f = Frame(P, C, M, seed)
            maxq = max(600, C)
            p = prm3d_defaults(max_particles=P, max_components=maxq, max_measurements=M)
            p.max_quantity = maxq
            if scale != 1:   # the same scene in pixels of 1 / scale: noise, ramps and clutter density scaled with them
                p.measurer[0] = p.measurer[0] / scale
                p.measurer[3:7] = [-w // 2, -h // 2, w, h]
                p.R[0], p.R[4] = p.R[0] / scale ** 2, p.R[4] / scale ** 2
                p.visibility_ramp[0], p.visibility_ramp[1] = p.visibility_ramp[0] / scale, p.visibility_ramp[1] / scale
                p.clutter_density = p.clutter_density * scale ** 2
                f.z[:, :2] /= scale
            nav = navigator.PHDNavigator(p, particlecount=P)
            nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
            nav.set_measurements(f.z)
            nav.set_frozen(True)
            nav.set_all_pairs(True)
            nav.timing_reset(False)
            stream = torch.cuda.ExternalStream(nav._lib.phd_stream(nav._h))
            maps = {"none": None, "inf": np.full((h, w), np.inf, np.float32),
                    "occluding": kinect_ref.occluding_map(np.random.default_rng(7), w, h)}
            for case, depth in maps.items():
                nav.set_depth_map(depth)
                times = []
                for _ in range(args.repeats):
                    for _ in range(args.warmup):
                        nav.step_async(0.5)
                    nav.sync()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    for _ in range(args.steps):
                        nav.step_async(0.5)
                    b.record(stream)
                    nav.sync()
                    b.synchronize()
                    times.append(a.elapsed_time(b) / args.steps)
                res["%dx%d_%s" % (w, h, case)] = float(np.median(times))
            nav.close()
            base = res["%dx%d_none" % (w, h)]
            for case in ("inf", "occluding"):
                res["%dx%d_%s_ratio" % (w, h, case)] = res["%dx%d_%s" % (w, h, case)] / base
        out["configs"][cfg] = {"P": P, "C": C, "M": M, "ms": res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
