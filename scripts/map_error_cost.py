"""What the map-error series costs on the device against the route a host had before it.

  device  phd_map_error over a map log of config-A-like maps (128 components, 40 truth points): the whole call, which waits
          for the device and copies the five small arrays back.
  host    the same series the way a host got it before: phd_map_history (the entry table and every component of the log over
          PCIe, converted to w / mean3 / cov9), then Map.BestMapEstimate and Plot.MapError per entry on one core, here with
          the C++ oracle's (oracle/phd_oracle.cpp: orc.best_map_estimate, orc.map_error) through ctypes.
Both legs read the same log, alternated in one process; the first round warms up and is not counted. The log is made without
steps: set_map on the best particle and an append per entry, the maps drawn around the truth set (a fifth of the components
far from it, one component heavy enough to be picked twice).

Prints one JSON line.   python scripts/map_error_cost.py [--entries 100,1000] [--repeats 5] [--components 128] [--truth 40]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def draw_map(rng, truth, n):
    w = rng.uniform(0.3, 1.3, n)
    w[0] = 2.6
    mean = truth[rng.integers(0, len(truth), n)] + rng.normal(0, 0.05, (n, 3))
    far = rng.uniform(size=n) < 0.2
    mean[far] += rng.uniform(3, 4, (int(far.sum()), 3))
    return w, mean, np.tile(np.eye(3), (n, 1, 1))


def host_route(nav, orc, truth, cutoff, order):
    out = []
    for t, best, pose, model in nav.WayMaps():
        est = orc.best_map_estimate(model)[0]
        ospa, spatial = orc.map_error(truth, est, cutoff=cutoff, order=order)
        out.append((t, ospa, spatial, len(est)))
    return out


def cost(navigator, prm3d_defaults, orc, entries, components, ntruth, repeats, cutoff=1.0, order=1.0):
    rng = np.random.default_rng(entries)
    truth = rng.uniform(-2, 2, (ntruth, 3))
    p = prm3d_defaults(max_particles=4, max_components=max(600, components), max_measurements=8)
    nav = navigator.PHDNavigator(p, particlecount=4)
    nav.timing_reset(False)
    nav.enable_map_history(entries, entries * components)
    for k in range(entries):
        nav.set_map(0, draw_map(rng, truth, components))
        nav.append_map_history(k / 30.0)
    nav.sync()
    ms = {"device": [], "host": [], "host_download": []}
    worst = 0.0
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        dev = nav.MapError(truth, cutoff, order)
        t1 = time.perf_counter()
        nav.WayMaps()
        t2 = time.perf_counter()
        host = host_route(nav, orc, truth, cutoff, order)
        t3 = time.perf_counter()
        if rep:
            ms["device"].append((t1 - t0) * 1e3)
            ms["host_download"].append((t2 - t1) * 1e3)
            ms["host"].append((t3 - t2) * 1e3)
        assert len(dev) == len(host) == entries
        for d, h in zip(dev, host):
            assert d[4] == h[3], "sizes differ"
            worst = max(worst, abs(d[1] - h[1]), abs(d[3] - h[2]))
    nav.close()
    out = {"entries": entries, "components": components, "truth": ntruth, "estimate_sizes": [min(d[4] for d in dev), max(d[4] for d in dev)],
           "max_abs_difference": worst}
    for leg in ms:
        out["ms_" + leg] = ms[leg]
        out["median_" + leg] = float(np.median(ms[leg]))
    out["host_over_device"] = out["median_host"] / out["median_device"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="100,1000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--components", type=int, default=128)
    ap.add_argument("--truth", type=int, default=40)
    args = ap.parse_args()
    import orc
    from monorfs_amd import navigator
    from monorfs_amd.abi import prm3d_defaults
    out = {"metric": "map error of a whole log: ms of phd_map_error against phd_map_history + the oracle's metric per entry on one core", "log": {}}
    for n in [int(e) for e in args.entries.split(",") if e]:
        out["log"][str(n)] = cost(navigator, prm3d_defaults, orc, n, args.components, args.truth, args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
