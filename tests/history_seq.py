"""The twelve-frame sequence of tests/test_gpu_history.py, the list model the trajectory log is checked against, and the
oracle's run of the sequence (which frames resample). No GPU is needed for anything here.

The model is the reference's, a list per particle (Vehicle.WayPoints): an append pushes (i, pose of particle i) onto particle
i's list; a step that resampled replaces the lists by new[i] = copy(old[source[i]]) (ResampleParticles, PHDNavigator.cs:740)."""
import functools

import numpy as np

import orc
from monorfs_amd.abi import prm3d_defaults
from monorfs_amd.synth import Frame

FRAMES = 12
SKEWED = (2, 3, 7, 10)                       # frames whose weights are all on one particle
READING = np.array([1e-3, 0, 0, 0, 0, 0])
# (particles, seed, min_effective_particle, PHD_NR_GRID_MIN or None): below a wave, the wave edge, more than one workgroup of
# 256 threads, and the resampling over a grid of workgroups (k_nr_*)
CASES = [(5, 13, 0.3, None), (64, 12, 0.1, None), (65, 12, 0.1, None), (257, 11, 0.1, None), (300, 12, 0.1, 1)]
CASE_IDS = ["P5", "P64", "P65", "P257", "P300-grid"]


def frame_of(case):
    P, seed = case[0], case[1]
    return Frame(P, 24, 8, seed, weight_profile="steady")


def params_of(case, **over):
    f = frame_of(case)
    p = prm3d_defaults(max_particles=f.P, max_components=600, max_measurements=max(f.M, over.pop("max_measurements", 0)))
    p.min_effective_particle = case[2]
    for k, v in over.items():
        setattr(p, k, v)
    return p


def skewed_weights(P, k):
    w = np.full(P, 1e-6)
    w[(3 * k) % P] = 1.0
    return w / w.sum()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """per frame: (time, noise[P][6], weights[P], z[M][3], u)"""
    P, seed = case[0], case[1]
    f = frame_of(case)
    rng = np.random.default_rng(seed)
    out = []
    for k in range(FRAMES):
        noise = (1.0 / 30) * rng.normal(size=(P, 6)) * np.sqrt([5e-3] * 3 + [2e-4] * 3)
        w = skewed_weights(P, k) if k in SKEWED else np.full(P, 1.0 / P)
        z = f.z + rng.normal(size=f.z.shape) * np.sqrt([2.0, 2.0, 1e-3]) * 0.3
        u = float(rng.uniform(0.05, 0.95))
        out.append((k / 30.0, noise, w, z, u))
    return out


def oracle_state(f, cap=700):
    st = orc.State(f.P, cap)
    st.poses[:] = f.poses
    st.w[:, :f.C], st.mean[:, :f.C], st.cov[:, :f.C], st.n[:] = f.w, f.mean, f.cov, f.C
    return st


class ListModel:
    """lists per particle, as arrays: slots[P][L], poses[P][L][7], times[L]"""

    def __init__(self, P):
        self.P = P
        self.times = np.zeros(0)
        self.slots = np.zeros((P, 0), np.int32)
        self.poses = np.zeros((P, 0, 7))

    def append(self, time, poses):
        self.times = np.append(self.times, float(time))
        self.slots = np.concatenate([self.slots, np.arange(self.P, dtype=np.int32)[:, None]], axis=1)
        self.poses = np.concatenate([self.poses, np.asarray(poses, float).reshape(self.P, 1, 7)], axis=1)

    def resample(self, src):
        src = np.asarray(src)
        self.slots, self.poses = self.slots[src].copy(), self.poses[src].copy()

    def copy(self):
        m = ListModel(self.P)
        m.times, m.slots, m.poses = self.times.copy(), self.slots.copy(), self.poses.copy()
        return m


@functools.lru_cache(maxsize=None)
def oracle_run(case, skip=()):
    """the sequence through the oracle alone: per frame (poses after the motion step, sources, resampled, best). Frames in
    `skip` take the motion step but no SlamUpdate (a dropped step)."""
    f = frame_of(case)
    p = params_of(case)
    st = oracle_state(f)
    out = []
    for k, (t, noise, w, z, u) in enumerate(inputs(case)):
        st.poses[:] = orc.update_motion(st.poses, READING, noise, False)
        moved = st.poses.copy()
        st.weights[:] = w
        if k in skip:
            out.append((moved, np.arange(f.P), False, -1))
            continue
        best, src, res, _ = orc.slam_update(p, st, z, u=u, threads=8)
        out.append((moved, np.array(src), bool(res), int(best)))
    return out


def pattern(case):
    return "".join("1" if r[2] else "0" for r in oracle_run(case))


def pattern_ok(pat):
    """at least 3 frames resample, at least 3 do not, and two adjacent frames both resample"""
    return pat.count("1") >= 3 and pat.count("0") >= 3 and "11" in pat
