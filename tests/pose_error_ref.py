"""The pose-error series of the reference's post-analysis, restated in numpy from postanalysis/Plot.cs:293-456 and the pose
arithmetic it calls (BaseStructures/Poses/Pose3D.cs, Quaternion.cs, Util/Util.cs) — not from include/phdhip.h and not from
monorfs_amd/host/PoseError.hpp: the tests hold both of those against this file.

A trajectory (TimedState) is a list of (time, state[7]); an estimate history (TimedTrajectory) a list of (time, trajectory).
Two departures from the text of Plot.cs, both stated where they are made: the two acos arguments are clamped to [-1, 1]
(Math.Acos returns NaN one ulp above 1), and Filter mode takes every estimate's newest pose against the truth of that
pose's entry (the reference's Estimate[i].Item2[i] against Trajectory[i] is that when the estimates start at entry 0)."""
import math

import numpy as np

TIMED, SMOOTH, FILTER = "timed", "smooth", "filter"


# Everything below works on whole trajectories at once: a quaternion argument is an array [n][4] (w x y z), a location [n][3];
# the operations per element and their order are the reference's.
# ---- Quaternion.cs
def q_mul(a, b):                                  # :295-301
    return np.stack([a[:, 0] * b[:, 0] - (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2] + a[:, 3] * b[:, 3]),
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2],
                     a[:, 0] * b[:, 2] + a[:, 2] * b[:, 0] + a[:, 3] * b[:, 1] - a[:, 1] * b[:, 3],
                     a[:, 0] * b[:, 3] + a[:, 3] * b[:, 0] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]], axis=1)


def q_conjugate(q):                               # :155-158
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def q_normalize(q):                               # :240-245: alpha = 1 / Magnitude
    alpha = 1 / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    return alpha[:, None] * q


def _euclidean(v):
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def q_exp(lie):                                   # :185-196
    phi = _euclidean(lie)
    small = phi < 1e-12
    unit = lie / np.where(small, 1.0, phi)[:, None]
    q = np.concatenate([np.cos(phi)[:, None], np.sin(phi)[:, None] * unit], axis=1)
    q[small] = [1.0, 0.0, 0.0, 0.0]
    return q


def q_log(q):                                     # :203-217
    q = q_normalize(q)
    phi = np.arccos(np.minimum(1.0, np.maximum(-1.0, q[:, 0])))   # (clamped)
    mag = _euclidean(q[:, 1:])
    small = mag < 1e-12
    lie = phi[:, None] * (q[:, 1:] / np.where(small, 1.0, mag)[:, None])
    lie[small] = 0.0
    return lie


# ---- Pose3D.cs (poses are (location[n][3], orientation[n][4]))
def from_state(states):                           # :142-162
    s = np.asarray(states, float).reshape(-1, 7)
    a = 1.0 / np.sqrt(s[:, 3] * s[:, 3] + s[:, 4] * s[:, 4] + s[:, 5] * s[:, 5] + s[:, 6] * s[:, 6])
    return s[:, :3].copy(), a[:, None] * s[:, 3:7]


def _pure(v):
    return np.concatenate([np.zeros((len(v), 1)), v], axis=1)


def pose_add(pose, delta):                        # :282-291
    loc, q = pose
    neworientation = q_mul(q, q_exp(0.5 * delta[:, 3:6]))
    dlocation = q_mul(q_mul(q, _pure(delta[:, :3])), q_conjugate(q))
    return loc + dlocation[:, 1:], q_normalize(neworientation)


def pose_subtract(pose, origin):                  # :297-308
    dq = q_mul(q_conjugate(origin[1]), pose[1])
    dxglobal = pose[0] - origin[0]
    dx = q_mul(q_mul(q_conjugate(origin[1]), _pure(dxglobal)), origin[1])
    lie = 2 * q_log(dq)                           # Quaternion.ToLinear, Quaternion.cs:135-139
    return np.concatenate([dx[:, 1:], lie], axis=1)


def from_linear(linear):                          # :247-250
    n = len(linear)
    return pose_add((np.zeros((n, 3)), np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))), linear)


def normalize_angle(angle):                       # Util.cs:79-87
    normal = np.fmod(angle + math.pi, 2 * math.pi)
    normal = np.where(normal >= 0, normal, normal + 2 * math.pi)
    return normal - math.pi


# ---- Plot.cs
def diffloc(a, b):                                # :445-448
    return _euclidean(from_linear(pose_subtract(a, b))[0])


def diffrot(a, b):                                # :450-456
    w = from_linear(pose_subtract(a, b))[1][:, 0]
    rawangle = 2 * np.arccos(np.minimum(1.0, np.maximum(-1.0, w)))   # Quaternion.Angle, Quaternion.cs:71-74 (clamped)
    return np.abs(normalize_angle(rawangle))


def _arrays(path):
    """a TimedState as (times[n], states[n][7])"""
    if isinstance(path, tuple) and len(path) == 2 and isinstance(path[1], np.ndarray) and path[1].ndim == 2:
        return path
    return np.array([t for t, _ in path], float), np.array([x for _, x in path], float).reshape(-1, 7)


def _relative(states, index, origin):
    return from_linear(pose_subtract(from_state(states[index]), from_state(states[origin])))


class _Series:
    """one of the four internal errors: which poses entry i is taken relative to, and which difference is reported"""

    def __init__(self, name, diff, odometry):
        self.__name__, self.diff, self.odometry = name, diff, odometry

    def indices(self, n, reftime):
        if self.odometry:                          # for (int i = 10; i < estimate.Count; i++): against i - 10
            index = np.arange(10, max(n, 10))
            return index, index - 10
        index = np.arange(n)                       # for (int i = 0; i < estimate.Count; i++): against min(i, RefTime)
        return index, np.minimum(index, reftime)

    def values(self, truth, states, index, origin):
        if len(index) == 0:
            return np.zeros(0)
        return self.diff(_relative(truth, index, origin), _relative(states, index, origin))

    def series(self, times, values):
        if self.odometry:                          # error.Add(Tuple.Create(groundtruth[0].Item1, 0.0)) first
            return [(times[0], 0.0)] + [(times[10 + j], float(v)) for j, v in enumerate(values)]
        return [(times[i], float(v)) for i, v in enumerate(values)]

    def __call__(self, groundtruth, estimate, reftime=0):
        gt, g = _arrays(groundtruth)
        _, e = _arrays(estimate)
        index, origin = self.indices(len(e), reftime)
        return self.series(gt, self.values(g, e, index, origin))

    def many(self, groundtruth, estimates, reftime):
        """__call__ for several estimates, the same operations per value: all their poses go through the arithmetic side by side"""
        gt, g = _arrays(groundtruth)
        paths = [_arrays(e)[1] for e in estimates]
        pairs = [self.indices(len(e), reftime) for e in paths]
        offset = np.cumsum([0] + [len(e) for e in paths])
        index = np.concatenate([i for i, _ in pairs])
        origin = np.concatenate([o for _, o in pairs])
        shift = np.concatenate([np.full(len(i), offset[k]) for k, (i, _) in enumerate(pairs)])
        values = self.values(g, np.concatenate(paths), index, origin) if len(index) == 0 else self.diff(
            _relative(g, index, origin), _relative(np.concatenate(paths), index + shift, origin + shift))
        cuts = np.cumsum([len(i) for i, _ in pairs])[:-1]
        return [self.series(gt, v) for v in np.split(values, cuts)]


location_error0 = _Series("location_error0", diffloc, False)           # :371-387
rotation_error0 = _Series("rotation_error0", diffrot, False)           # :389-405
odolocation_error0 = _Series("odolocation_error0", diffloc, True)      # :407-424
odorotation_error0 = _Series("odorotation_error0", diffrot, True)      # :426-443


def pose_error(internalerror, mode, trajectory, estimate, reftime, slamtime, memo=None):   # :325-369
    """memo: a dict that keeps a path's per-pose errors by (series, length of the path, reftime) between calls over the same
    trajectory and estimates; None: nothing is kept"""
    if mode == SMOOTH:
        return internalerror(trajectory, estimate[-1][1], reftime)
    if mode == FILTER:
        # (the newest pose of every estimate, against the truth of the same entry: see the head of this file)
        newest = [(t, path[len(path) - 1][1]) for t, path in estimate]
        truth = [trajectory[len(path) - 1] for _, path in estimate]
        return internalerror(truth, newest, reftime)
    if mode != TIMED:
        raise ValueError(mode)
    memo = {} if memo is None else memo
    keys = [(internalerror.__name__, len(path), None if internalerror.odometry else reftime) for _, path in estimate]
    missing = [i for i, k in enumerate(keys) if k not in memo]
    if missing:                                     # TimedValue localerror = internalerror(Trajectory, Estimate[i].Item2)
        for i, localerror in zip(missing, internalerror.many(trajectory, [estimate[i][1] for i in missing], reftime)):
            memo[keys[i]] = np.array([v for _, v in localerror], float)
    error, startindex = [], 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for (t, path), key in zip(estimate, keys):
            values = memo[key]
            # mean = 0; mean += localerror[k] for k = startindex .. Count - 1, one by one in this order: what accumulate does
            mean = np.add.accumulate(values[startindex:])[-1] if startindex < len(values) else np.float64(0)
            mean = mean / np.float64(len(values) - startindex)   # (a double division: 0 / 0 is NaN, 0 / -2 is -0)
            error.append((t, float(mean)))
            if t < slamtime:
                startindex += 1
    return error


SERIES = (location_error0, rotation_error0, odolocation_error0, odorotation_error0)


def all_series(mode, trajectory, estimate, reftime=0, slamtime=0.0, memo=None):
    """the four series as (times, values) arrays: location, rotation, odometry location, odometry rotation"""
    out = []
    for f in SERIES:
        s = pose_error(f, mode, trajectory, estimate, reftime, slamtime, memo)
        out.append((np.array([a for a, _ in s], float), np.array([b for _, b in s], float)))
    return out


def histories(times, truth, paths, first_entry):
    """(trajectory, estimate) from a log: truth[L][7] at times[L]; paths[i] = the estimated path as of entry i (i + 1 poses),
    used for i >= first_entry"""
    trajectory = [(float(times[k]), np.asarray(truth[k], float)) for k in range(len(times))]
    estimate = [(float(times[i]), [(float(times[k]), np.asarray(paths[i][k], float)) for k in range(i + 1)]) for i in range(first_entry, len(times))]
    return trajectory, estimate
