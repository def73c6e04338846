#!/usr/bin/env python3
"""Replay a monorfs record through the HIP solver: the measurements.out / odometry.out stream that
drives the C# solver with `-i=record` drives PHDNavigator here, and estimate.out / maps.out come back in the same
format (Simulation.SaveToFile, Simulation.cs:391-488).

    python scripts/replay.py <record.zip | record dir> [--particles N] [--seed S] [--out DIR] [--estimate poses|waypoints] [--posted [--map-error]
                             [--pose-error [--history timed|smooth|filter] [--reftime T]]]
    python scripts/replay.py --make DIR [--frames K]      # write a small synthetic record first

The host keeps what the reference keeps managed: the motion noise dt * chol(Q) * N(0, I) per particle and the
resampling uniform are drawn here (numpy), the motion step itself runs on the device (phd_update_motion).

estimate.out: with --estimate poses (the default) every frame's trajectory is the list of the best poses of the frames so
far; with --estimate waypoints it is what the reference writes, the best particle's own path (BestEstimate.WayPoints,
copied by Navigator.UpdateTrajectory, Navigator.cs:258-262), read from the trajectory log on the device
(phd_history_enable / phd_trajectories). The two differ whenever a step resamples or the best particle changes.

--posted: the whole record is posted to the device without a host wait between the first frame and the last (phd_step_async,
the map log phd_map_history_* and, for waypoints, the trajectory log); the two files are built afterwards from the logs and are
the same bytes.

--map-error (with --posted): the map-error time series of the post-analysis (Plot.MapError, postanalysis/Plot.cs:478-529) as well,
computed on the device over the map log (phd_map_error): maperror.out (OSPA) and spatialmaperror.out (its spatial part), one
`t value` line per frame in g6, with cut-off 1 and order 1 and without the alignment at a reference time. Truth is the visited
map of the record's vismaps.out where it has one (visited_map below), else the scene's landmarks.

--pose-error (with --posted --estimate waypoints): the four pose-error series of the post-analysis (Plot.LocationError,
RotationError, OdoLocationError, OdoRotationError, postanalysis/Plot.cs:293-456) as well, computed on the device over the trajectory
log (phd_pose_error): locerror.out, roterror.out, odolocerror.out, odoroterror.out, one `t value` line per value in g6. --history
is the post-analysis' -H (timed, the default: per frame the mean error of the whole path estimated then; smooth; filter),
--reftime its -t, turned into an entry by the binary search of Plot.cs:99-101 over the times of the log's entries. The truth is the
record's trajectory.out behind the scene's start pose for entry 0 (the constructor's waypoint); the time of the "SLAM ... on" tag
comes from tags.out (Plot.cs:343)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monorfs_amd import recordio as rio
from monorfs_amd.abi import prm3d_defaults



def frames_of(rec):
    odo = rio.timed_array_from_descriptor([l for l in rec["odometry.out"].split("\n") if l != ""], 6)
    z = rio.measurements_from_descriptor(rec["measurements.out"], 3)
    zt = {round(t, 9): pts for t, pts in z}
    return [(t, reading, zt.get(round(t, 9), np.zeros((0, 3)))) for t, reading in odo]


def config_of(rec):
    """the record's config.cfg over the defaults (Config.FromRecordFile, Config.cs:127-148), or the defaults"""
    return rio.config_from_descriptor(rec["config.cfg"].splitlines()) if "config.cfg" in rec else rio.default_config()


def params_of(rec, particles, maxm):
    pose, measurer, _ = rio.scene_from_descriptor(rec["scene.world"])
    p = rio.phd_params_from_config(config_of(rec), max_particles=particles, max_components=600, max_measurements=max(maxm, 1))
    if measurer is not None:
        p.measurer[:] = [measurer[0], float(np.float32(measurer[1])), float(np.float32(measurer[2]))] + list(measurer[3:7])
    return p, pose


def visited_map(frames):
    """Plot.VisitedMap (postanalysis/Plot.cs:230-248), the rule of monorfs_amd/host/Ospa.hpp::VisitedMap: the landmarks seen
    (weight > 0) in any frame so far, each once — a landmark is new when nothing already kept lies within 1e-5 of it.
    frames: per frame (weights[n], means[n][3]) of the visible landmarks. Returns the kept means, [k][3]."""
    kept = []
    for w, m in frames:
        for wi, x in zip(w, np.asarray(m, float).reshape(-1, 3)):
            if not wi > 0:
                continue
            if not any(np.sqrt(np.sum((c - x) ** 2)) <= 1e-5 for c in kept):
                kept.append(np.array(x))
    return np.array(kept).reshape(-1, 3)


def truth_of(rec):
    """what --map-error measures against: the visited map of vismaps.out, or the scene's landmarks"""
    if "vismaps.out" in rec:
        return visited_map([(mix[0], mix[1]) for _, mix in rio.map_history_from_descriptor(rec["vismaps.out"])])
    return np.asarray(rio.scene_from_descriptor(rec["scene.world"])[2], float).reshape(-1, 3)


def reference_entry(times, reftime):
    """Plot.RefTime (postanalysis/Plot.cs:99-101): List.BinarySearch for `reftime` among the entries' times — the index it hits, the
    first entry behind reftime where it hits none, 0 where reftime lies behind every entry"""
    lo, hi = 0, len(times) - 1
    while lo <= hi:
        mid = lo + ((hi - lo) >> 1)
        if times[mid] == reftime:
            return mid
        if times[mid] < reftime:
            lo = mid + 1
        else:
            hi = mid - 1
    return lo if lo != len(times) else 0


def slam_time_of(rec):
    """the time of the first tag that names SLAM and on, 0 without one (Plot.cs:343-346)"""
    tags = rio.timed_message_from_descriptor([l for l in rec.get("tags.out", "").split("\n") if l != ""])
    return next((t for t, message in tags if "SLAM" in message and "on" in message), 0.0)


def true_poses_of(rec):
    """what --pose-error measures against, one pose per entry of the trajectory log: the scene's start pose for entry 0
    (start_waypoints), then trajectory.out frame by frame. Returns (times[L], poses[L][7])."""
    traj = rio.timed_array_from_descriptor([l for l in rec["trajectory.out"].split("\n") if l != ""], 7)
    start = np.asarray(rio.scene_from_descriptor(rec["scene.world"])[0], float)
    return np.array([0.0] + [t for t, _ in traj]), np.array([start] + [np.asarray(x, float) for _, x in traj]).reshape(-1, 7)


class DeviceSolver:
    def __init__(self, p, pose, particles):
        from monorfs_amd import navigator
        self.nav = navigator.PHDNavigator(p, particlecount=particles)
        self.nav.reset(pose, (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3))), particles)

    def step(self, reading, noise, z, u):
        self.nav.UpdateOdometry(None, reading, noise)
        if len(z):
            self.nav.SlamUpdate(None, z, u_resample=u)
        b = self.nav.BestParticle
        return self.nav.poses()[b], self.nav.MapModel(b)

    def start_waypoints(self, capacity):
        """the trajectory log, with entry 0 at time 0 as Vehicle's constructor leaves it (Vehicle.cs:228)"""
        self.nav.enable_history(capacity)
        self.nav.append_history(0.0)

    def step_waypoints(self, time, reading, noise, z, u):
        """PHDNavigator.Update (:295-314): the motion step, its waypoint, then UpdateTrajectory's copy of BestEstimate.WayPoints
        (:313) — BestParticle is still the one the previous SlamUpdate left — and only then this frame's SlamUpdate"""
        self.nav.UpdateOdometry(time, reading, noise)   # (appends: the log is on)
        times, poses, _ = self.nav.WayPoints([self.nav.BestParticle])
        if len(z):
            self.nav.SlamUpdate(time, z, u_resample=u)
        return (times, poses[0]), self.nav.MapModel(self.nav.BestParticle)

    def start_posted(self, frames, components):
        """the map log (Navigator.WayMaps): one entry per frame"""
        self.nav.enable_map_history(frames, components)

    def post(self, time, reading, noise, z, u):
        """a frame with no getter and no wait: the motion step (and its waypoint if the trajectory log is on), the step if the
        frame has measurements, the best map behind it"""
        self.nav.UpdateOdometry(time, reading, noise)
        if len(z):
            self.nav.set_measurements(z)
            self.nav.step_async(u)
        self.nav.append_map_history(time)

    def finish_posted(self, waypoints):
        """per frame (best pose | the best particle's path as of the frame's Update, as step_waypoints copies it), best map"""
        self.nav.sync()   # (raises what a dropped step left)
        out, best = [], 0   # BestParticle = 0 after reset (PHDNavigator.cs:265)
        for k, (t, b, pose, model) in enumerate(self.nav.WayMaps()):
            if waypoints:
                times, poses, _ = self.nav.WayPointsAt(k + 1, [best])   # (entry 0 is start_waypoints')
                out.append(((times, poses[0]), model))
            else:
                out.append((pose, model))
            best = b
        return out

    def map_error(self, truth, cutoff=1.0, order=1.0):
        """per frame (time, ospa, cardinality, spatial, size) over the map log (phd_map_error)"""
        return self.nav.MapError(truth, cutoff, order)

    def pose_error(self, truth, mode, ref_entry, slam_time):
        """(times, location, rotation, odo_times, odo_location, odo_rotation) over the trajectory log (phd_pose_error): the
        estimate of every frame is the path finish_posted reads for it, the best particle of the map log; entry 0 is
        start_waypoints' and no frame's"""
        return self.nav.PoseError(truth, mode=mode, slots=None, first_entry=1, ref_entry=ref_entry, slam_time=slam_time)


def replay(rec, particles, seed, solver_cls, estimate="poses", map_error=False, pose_error=None, reftime=0.0, posted=False):
    if estimate not in ("poses", "waypoints"):
        raise ValueError("estimate is 'poses' or 'waypoints'")
    if map_error and not posted:
        raise ValueError("map_error needs posted: the metric is computed over the map log on the device")
    if pose_error is not None:
        if pose_error not in ("timed", "smooth", "filter"):
            raise ValueError("pose_error is None, 'timed', 'smooth' or 'filter'")
        if not posted or estimate != "waypoints":
            raise ValueError("pose_error needs posted and estimate='waypoints': the metric is computed over the trajectory log on the device")
    frames = frames_of(rec)
    p, pose = params_of(rec, particles, max(len(z) for _, _, z in frames))
    solver = solver_cls(p, pose, particles)
    if posted:   # (the map log first: phd_pose_error takes the estimates from it only if it was on when every waypoint was made)
        solver.start_posted(len(frames), len(frames) * p.max_components)
    if estimate == "waypoints":
        solver.start_waypoints(len(frames) + 1)
    rng = np.random.default_rng(seed)
    cfg = config_of(rec)
    chol = np.linalg.cholesky(cfg["MotionCovarianceMultiplier"] * np.array(cfg["MotionCovariance"], float))   # PHDNavigator.cs:257-259
    trajectory, history, maps = [], [], []
    tprev = frames[0][0]
    for t, reading, z in frames:
        dt = t - tprev
        tprev = t
        noise = dt * (rng.normal(size=(particles, 6)) @ chol.T)     # Util.RandomGaussianVector, Util.cs:173-202
        u = float(rng.uniform(1e-6, 1.0))
        if posted:
            solver.post(t, reading, noise, z, u)
        elif estimate == "waypoints":
            (wt, wp), bmap = solver.step_waypoints(t, reading, noise, z, u)
            history.append((t, [(float(a), np.array(b)) for a, b in zip(wt, wp)]))
        else:
            bpose, bmap = solver.step(reading, noise, z, u)
            trajectory.append((t, bpose))
            history.append((t, list(trajectory)))
        if not posted:
            maps.append((t, bmap))
    if posted:
        for (t, _, _), (est, bmap) in zip(frames, solver.finish_posted(estimate == "waypoints")):
            if estimate == "waypoints":
                history.append((t, [(float(a), np.array(b)) for a, b in zip(*est)]))
            else:
                trajectory.append((t, est))
                history.append((t, list(trajectory)))
            maps.append((t, bmap))
    out = {"estimate.out": rio.serialize_trajectories(history), "maps.out": rio.serialize_maps(maps)}
    if map_error:
        series = solver.map_error(truth_of(rec))
        out["maperror.out"] = rio.serialize_timed_array([(t, [e[1]]) for (t, _, _), e in zip(frames, series)])
        out["spatialmaperror.out"] = rio.serialize_timed_array([(t, [e[3]]) for (t, _, _), e in zip(frames, series)])
    if pose_error is not None:
        times, truth = true_poses_of(rec)
        if len(truth) != len(frames) + 1:
            raise ValueError("trajectory.out has %d poses for %d frames" % (len(truth) - 1, len(frames)))
        times[1:] = [t for t, _, _ in frames]   # (the log's times: the frames')
        t, loc, rot, ot, oloc, orot = solver.pose_error(truth, pose_error, reference_entry(list(times), reftime), slam_time_of(rec))
        out["locerror.out"] = rio.serialize_timed_array([(a, [b]) for a, b in zip(t, loc)])
        out["roterror.out"] = rio.serialize_timed_array([(a, [b]) for a, b in zip(t, rot)])
        out["odolocerror.out"] = rio.serialize_timed_array([(a, [b]) for a, b in zip(ot, oloc)])
        out["odoroterror.out"] = rio.serialize_timed_array([(a, [b]) for a, b in zip(ot, orot)])
    return out


def make_synthetic_record(path, frames=12, landmarks=14, seed=3):
    """a vehicle drifting forward past a handful of landmarks; measurements = MeasurePerfect + N(0, R) of the visible
    ones (+ one clutter point now and then), written exactly as Simulation.SaveToFile would"""
    from monorfs_amd import prm3d
    from monorfs_amd.pose3d import add_odometry
    rng = np.random.default_rng(seed)
    p = prm3d_defaults()
    focal, measurer, ramp = p.measurer[0], list(p.measurer), list(p.visibility_ramp)
    pose = np.array([0, 0, 0, 1.0, 0, 0, 0])
    zs = np.column_stack([rng.uniform(-260, 260, landmarks), rng.uniform(-190, 190, landmarks), rng.uniform(0.5, 1.6, landmarks)])
    lm = np.array([prm3d.measure_to_map(pose, z, focal) for z in zs])
    scene = rio.serialize_scene(pose, p.measurer, lm)
    _, _, lm = rio.scene_from_descriptor(scene)                     # what a reader of the file sees
    odo, meas, traj = [], [], []
    R = np.array(p.R).reshape(3, 3)
    for k in range(frames):
        t = k / 30.0
        reading = np.array([0.004, 0.001 * np.sin(k), 0.006, 0.002, -0.001, 0.0005]) if k else np.zeros(6)
        pose = add_odometry(pose, reading)
        pts = []
        for x in lm:
            z = prm3d.measure_perfect(pose, x, focal)
            if prm3d.fuzzy_visible(z, measurer, ramp) > 0 and rng.uniform() < 0.9:
                pts.append(z + rng.normal(size=3) * np.sqrt(np.diag(R)))
        if k % 4 == 1:
            pts.append([rng.uniform(-300, 300), rng.uniform(-220, 220), rng.uniform(0.3, 1.8)])
        odo.append((t, reading))
        meas.append((t, pts))
        traj.append((t, pose))
    rio.write_record(path, {"scene.world": scene, "odometry.out": rio.serialize_timed_array(odo),
                            "measurements.out": rio.serialize_measurements(meas), "trajectory.out": rio.serialize_timed_array(traj),
                            "tags.out": "0 SLAM mode on", "config.cfg": rio.serialize_config(rio.default_config())})
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("record", nargs="?")
    ap.add_argument("--make")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--particles", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out")
    ap.add_argument("--estimate", choices=("poses", "waypoints"), default="poses")
    ap.add_argument("--posted", action="store_true", help="post the whole record without a host wait; the files are built from the device's logs")
    ap.add_argument("--map-error", action="store_true", help="with --posted: maperror.out and spatialmaperror.out from the device's map log")
    ap.add_argument("--pose-error", action="store_true", help="with --posted --estimate waypoints: locerror.out, roterror.out, odolocerror.out and odoroterror.out "
                                                              "from the device's trajectory log")
    ap.add_argument("--history", choices=("timed", "smooth", "filter"), default="timed", help="the history mode of --pose-error (postanalysis -H)")
    ap.add_argument("--reftime", type=float, default=0.0, help="the reference time of --pose-error (postanalysis -t)")
    a = ap.parse_args()
    if a.map_error and not a.posted:
        ap.error("--map-error needs --posted")
    if a.pose_error and not (a.posted and a.estimate == "waypoints"):
        ap.error("--pose-error needs --posted --estimate waypoints")
    if a.make:
        print("wrote", make_synthetic_record(a.make, a.frames))
        if not a.record:
            return
    rec = rio.read_record(a.record)
    out = replay(rec, a.particles, a.seed, DeviceSolver, estimate=a.estimate, map_error=a.map_error, posted=a.posted,
                 pose_error=a.history if a.pose_error else None, reftime=a.reftime)
    if a.out:
        rio.write_record(a.out, dict(rec, **out))
    maps = rio.map_history_from_descriptor(out["maps.out"])
    print("replayed %d frames, final map: %d components, expected size %.3f" % (len(maps), len(maps[-1][1][0]), maps[-1][1][0].sum()))


if __name__ == "__main__":
    main()
