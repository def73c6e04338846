"""Python host-side mirror of the reference's solver interface for the PHD path.

`PHDNavigator` here keeps the member names of
    class PHDNavigator<MeasurerT, PoseT, MeasurementT> : Navigator<...>
    (mono-rfs-lib/SLAM/Navigators/PHDNavigator.cs:52-983, Navigator.cs:47-396)
and forwards every one of them to libphdhip.so through the C-ABI of include/phdhip.h — it is what
tests/ and bench.py drive; the C++ twin for native hosts is monorfs_amd/host/PHDNavigator.hpp and the
C# adapter a maintainer would add is bindings/csharp/HipPHDNavigator.cs.

No compute happens in this file: it marshals arrays and raises on a non-zero status."""
import ctypes as C

import numpy as np

from . import _lib
from .abi import (PHD_ERR_ASSOCIATION, PHD_ERR_CAPACITY, PHD_STAGE_CORRECTED, PHD_STAGE_PREDICTED, PHD_STAGE_PRUNED, PhdParams,
                  prm3d_defaults)

dp = _lib.dp
ip = _lib.ip
i64p = _lib.i64p


def pose3d_add(pose7, delta6):
    """Pose3D.Add (Pose3D.cs:282-291): x + q dx q*, q Exp(dr / 2) normalised"""
    x, q = np.asarray(pose7[:3], float), np.asarray(pose7[3:], float)
    lie = 0.5 * np.asarray(delta6[3:], float)
    phi = np.linalg.norm(lie)
    dq = np.array([1.0, 0, 0, 0]) if phi < 1e-12 else np.concatenate([[np.cos(phi)], np.sin(phi) * (lie / phi)])

    def mul(a, b):
        return np.array([a[0] * b[0] - (a[1] * b[1] + a[2] * b[2] + a[3] * b[3]),
                         a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                         a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])
    nq = mul(q, dq)
    nq = nq / np.linalg.norm(nq)
    dl = mul(mul(q, np.concatenate([[0.0], np.asarray(delta6[:3], float)])), q * [1, -1, -1, -1])
    return np.concatenate([x + dl[1:], nq])


class PHDError(RuntimeError):
    """≙ the InvalidOperationException with Data["module"] that Simulation.Update catches
    (Simulation.cs:655-670); `module` is "association" for PHD_ERR_ASSOCIATION."""

    def __init__(self, status, message):
        super().__init__("libphdhip status %d: %s" % (status, message))
        self.status = status
        self.module = "association" if status == PHD_ERR_ASSOCIATION else "phdhip"


def _ptr(a):
    return a.ctypes.data_as(dp)


class PHDNavigator:
    def __init__(self, params: PhdParams = None, particlecount=1, onlymapping=False, device=0,
                 pose=(0, 0, 0, 1, 0, 0, 0), devices=None):
        """≙ new PHDNavigator(vehicle, particlecount, onlymapping) (PHDNavigator.cs:192-208).
        devices: a list of HIP ordinals -> one multi-device handle (phd_create_multi), the particles sharded
        contiguously over them; params.max_particles and the particle count are then totals (multiples of len(devices))."""
        self._lib = _lib.load()
        self.params = params if params is not None else prm3d_defaults(max_particles=max(1, particlecount))
        if devices is not None:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            self._h = self._lib.phd_create_multi(C.byref(self.params), devs, len(devices))
        else:
            self._h = self._lib.phd_create(C.byref(self.params), device)
        if not self._h:
            raise PHDError(-1, self._lib.phd_create_error().decode())
        self._history, self._history_len = False, 0   # the trajectory log is on | its entries (the library's count, mirrored)
        self._map_history, self._map_history_len = False, 0   # ... the map log
        self.ParticleCount = particlecount
        self.OnlyMapping = bool(onlymapping)
        n = 1 if onlymapping else particlecount   # :201-203
        self.reset(np.asarray(pose, float), (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3))), n)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc != 0:
            raise PHDError(rc, self._lib.phd_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.phd_destroy(self._h)
            self._h = None

    Dispose = close   # Navigator.Dispose (Navigator.cs:395)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ state
    def reset(self, pose, model, particlecount):
        """≙ PHDNavigator.reset (:245-266)."""
        w, m, c = (np.ascontiguousarray(x, np.float64) for x in model)
        pose = np.ascontiguousarray(pose, np.float64)
        self._check(self._lib.phd_reset(self._h, int(particlecount), _ptr(pose), _ptr(w), _ptr(m), _ptr(c), len(w)))
        self._history_len = self._map_history_len = 0   # (the library restarts the logs)

    def CollapseParticles(self, particlecount):
        """≙ :233-236: every particle becomes a copy of the best one."""
        best = self.BestParticle
        pose = self.poses()[best]
        self.reset(pose, self.MapModel(best), particlecount)

    def ResetMapModel(self):
        """≙ :271-276."""
        empty = (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3)))
        poses, weights = self.poses().copy(), self.VehicleWeights.copy()
        for i in range(self.particle_count):
            self.set_map(i, empty)
        self.set_poses(poses)
        self.set_weights(weights)

    @property
    def particle_count(self):
        return self._lib.phd_particle_count(self._h)

    def set_poses(self, poses):
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        self._check(self._lib.phd_set_poses(self._h, _ptr(poses), len(poses)))

    def set_weights(self, weights):
        weights = np.ascontiguousarray(weights, np.float64)
        self._check(self._lib.phd_set_weights(self._h, _ptr(weights), len(weights)))

    def set_map(self, particle, model):
        w, m, c = (np.ascontiguousarray(x, np.float64) for x in model)
        self._check(self._lib.phd_set_map(self._h, int(particle), _ptr(w), _ptr(m), _ptr(c), len(w)))

    def upload_state(self, planes, counts, poses, weights):
        """planes: [10][P][stride] float64 in the device layout (w, mean xyz, cov xx xy xz yy yz zz)."""
        planes = np.ascontiguousarray(planes, np.float64)
        counts = np.ascontiguousarray(counts, np.int32)
        poses = np.ascontiguousarray(poses, np.float64)
        weights = np.ascontiguousarray(weights, np.float64)
        _, P, stride = planes.shape
        self._check(self._lib.phd_upload_state_soa(self._h, P, stride, _ptr(planes), counts.ctypes.data_as(ip),
                                                   _ptr(poses), _ptr(weights)))
        self._history_len = self._map_history_len = 0

    def download_state(self, stride):
        P = self.particle_count
        planes = np.zeros((10, P, stride))
        counts = np.zeros(P, np.int32)
        poses = np.zeros((P, 7))
        weights = np.zeros(P)
        self._check(self._lib.phd_download_state_soa(self._h, stride, _ptr(planes), counts.ctypes.data_as(ip),
                                                     _ptr(poses), _ptr(weights)))
        return planes, counts, poses, weights

    def poses(self):
        n = C.c_int32(0)
        ptr = self._lib.phd_poses(self._h, C.byref(n))
        if not ptr:
            raise PHDError(-1, self._lib.phd_last_error(self._h).decode())
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).reshape(-1, 7).copy()

    # ------------------------------------------------------------------ Navigator interface
    def Update(self, time, poses):
        """≙ PHDNavigator.Update (:295-314). The motion model and its RNG stay on the host
        (TrackVehicle.UpdateNoisy): the caller hands over the propagated particle poses."""
        self.set_poses(poses)
        if self._history:
            self.append_history(time)

    def UpdateOdometry(self, time, reading, noise=None, perfect_still=False):
        """≙ PHDNavigator.Update (:295-314) with the motion step on the device (phd_update_motion):
        `reading` is the odometry (dx dy dz dpitch dyaw droll), `noise` the per-particle vectors
        dt * chol(MotionCovariance) * N(0, I) the host drew (TrackVehicle.UpdateNoisy, TrackVehicle.cs:89-102)."""
        reading = np.ascontiguousarray(reading, np.float64).reshape(6)
        if noise is not None:
            noise = np.ascontiguousarray(noise, np.float64).reshape(-1, 6)
            if len(noise) != self.particle_count:
                raise ValueError("one noise vector per particle")
        self._check(self._lib.phd_update_motion(self._h, _ptr(reading), _ptr(noise) if noise is not None else None,
                                                self.particle_count, int(bool(perfect_still))))
        if self._history:
            self.append_history(time)

    # ------------------------------------------------------------------ trajectories (Vehicle.WayPoints per particle)
    def enable_history(self, capacity):
        """The trajectory log on the device (phd_history_enable): room for `capacity` entries, one per Update / UpdateOdometry
        from now on; 0 switches it off. Every call restarts the log at length 0 (ResetHistory)."""
        self._check(self._lib.phd_history_enable(self._h, int(capacity)))
        self._history = int(capacity) > 0
        self._history_len = 0

    def append_history(self, time=None):
        """One entry of the log: the current particle poses (phd_history_append; asynchronous). time=None: the entry's index."""
        if time is None:
            time = float(self.history_length)
        self._check(self._lib.phd_history_append(self._h, float(time)))
        self._history_len += 1

    @property
    def history_length(self):
        return self._history_len if self._history else 0

    def WayPoints(self, particles):
        """≙ VehicleParticles[i].WayPoints (Vehicle.cs:141) for the listed particles of the current state, as the reference's
        deep copies in ResampleParticles (:740) leave them: (times[L], poses[n][L][7], slots[n][L]), oldest entry first;
        slots[j][k] is the slot the ancestor of particles[j] held at entry k (phd_trajectories; waits for the device)."""
        q = np.ascontiguousarray(list(particles) if not isinstance(particles, np.ndarray) else particles, np.int32).reshape(-1)
        n = C.c_int(0)
        t, x, s = dp(), dp(), ip()
        self._check(self._lib.phd_trajectories(self._h, q.ctypes.data_as(ip), len(q), C.byref(n), C.byref(t), C.byref(x), C.byref(s)))
        L = n.value
        if L == 0:
            return np.zeros(0), np.zeros((len(q), 0, 7)), np.zeros((len(q), 0), np.int32)
        return (np.ctypeslib.as_array(t, shape=(L,)).copy(), np.ctypeslib.as_array(x, shape=(len(q) * L * 7,)).reshape(len(q), L, 7).copy(),
                np.ctypeslib.as_array(s, shape=(len(q) * L,)).reshape(len(q), L).copy())

    def WayPointsAt(self, entry, slots):
        """WayPoints as they were at trajectory-log entry `entry`, for the particles that held `slots` then: entry + 1 entries,
        nothing that resampled later enters (phd_trajectories_at; waits for the device)."""
        q = np.ascontiguousarray(list(slots) if not isinstance(slots, np.ndarray) else slots, np.int32).reshape(-1)
        n = C.c_int(0)
        t, x, s = dp(), dp(), ip()
        self._check(self._lib.phd_trajectories_at(self._h, int(entry), q.ctypes.data_as(ip), len(q), C.byref(n), C.byref(t), C.byref(x), C.byref(s)))
        L = n.value
        return (np.ctypeslib.as_array(t, shape=(L,)).copy(), np.ctypeslib.as_array(x, shape=(len(q) * L * 7,)).reshape(len(q), L, 7).copy(),
                np.ctypeslib.as_array(s, shape=(len(q) * L,)).reshape(len(q), L).copy())

    # ------------------------------------------------------------------ map history (Navigator.WayMaps)
    def enable_map_history(self, entries, components):
        """The map log on the device (phd_map_history_enable): room for `entries` entries, one per SlamUpdate with a time from
        now on, and `components` components over all of them; entries = 0 switches it off. Every call restarts the log."""
        self._check(self._lib.phd_map_history_enable(self._h, int(entries), int(components)))
        self._map_history = int(entries) > 0
        self._map_history_len = 0

    def append_map_history(self, time=None):
        """One entry of the log: the best particle's map, slot and pose (phd_map_history_append; asynchronous).
        time=None: the entry's index."""
        if time is None:
            time = float(self.map_history_length)
        self._check(self._lib.phd_map_history_append(self._h, float(time)))
        self._map_history_len += 1

    @property
    def map_history_length(self):
        return self._map_history_len if self._map_history else 0

    def WayMaps(self, allow_missing=False):
        """≙ Navigator.WayMaps (Navigator.cs:269-272) with the best particle beside every map: a list of
        (time, best, pose[7], (w, mean, cov)), oldest entry first (phd_map_history; waits for the device). An entry whose
        components did not fit the log raises PHDError (status 2); allow_missing=True returns the list with None as its map."""
        n = C.c_int(0)
        t, b, x, cnt, off, w, m, c = dp(), ip(), dp(), ip(), i64p(), dp(), dp(), dp()
        rc = self._lib.phd_map_history(self._h, C.byref(n), C.byref(t), C.byref(b), C.byref(x), C.byref(cnt), C.byref(off), C.byref(w), C.byref(m), C.byref(c))
        if rc != 0 and not (allow_missing and rc == PHD_ERR_CAPACITY and n.value > 0):
            self._check(rc)
        out = []
        for k in range(n.value):
            lo, k_n = off[k], cnt[k]
            if k_n < 0:
                model = None
            elif k_n == 0:
                model = (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3)))
            else:
                model = (np.ctypeslib.as_array(w, shape=(lo + k_n,))[lo:].copy(), np.ctypeslib.as_array(m, shape=((lo + k_n) * 3,))[lo * 3:].reshape(k_n, 3).copy(),
                         np.ctypeslib.as_array(c, shape=((lo + k_n) * 9,))[lo * 9:].reshape(k_n, 3, 3).copy())
            out.append((t[k], b[k], np.array(x[k * 7:k * 7 + 7]), model))
        return out

    def MapError(self, truth, cutoff=1.0, order=1.0, align=None, allow_missing=False):
        """≙ Plot.MapError (postanalysis/Plot.cs:478-529) over the map log, on the device (phd_map_error; waits for it): a list of
        (time, ospa, cardinality, spatial, size), oldest entry first, of the OSPA distance with cut-off `cutoff` and order `order`
        between `truth` (the visited map, [n][3]) and Map.BestMapEstimate of every logged map; size is the estimate's.
        align: None, or per entry (estimated pose[7], true pose[7]) at the reference time — an entry whose pair is None is not
        aligned (the estimate is shorter than the reference time, :500). An entry without records or with an estimate beyond
        PHD_MAP_ERROR_MAX raises PHDError (status 2); allow_missing=True returns the list with NaN values for it."""
        truth = np.ascontiguousarray(truth, np.float64).reshape(-1, 3)
        poses, has = None, None
        if align is not None:
            align = list(align)
            has = np.array([a is not None for a in align], np.uint8)
            poses = np.ascontiguousarray([np.concatenate([np.asarray(a[0], float), np.asarray(a[1], float)]) if a is not None else
                                          np.tile([0.0, 0, 0, 1, 0, 0, 0], 2) for a in align], np.float64).reshape(-1, 14)
            if len(poses) != self.map_history_length:
                raise ValueError("one (estimated, true) pose pair per entry of the map log")
        n = C.c_int(0)
        t, o, c, s, z = dp(), dp(), dp(), dp(), ip()
        rc = self._lib.phd_map_error(self._h, _ptr(truth) if len(truth) else None, len(truth), float(cutoff), float(order),
                                     _ptr(poses) if poses is not None and len(poses) else None,
                                     has.ctypes.data_as(_lib.u8p) if has is not None and len(has) else None,
                                     C.byref(n), C.byref(t), C.byref(o), C.byref(c), C.byref(s), C.byref(z))
        if rc != 0 and not (allow_missing and rc == PHD_ERR_CAPACITY and n.value > 0):
            self._check(rc)
        return [(t[k], o[k], c[k], s[k], z[k]) for k in range(n.value)]

    POSE_ERROR_MODES = {"timed": 0, "smooth": 1, "filter": 2}   # PHD_POSE_ERROR_* (HistMode, postanalysis/Program.cs:68)

    def PoseError(self, truth, mode="timed", slots=None, first_entry=0, ref_entry=0, slam_time=0.0):
        """≙ Plot.LocationError / RotationError / OdoLocationError / OdoRotationError (postanalysis/Plot.cs:293-456) over the
        trajectory log, on the device (phd_pose_error; waits for it): (times, location, rotation, odo_times, odo_location,
        odo_rotation). truth: [L][7], the true pose at every entry of the log. mode: "timed" (per estimate the mean error of its
        whole path, from the `slam_time` index on), "smooth" (the newest estimate's path, per entry) or "filter" (every
        estimate's newest pose). slots: per entry the slot whose path is the estimate then; None: the best particle of the map
        log (the rule of WayPointsAt). The estimates are the entries from first_entry on; ref_entry is the entry both paths are
        taken relative to (Plot.RefTime). monorfs_amd/host/PoseError.hpp is the same metric on the host."""
        if mode not in self.POSE_ERROR_MODES:
            raise ValueError("mode is 'timed', 'smooth' or 'filter'")
        truth = np.ascontiguousarray(truth, np.float64).reshape(-1, 7)
        q = None
        if slots is not None:
            q = np.ascontiguousarray(list(slots) if not isinstance(slots, np.ndarray) else slots, np.int32).reshape(-1)
            if len(q) != len(truth):
                raise ValueError("one slot per true pose (one per entry of the trajectory log)")
        n, m = C.c_int(0), C.c_int(0)
        t, a, r, ot, oa, orot = dp(), dp(), dp(), dp(), dp(), dp()
        self._check(self._lib.phd_pose_error(self._h, self.POSE_ERROR_MODES[mode], _ptr(truth) if len(truth) else None, len(truth),
                                             q.ctypes.data_as(ip) if q is not None and len(q) else None, int(first_entry), int(ref_entry), float(slam_time),
                                             C.byref(n), C.byref(t), C.byref(a), C.byref(r), C.byref(m), C.byref(ot), C.byref(oa), C.byref(orot)))

        def arr(p, k):
            return np.ctypeslib.as_array(p, shape=(k,)).copy() if k else np.zeros(0)
        return (arr(t, n.value), arr(a, n.value), arr(r, n.value), arr(ot, m.value), arr(oa, m.value), arr(orot, m.value))

    def QuasiSetLogLikelihood(self, measurements, landmarks, poses):
        """≙ static PHDNavigator.QuasiSetLogLikelihood(measurements, map, pose) (PHDNavigator.cs:526-531), batched over
        candidate poses (phd_quasi_set_loglik): returns one value per pose."""
        z = np.ascontiguousarray(measurements, np.float64).reshape(-1, 3)
        lm = np.ascontiguousarray(landmarks, np.float64).reshape(-1, 3)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        out = np.zeros(len(poses))
        self._check(self._lib.phd_quasi_set_loglik(self._h, _ptr(poses), len(poses), _ptr(lm) if len(lm) else None, len(lm),
                                                   _ptr(z) if len(z) else None, len(z), _ptr(out)))
        return out

    def QuasiSetLogLikelihoodGradient(self, measurements, landmarks, poses, average_mode=0):
        """≙ static PHDNavigator.QuasiSetLogLikelihood(measurements, map, pose, out gradient) (PHDNavigator.cs:543-548),
        batched over candidate poses (phd_quasi_set_loglik_grad): returns (values[n], gradients[n][6]).
        average_mode: TemperedAverage as its source reads (0) or with weights that sum to one (1), see include/phdhip.h."""
        z = np.ascontiguousarray(measurements, np.float64).reshape(-1, 3)
        lm = np.ascontiguousarray(landmarks, np.float64).reshape(-1, 3)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        out, grad = np.zeros(len(poses)), np.zeros((len(poses), 6))
        self._check(self._lib.phd_quasi_set_loglik_grad(self._h, _ptr(poses), len(poses), _ptr(lm) if len(lm) else None, len(lm),
                                                        _ptr(z) if len(z) else None, len(z), int(average_mode), _ptr(out), _ptr(grad)))
        return out, grad

    ASCENT_LINE = 16   # PHD_ASCENT_LINE: a call serves max_particles // 16 estimates

    def QuasiAscent(self, initial, measurements, landmarks, linearpoint, average_mode=0, max_iterations=1000, round_iterations=0,
                    hessians=False):
        """≙ LoopyPHDNavigator.LogLikeGradientAscent (LoopyPHDNavigator.cs:916-965) for the initial estimates [n][6] side by
        side, resident on the device (phd_quasi_ascent): returns (poses[n][6], values[n], iterations[n], capped) and, with
        hessians=True, the raw finite-difference Hessian rows [n][6][6] of LogLikeFitCovariance at the returned poses behind
        them. More than max_particles // 16 estimates go as several calls. capped: some estimate was still climbing after
        max_iterations iterations (PHD_ERR_CAPACITY; its state at the bound is what is returned).
        round_iterations: iterations enqueued between two looks at the active count, 0 the library's default."""
        z = np.ascontiguousarray(measurements, np.float64).reshape(-1, 3)
        lm = np.ascontiguousarray(landmarks, np.float64).reshape(-1, 3)
        lin = np.ascontiguousarray(linearpoint, np.float64).reshape(7)
        initial = np.ascontiguousarray(initial, np.float64).reshape(-1, 6)
        n = len(initial)
        poses, values, iters = np.zeros((n, 6)), np.zeros(n), np.zeros(n, np.int32)
        hess = np.zeros((n, 6, 6)) if hessians else None
        chunk = max(1, self.params.max_particles // self.ASCENT_LINE)
        capped = False
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            rc = self._lib.phd_quasi_ascent(self._h, _ptr(initial[s:e]), e - s, _ptr(lin), _ptr(lm) if len(lm) else None, len(lm),
                                            _ptr(z) if len(z) else None, len(z), int(average_mode), int(max_iterations), int(round_iterations),
                                            _ptr(poses[s:e]), _ptr(values[s:e]), iters[s:e].ctypes.data_as(ip),
                                            _ptr(hess[s:e]) if hessians else None)
            if rc == PHD_ERR_CAPACITY:
                capped = True
            else:
                self._check(rc)
        return (poses, values, iters, capped, hess) if hessians else (poses, values, iters, capped)

    # ------------------------------------------------------------------ many problems in one call (phd_ascent_multi.h)
    @staticmethod
    def _block_class(m):
        """the measurement-block class of a problem with m measurements (0 fits any class: None)"""
        return None if m == 0 else (1 if m <= 64 else (2 if m <= 128 else 4))

    @staticmethod
    def _problem_table(problems):
        """[(landmarks, measurements[, linearpoint]), ...] as contiguous arrays"""
        lms = [np.ascontiguousarray(p[0], np.float64).reshape(-1, 3) for p in problems]
        zs = [np.ascontiguousarray(p[1], np.float64).reshape(-1, 3) for p in problems]
        lins = [np.ascontiguousarray(p[2], np.float64).reshape(7) if len(p) > 2 else None for p in problems]
        return lms, zs, lins

    def _multi_calls(self, zs, problem, per_call):
        """The C calls that serve the items (estimates or poses) `problem`[n]: lists of item indices, each of one block class and at
        most per_call long, in the caller's order within a call. The items of problems without measurements ride with the first
        class that has any."""
        classes = [self._block_class(len(z)) for z in zs]
        present = sorted({c for c in (classes[q] for q in problem) if c is not None}) or [1]
        groups = {c: [] for c in present}
        for i, q in enumerate(problem):
            groups[classes[q] if classes[q] is not None else present[0]].append(i)
        calls = []
        for c in present:
            calls += [groups[c][s:s + per_call] for s in range(0, len(groups[c]), per_call)]
        return calls

    @staticmethod
    def _pack_problems(lms, zs, lins, used):
        """offsets, pools and linearisation poses of the problems `used` (in that order), and the map old index -> new"""
        lmoff = np.zeros(len(used) + 1, np.int32)
        zoff = np.zeros(len(used) + 1, np.int32)
        for k, q in enumerate(used):
            lmoff[k + 1] = lmoff[k] + len(lms[q])
            zoff[k + 1] = zoff[k] + len(zs[q])
        lm = np.ascontiguousarray(np.concatenate([lms[q] for q in used] + [np.zeros((0, 3))]))
        z = np.ascontiguousarray(np.concatenate([zs[q] for q in used] + [np.zeros((0, 3))]))
        lin = np.ascontiguousarray([lins[q] for q in used]) if lins is not None else None
        return lmoff, lm, zoff, z, lin, {q: k for k, q in enumerate(used)}

    def QuasiAscentMulti(self, problems, initial, problem, average_mode=0, max_iterations=1000, round_iterations=0, hessians=False):
        """QuasiAscent for the estimates of many problems in the same launches (phd_quasi_ascent_multi): problems is a list of
        (landmarks, measurements, linearpoint), estimate e starts at initial[e] and is searched against problems[problem[e]].
        Returns what QuasiAscent returns, every estimate bit for bit as from QuasiAscent with its problem alone. A C call takes
        problems of one measurement-block class (<= 64, 65..128, 129..256 measurements) and max_particles // 16 estimates: the
        estimates are split by class and chunked, each call is handed only the problems its estimates name, and the results
        come back in the caller's order."""
        lms, zs, lins = self._problem_table(problems)
        initial = np.ascontiguousarray(initial, np.float64).reshape(-1, 6)
        problem = [int(q) for q in np.asarray(problem).reshape(-1)]
        n = len(initial)
        if len(problem) != n or any(q < 0 or q >= len(problems) for q in problem):
            raise ValueError("one problem index in [0, len(problems)) per estimate")
        poses, values, iters = np.zeros((n, 6)), np.zeros(n), np.zeros(n, np.int32)
        hess = np.zeros((n, 6, 6)) if hessians else None
        capped = False
        for idx in self._multi_calls(zs, problem, max(1, self.params.max_particles // self.ASCENT_LINE)):
            used = sorted({problem[i] for i in idx})
            lmoff, lm, zoff, z, lin, renum = self._pack_problems(lms, zs, lins, used)
            k = len(idx)
            start = np.ascontiguousarray(initial[idx])
            which = np.array([renum[problem[i]] for i in idx], np.int32)
            p, v, it = np.zeros((k, 6)), np.zeros(k), np.zeros(k, np.int32)
            h = np.zeros((k, 6, 6)) if hessians else None
            rc = self._lib.phd_quasi_ascent_multi(self._h, len(used), lmoff.ctypes.data_as(ip), _ptr(lm) if len(lm) else None,
                                                  zoff.ctypes.data_as(ip), _ptr(z) if len(z) else None, _ptr(lin), _ptr(start),
                                                  which.ctypes.data_as(ip), k, int(average_mode), int(max_iterations), int(round_iterations),
                                                  _ptr(p), _ptr(v), it.ctypes.data_as(ip), _ptr(h) if hessians else None)
            if rc == PHD_ERR_CAPACITY:
                capped = True
            else:
                self._check(rc)
            poses[idx], values[idx], iters[idx] = p, v, it
            if hessians:
                hess[idx] = h
        return (poses, values, iters, capped, hess) if hessians else (poses, values, iters, capped)

    def _quasi_batch_multi(self, problems, poses, problem, average_mode, gradient):
        lms, zs, _ = self._problem_table(problems)
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        problem = [int(q) for q in np.asarray(problem).reshape(-1)]
        n = len(poses)
        if len(problem) != n or any(q < 0 or q >= len(problems) for q in problem):
            raise ValueError("one problem index in [0, len(problems)) per pose")
        out, grad = np.zeros(n), (np.zeros((n, 6)) if gradient else None)
        for idx in self._multi_calls(zs, problem, max(1, self.params.max_particles)):
            used = sorted({problem[i] for i in idx})
            lmoff, lm, zoff, z, _, renum = self._pack_problems(lms, zs, None, used)
            k = len(idx)
            at = np.ascontiguousarray(poses[idx])
            which = np.array([renum[problem[i]] for i in idx], np.int32)
            o, g = np.zeros(k), (np.zeros((k, 6)) if gradient else None)
            self._check(self._lib.phd_quasi_set_loglik_multi(self._h, len(used), lmoff.ctypes.data_as(ip), _ptr(lm) if len(lm) else None,
                                                             zoff.ctypes.data_as(ip), _ptr(z) if len(z) else None, _ptr(at),
                                                             which.ctypes.data_as(ip), k, int(average_mode), _ptr(o), _ptr(g) if gradient else None))
            out[idx] = o
            if gradient:
                grad[idx] = g
        return (out, grad) if gradient else out

    def QuasiSetLogLikelihoodMulti(self, problems, poses, problem):
        """QuasiSetLogLikelihood for poses of many problems in one launch (phd_quasi_set_loglik_multi): problems is a list of
        (landmarks, measurements[, linearpoint]), pose i is evaluated against problems[problem[i]]. One value per pose, bit for
        bit QuasiSetLogLikelihood's with that problem alone; split by block class and chunked by max_particles."""
        return self._quasi_batch_multi(problems, poses, problem, 0, False)

    def QuasiSetLogLikelihoodGradientMulti(self, problems, poses, problem, average_mode=0):
        """QuasiSetLogLikelihoodGradient for poses of many problems in one launch: (values[n], gradients[n][6])."""
        return self._quasi_batch_multi(problems, poses, problem, average_mode, True)

    def QuasiGuessesMulti(self, problems, pose0s, radius=0.5):
        """The starting guesses of GuidedFitMixture (LoopyPHDNavigator.cs:789-797) for many problems and their first values
        (phd_quasi_guesses_multi): problems is a list of (landmarks, measurements, linearpoint), problem q starts at the linear
        pose pose0s[q]. Returns (offsets[len(problems) + 1], pairs[n][2], guesses6[n][6], poses7[n][7], values[n],
        emptyspace[len(problems)]): the guesses of problem q stand at offsets[q] .. offsets[q + 1], pose0s[q] first (pair -1, -1),
        then the (landmark, measurement) pairs within `radius` of the initial pose in landmark-major order; poses7 =
        Add(linearpoint, guess), values = QuasiSetLogLikelihood there, emptyspace[q] = the value of the pose far from everything.
        A C call takes problems of one measurement-block class: the problems are split by class, a call that reports more
        guesses than its arrays hold is repeated once with the reported total, and the results come back in the caller's order."""
        lms, zs, lins = self._problem_table(problems)
        pose0s = np.ascontiguousarray(pose0s, np.float64).reshape(-1, 6)
        T = len(problems)
        if len(pose0s) != T or any(lin is None for lin in lins):
            raise ValueError("one initial pose and one linearisation pose per problem")
        far7 = pose3d_add(np.array([0, 0, 0, 1.0, 0, 0, 0]), np.full(6, 1e5))   # the pose far from everything (:808)
        per = [None] * T
        empty = np.zeros(T)
        for used in self._multi_calls(zs, list(range(T)), max(T, 1)):
            lmoff, lm, zoff, z, lin, _ = self._pack_problems(lms, zs, lins, used)
            start = np.ascontiguousarray(pose0s[used])
            k = len(used)
            goff, e = np.zeros(k + 1, np.int32), np.zeros(k)
            capacity = k + min(sum(len(lms[q]) * len(zs[q]) for q in used), 64 * k)   # (every pair, or a first try of 64 a problem)
            for attempt in (0, 1):
                pairs, g6, p7, v = np.zeros((capacity, 2), np.int32), np.zeros((capacity, 6)), np.zeros((capacity, 7)), np.zeros(capacity)
                rc = self._lib.phd_quasi_guesses_multi(self._h, k, lmoff.ctypes.data_as(ip), _ptr(lm) if len(lm) else None,
                                                       zoff.ctypes.data_as(ip), _ptr(z) if len(z) else None, _ptr(lin), _ptr(start), _ptr(far7),
                                                       float(radius), capacity, goff.ctypes.data_as(ip), pairs.ctypes.data_as(ip),
                                                       _ptr(g6), _ptr(p7), _ptr(v), _ptr(e))
                if rc != PHD_ERR_CAPACITY or attempt:
                    break
                capacity = int(goff[k])   # (guess_offsets is set: the total the retry needs)
            self._check(rc)
            for j, q in enumerate(used):
                per[q] = slice(int(goff[j]), int(goff[j + 1])), pairs, g6, p7, v
                empty[q] = e[j]
        offsets = np.zeros(T + 1, np.int32)
        for q in range(T):
            offsets[q + 1] = offsets[q] + (per[q][0].stop - per[q][0].start)
        cat = lambda i, tail, dtype: (np.concatenate([per[q][i][per[q][0]] for q in range(T)]) if T else np.zeros((0,) + tail, dtype))
        return offsets, cat(1, (2,), np.int32), cat(2, (6,), np.float64), cat(3, (7,), np.float64), cat(4, (), np.float64), empty

    def LogLikeGradient(self, pose, measurements, landmarks, linearpoint):
        """≙ LoopyPHDNavigator.LogLikeGradient (LoopyPHDNavigator.cs:876-909): central differences (eps = 1e-5) of the
        quasi set log-likelihood at linearpoint.Add(pose +- eps e_i) — the 12 evaluations go to the device as one batch.
        `pose` may hold several linear poses [n][6]: the 12 n evaluations are still one batch."""
        pose = np.ascontiguousarray(pose, np.float64).reshape(-1, 6)
        eps = 1e-5
        cand = np.empty((len(pose), 6, 2, 7))
        for a in range(len(pose)):
            for i in range(6):
                for s, sign in enumerate((1.0, -1.0)):
                    d = pose[a].copy()
                    d[i] += sign * eps
                    cand[a, i, s] = pose3d_add(linearpoint, d)
        ll = self.QuasiSetLogLikelihood(measurements, landmarks, cand.reshape(-1, 7)).reshape(len(pose), 6, 2)
        g = (ll[:, :, 0] - ll[:, :, 1]) / (2 * eps)
        return g[0] if len(g) == 1 else g

    def set_depth_map(self, depth):
        """The current Kinect depth frame (phd_set_depth_map): a (height, width) array, row-major depth[y][x] — the reference's
        float[ResX][ResY] frame transposed —, taken as float32; NaN means no reading. Every step after this call uses it until
        the next; None switches it off (the PRM3D detection probability again)."""
        if depth is None:
            self._check(self._lib.phd_set_depth_map(self._h, None, 0, 0))
            return
        d = np.ascontiguousarray(depth, np.float32)
        if d.ndim != 2:
            raise ValueError("the depth map is a (height, width) array")
        self._check(self._lib.phd_set_depth_map(self._h, d.ctypes.data_as(C.POINTER(C.c_float)), int(d.shape[1]), int(d.shape[0])))

    def DetectionProbabilityM(self, z):
        """≙ SimulatedVehicle.DetectionProbabilityM (SimulatedVehicle.cs:336) at pixel-range points z[n][3], evaluated by the
        device function the step uses, with the handle's parameters and current depth map (phd_test_detection_probability)."""
        z = np.ascontiguousarray(z, np.float64).reshape(-1, 3)
        out = np.zeros(len(z))
        if len(z):
            self._check(self._lib.phd_test_detection_probability(self._h, _ptr(z), len(z), _ptr(out)))
        return out

    def SlamUpdate(self, time, measurements, u_resample=0.5):
        """≙ PHDNavigator.SlamUpdate (:323-362). With the map log on and a time given, the step's best map is appended behind it
        (UpdateMapHistory, :361)."""
        z = np.ascontiguousarray(measurements, np.float64).reshape(-1, 3)
        self._check(self._lib.phd_slam_update(self._h, _ptr(z), len(z), int(self.OnlyMapping), float(u_resample)))
        if self._map_history and time is not None:
            self.append_map_history(time)

    @property
    def VehicleWeights(self):
        n = C.c_int32(0)
        ptr = self._lib.phd_weights(self._h, C.byref(n))
        if not ptr:
            raise PHDError(-1, self._lib.phd_last_error(self._h).decode())
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).copy()

    @property
    def BestParticle(self):
        return self._lib.phd_best_particle(self._h)

    def _map_from(self, fn, *args):
        n = C.c_int32(0)
        w, m, c = dp(), dp(), dp()
        self._check(fn(self._h, *args, C.byref(n), C.byref(w), C.byref(m), C.byref(c)))
        k = n.value
        if k == 0:
            return np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3))
        return (np.ctypeslib.as_array(w, shape=(k,)).copy(), np.ctypeslib.as_array(m, shape=(k * 3,)).reshape(k, 3).copy(),
                np.ctypeslib.as_array(c, shape=(k * 9,)).reshape(k, 3, 3).copy())

    def MapModel(self, particle):
        """≙ MapModels[particle] (:134)."""
        return self._map_from(self._lib.phd_map, int(particle))

    @property
    def BestMapModel(self):
        """≙ :155-161."""
        return self.MapModel(self.BestParticle)

    @property
    def BestEstimate(self):
        """≙ :144-150 — the pose of the best particle."""
        return self.poses()[self.BestParticle]

    def resample_sources(self):
        n = C.c_int32(0)
        r = C.c_uint8(0)
        ptr = self._lib.phd_resample_sources(self._h, C.byref(n), C.byref(r))
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).copy(), bool(r.value)

    def ResampleParticles(self, weights, u):
        """≙ :724-760 on caller-supplied weights; returns (sources, best slot)."""
        weights = np.ascontiguousarray(weights, np.float64)
        src = np.zeros(len(weights), np.int32)
        best = C.c_int32(0)
        self._check(self._lib.phd_resample(self._h, _ptr(weights), len(weights), float(u), src.ctypes.data_as(ip), C.byref(best)))
        return src, best.value

    def ParticleDepleted(self, weights):
        """≙ :768-777."""
        weights = np.ascontiguousarray(weights, np.float64)
        d = C.c_uint8(0)
        self._check(self._lib.phd_particle_depleted(self._h, _ptr(weights), len(weights), C.byref(d)))
        return bool(d.value)

    # ------------------------------------------------------------------ stage-level (unit KAT surface)
    def run_stages(self, measurements, with_alpha=True):
        z = np.ascontiguousarray(measurements, np.float64).reshape(-1, 3)
        self._check(self._lib.phd_stage_run(self._h, _ptr(z), len(z), int(with_alpha)))

    def PredictConditional(self, particle=0):
        return self._map_from(self._lib.phd_stage_map, PHD_STAGE_PREDICTED, int(particle))

    def CorrectConditional(self, particle=0):
        """Corrected components with weight >= MinWeight (the rest cannot survive PruneModel), unsorted."""
        return self._map_from(self._lib.phd_stage_map, PHD_STAGE_CORRECTED, int(particle))

    def PruneModel(self, particle=0):
        return self._map_from(self._lib.phd_stage_map, PHD_STAGE_PRUNED, int(particle))

    def WeightAlpha(self):
        n = C.c_int32(0)
        ptr = self._lib.phd_stage_alpha(self._h, C.byref(n))
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).copy()

    def SetLogLikelihood(self):
        n = C.c_int32(0)
        ptr = self._lib.phd_stage_setloglik(self._h, C.byref(n))
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).copy()

    def test_pairing(self, matrix, lexicographic=False, modelsize=0, maxcount=200):
        """the device's MurtyPairing (best first) or LexicographicalPairing(matrix, modelsize) on a dense profit matrix:
        (assignments [k][n], values [k]) — phd_test_pairing, the surface GraphCombinatoricsTest's vectors go through"""
        m = np.ascontiguousarray(matrix, np.float64)
        n = m.shape[0]
        asg = np.zeros((maxcount, n), np.int32)
        val = np.zeros(maxcount)
        cnt = C.c_int(0)
        self._check(self._lib.phd_test_pairing(self._h, _ptr(m), n, 1 if lexicographic else 0, int(modelsize), maxcount,
                                               asg.ctypes.data_as(ip), _ptr(val), C.byref(cnt)))
        k = min(cnt.value, maxcount)
        return asg[:k].tolist(), val[:k].copy()

    def test_primitive(self, op, in_array, out_dtype, out_count):
        """one device arithmetic primitive on raw records (phd_test_primitive; ops and record layouts:
        monorfs_amd/csrc/phd_primitives_test.h): the bytes of `in_array` in, `out_count` items of `out_dtype` back"""
        a = np.ascontiguousarray(in_array)
        out = np.zeros(int(out_count), out_dtype)
        self._check(self._lib.phd_test_primitive(self._h, int(op), a.ctypes.data_as(C.c_void_p) if a.nbytes else None, a.nbytes,
                                                 out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    # ------------------------------------------------------------------ benchmark surface
    def set_measurements(self, measurements):
        z = np.ascontiguousarray(measurements, np.float64).reshape(-1, 3)
        self._check(self._lib.phd_set_measurements(self._h, _ptr(z), len(z)))

    def step_async(self, u_resample=0.5):
        self._check(self._lib.phd_step_async(self._h, int(self.OnlyMapping), float(u_resample)))

    def StepHold(self, held):
        """One mapping-only step that particle slot `held` sits out: behind it the slot has the mixture it had in front of it,
        bit for bit; -1 holds nobody (phd_step_hold_async). Posts the step and returns: nothing waits for the device."""
        self._check(self._lib.phd_step_hold_async(self._h, int(held)))

    def sync(self):
        self._check(self._lib.phd_sync(self._h))

    def set_frozen(self, frozen):
        self._check(self._lib.phd_set_frozen(self._h, int(bool(frozen))))

    def set_all_pairs(self, on):
        """SURVEY 8d's benchmark mode: every (component, measurement) pair evaluated, the gate only masks (phd_set_all_pairs)"""
        self._check(self._lib.phd_set_all_pairs(self._h, int(bool(on))))

    def set_split(self, nsplit):
        """Launch a step's per-particle kernels as `nsplit` sub-ranges on concurrent streams (phd_set_split)."""
        self._check(self._lib.phd_set_split(self._h, int(nsplit)))

    def timing_reset(self, enabled=True):
        """enabled: False / 0 off, True / 1 every step, n > 1 every n-th step"""
        self._check(self._lib.phd_timing_reset(self._h, int(enabled)))

    def last_timings(self):
        names = C.POINTER(C.c_char_p)()
        ms = dp()
        n = self._lib.phd_last_timings(self._h, C.byref(names), C.byref(ms))
        return {names[i].decode(): ms[i] for i in range(n)}

    def multi_report(self):
        """diagnostics of a multi-device handle (phd_multi_report): per-phase device time of the sampled steps on the first
        shard's stream, the host's cost of posting / issuing a step, and which shard pairs exchange by direct peer access"""
        out = np.zeros(9)
        p2p = np.zeros(64 * 64, np.uint8)
        n = C.c_int32(0)
        self._check(self._lib.phd_multi_report(self._h, _ptr(out), p2p.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(n)))
        k = n.value
        names = ("local", "gather_wait", "global_and_plan", "pack", "exchange_wait_and_unpack")
        return {"phase_ms": {nm: float(out[i]) for i, nm in enumerate(names)}, "post_us": float(out[5]), "issue_us": float(out[6]), "issue_calls_us": float(out[8]),
                "sampled_steps": int(out[7]), "shards": k, "p2p": p2p[:k * k].reshape(k, k).astype(bool).tolist()}

    def test_migration_plan(self, gsrc, particles_per_rank, world, rank, resampled=True):
        """the migration plan as the device makes it inside a sharded step (phd_test_migration_plan): dict of the lists"""
        g = np.ascontiguousarray(gsrc, np.int32)
        Pl, n = int(particles_per_rank), int(world)
        sc, rc = np.zeros(n, np.int32), np.zeros(n, np.int32)
        sl, code, fs = np.zeros(Pl + 64, np.int32), np.zeros(Pl, np.int32), np.zeros(Pl, np.int32)
        sd = np.zeros((Pl + 64, 2), np.int32)
        ns, nr, st = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        q = lambda a: a.ctypes.data_as(ip)
        self._check(self._lib.phd_test_migration_plan(self._h, q(g), Pl, n, int(rank), int(bool(resampled)), q(sc), q(rc), q(sl), q(code), q(fs), q(sd),
                                                      C.byref(ns), C.byref(nr), C.byref(st)))
        return {"send_counts": sc, "recv_counts": rc, "send_list": sl[:ns.value].copy(), "dst_code": code, "fslot": fs[:nr.value].copy(),
                "send_dst": sd[:ns.value].copy(), "nsend": ns.value, "nrecv": nr.value, "status": st.value}

    def last_timing_counts(self):
        """launches behind each mean of the last last_timings() call (a split step launches each kernel per sub-range)"""
        names = C.POINTER(C.c_char_p)()
        ms = dp()
        n = self._lib.phd_last_timings(self._h, C.byref(names), C.byref(ms))
        cnt = C.POINTER(C.c_int)()
        self._lib.phd_last_timing_counts(self._h, C.byref(cnt))
        return {names[i].decode(): cnt[i] for i in range(n)}
