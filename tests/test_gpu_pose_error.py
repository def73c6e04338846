"""phd_pose_error on the device: the pose-error series of the post-analysis (Plot.LocationError, RotationError, OdoLocationError,
OdoRotationError in the history modes Timed, Smooth and Filter) over the trajectory log, at the kernel's shape edges, through
real steps that resample, for its determinism, at its refusals, and through scripts/replay.py --posted --pose-error.

Expected values never come from the new kernel: the paths are those of WayPointsAt(i, [s_i]) (phd_trajectories_at), fed to the
numpy statement of tests/pose_error_ref.py; monorfs_amd/host/PoseError.hpp (through tests/pose_error_host.cpp) runs on the same
inputs beside it.

Tolerances. Location and odometry location: abs <= 1e-12 * S * max(1, L / 256) with S = 1 + max |coordinate| — a mean of at
most L norms of differences of coordinates of size S, each good to a few ulp of S, and a re-ordered sum of L non-negative terms
good to L * 2^-53 relative. Rotation: the two acos calls magnify rounding by 1 / sin(angle / 2), at most 4e3 ulp with every
rotation error that is not identically 0 (an entry against itself) at or above 1e-3, which every test asserts of its inputs.
The bound is not fixed in advance: the largest difference between PoseError.hpp and pose_error_ref.py on the very inputs of a
test is measured (two libms, two evaluation orders, both on the CPU) and printed, the device is allowed 16 times that, at least
1e-13, and the test asserts that this allowance stays under 1e-9. Measured on the inputs below (profiles/pose_error_cost.md has
the run): at most 3.2e-13 between the two CPU statements, so an allowance of at most 5.2e-12; the device differed from
pose_error_ref.py by at most 1.2e-12. The -0 and NaN of the Timed division are compared by kind.

PHD_ERR_CAPACITY for a log beyond PHD_POSE_ERROR_MAX entries is tested at one particle (test_capacity_refusal, which prints what
its PHD_POSE_ERROR_MAX + 1 appends took). The other PHD_ERR_CAPACITY, for a handle of more than 65 536 particles, is not covered:
no test of this suite runs a handle beyond a few hundred particles, and one of 65 537 would be the first run of every reset,
upload and append kernel at that size, a test of those kernels and not of the one comparison that refuses."""
import ctypes as C
import functools
import os
import re
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import history_seq as hs
import pose_error_ref as ref
from monorfs_amd import _lib
from monorfs_amd import recordio as rio
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, PHD_ERR_CAPACITY, prm3d_defaults
from pose_error_tools import MODES, build_host, host_series, same_kind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# below, at and behind the odometry series' ten, a wave's 64 entries (one and two chunks of the trace), a workgroup's 256 threads
LENGTHS = (1, 2, 10, 11, 12, 63, 64, 65, 66, 129, 257)
NAMES = ("location", "rotation", "odolocation", "odorotation")


@pytest.fixture(scope="module")
def nav_mod():
    from monorfs_amd import navigator
    return navigator


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return build_host(str(tmp_path_factory.mktemp("pose_error_host")))


def make_nav(nav_mod, particles, capacity, **over):
    p = hs.params_of((particles, 1, 0.1, None), **over)
    nav = nav_mod.PHDNavigator(p, particlecount=particles)
    nav.enable_history(capacity)
    return nav


def quats(rng, angle):
    v = rng.normal(size=(len(angle), 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return np.concatenate([np.cos(angle / 2)[:, None], np.sin(angle / 2)[:, None] * v], axis=1)


def qmul(a, b):
    return np.stack([a[:, 0] * b[:, 0] - (a[:, 1:] * b[:, 1:]).sum(1),
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2],
                     a[:, 0] * b[:, 2] + a[:, 2] * b[:, 0] + a[:, 3] * b[:, 1] - a[:, 1] * b[:, 3],
                     a[:, 0] * b[:, 3] + a[:, 3] * b[:, 0] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]], axis=1)


def noisy(rng, poses, noise=1e-2):
    """the same path plus noise of `noise` in position and `noise` rad in rotation"""
    n = len(poses)
    return np.concatenate([poses[:, :3] + noise * rng.normal(size=(n, 3)), qmul(poses[:, 3:], quats(rng, noise * np.abs(rng.normal(size=n)) + noise))], axis=1)


@functools.lru_cache(maxsize=None)
def edge_inputs(L):
    """(particles, poses[L][P][7] of the entries, truth[L][7], slots[L]): every particle's poses random, with rotations of 0.05
    to 1 rad; a random slot per entry; the truth is the newest estimate's path (the slot of entry L - 1) plus noise of 1e-2"""
    rng = np.random.default_rng(700 + L)
    P = 3 + L % 6
    poses = np.stack([np.concatenate([rng.uniform(-2, 2, size=(L, 3)), quats(rng, rng.uniform(0.05, 1.0, L))], axis=1) for _ in range(P)], axis=1)
    slots = rng.integers(0, P, L).astype(np.int32)
    return P, poses, noisy(rng, poses[:, slots[L - 1]]), slots


def combos(L):
    """(mode index, first_entry, ref_entry, slam_time) with times k / 30: every mode, first_entry 0 and 1, ref_entry 0, 5, L - 1 and
    L + 3, slam_time before, inside and behind the record, all of them crossed (Smooth reads no first_entry and only Timed a
    slam_time). The expected values cost little more than one query's: pose_error_ref.py keeps every path's per-pose series."""
    firsts = sorted({0, min(1, L - 1)})
    refs = (0, 5, L - 1, L + 3)
    slams = (-1.0, (L // 2) / 30.0 + 1e-3, (L + 5) / 30.0)
    return [(0, f, r, s) for f in firsts for r in refs for s in slams] + [(1, 0, r, 0.0) for r in refs] + [(2, f, r, 0.0) for f in firsts for r in refs]


def expected(times, truth, paths, queries):
    """pose_error_ref.py per query, and every per-pose rotation error it met (for the precondition)"""
    memo, out = {}, []
    for m, first, refentry, slam in queries:
        trajectory, estimate = ref.histories(times, truth, paths, first)
        out.append(ref.all_series(MODES[m], trajectory, estimate, refentry, slam, memo))
    rotations = [v for (name, _, _), v in memo.items() if "rotation" in name]
    rotations += [s[i][1] for q, s in zip(queries, out) if q[0] != 0 for i in (1, 3)]
    return out, np.concatenate(rotations) if rotations else np.zeros(0)


def check(nav, times, truth, paths, slots, queries, host_exe, what, pass_slots=True):
    """the device against pose_error_ref.py on every query, with the rotation allowance measured on these inputs; returns it"""
    L = len(times)
    want, rotations = expected(times, truth, paths, queries)
    moving = rotations[rotations != 0]
    print("%s: %d per-pose rotation errors, the smallest that is not identically 0: %.3g" % (what, len(rotations), moving.min() if len(moving) else np.inf))
    assert np.all(rotations[~np.isnan(rotations)] >= 0) and (len(moving) == 0 or moving.min() >= 1e-3), "%s: a rotation error below 1e-3: the acos would decide the comparison" % what
    host = host_series(host_exe, times, truth, paths, queries)
    measured = 0.0
    for q, h, w in zip(queries, host, want):
        for i in (1, 3):
            ok = ~np.isnan(w[i][1])
            assert same_kind(h[i][1], w[i][1]), (what, q, NAMES[i])
            measured = max(measured, float(np.max(np.abs(h[i][1][ok] - w[i][1][ok]), initial=0.0)))
    allowed = max(16 * measured, 1e-13)
    print("%s: PoseError.hpp against pose_error_ref.py on these inputs: %.3g; the device is allowed %.3g" % (what, measured, allowed))
    assert allowed <= 1e-9, "%s: the two CPU statements differ by %g" % (what, measured)
    S = 1 + max(np.abs(np.asarray(truth)[:, :3]).max(), max(np.abs(np.asarray(p)[:, :3]).max() for p in paths))
    loctol = 1e-12 * S * max(1.0, L / 256.0)
    worst = [0.0, 0.0]
    for q, w in zip(queries, want):
        got = nav.PoseError(truth, mode=MODES[q[0]], slots=slots if pass_slots else None, first_entry=q[1], ref_entry=q[2], slam_time=q[3])
        series = ((got[0], got[1]), (got[0], got[2]), (got[3], got[4]), (got[3], got[5]))
        for i, ((gt, gv), (wt, wv)) in enumerate(zip(series, w)):
            assert np.array_equal(gt, wt), "%s %r: the times of %s" % (what, q, NAMES[i])
            assert same_kind(gv, wv), "%s %r: %s has NaN or -0 elsewhere: %r / %r" % (what, q, NAMES[i], gv, wv)
            ok = ~np.isnan(wv)
            d = float(np.max(np.abs(gv[ok] - wv[ok]), initial=0.0))
            worst[i % 2] = max(worst[i % 2], d)
            assert d <= (loctol if i % 2 == 0 else allowed), "%s %r: %s differs by %g (allowed %g)" % (what, q, NAMES[i], d, loctol if i % 2 == 0 else allowed)
    print("%s: device against pose_error_ref.py: location %.3g (allowed %.3g), rotation %.3g (allowed %.3g)" % (what, worst[0], loctol, worst[1], allowed))
    return allowed


# ---- 1. the shape edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_shape_edges(nav_mod, host_exe, L):
    """entries logged without steps (set_poses + append_history: identity ancestry), a random slot per entry: the paths of
    different estimates are different particles', no prefixes of one another"""
    P, poses, truth, slots = edge_inputs(L)
    nav = make_nav(nav_mod, P, L)
    times = np.arange(L) / 30.0
    for k in range(L):
        nav.set_poses(poses[k])
        nav.append_history(times[k])
    paths = [nav.WayPointsAt(i, [slots[i]])[1][0] for i in range(L)]
    assert all(np.array_equal(paths[i], poses[:i + 1, slots[i]]) for i in range(L))
    check(nav, times, truth, paths, slots, combos(L), host_exe, "L = %d" % L)
    nav.close()


def test_quirk_values_of_the_timed_division(nav_mod):
    """slam_time behind every entry: start_i = i, so the odometry series of estimate 1 is 0 / 0 = NaN and that of every later
    estimate 0 / a negative count = -0 (the reference prints both); the location mean is the newest pose's error alone"""
    L = 14
    P, poses, truth, slots = edge_inputs(63)
    poses, truth, slots = poses[:L], truth[:L], slots[:L]
    nav = make_nav(nav_mod, P, L)
    for k in range(L):
        nav.set_poses(poses[k])
        nav.append_history(k / 30.0)
    t, loc, rot, ot, oloc, orot = nav.PoseError(truth, mode="timed", slots=slots, slam_time=100.0)
    assert len(t) == L == len(ot) and np.array_equal(t, ot)
    for series in (oloc, orot):
        assert series[0] == 0.0 and not np.signbit(series[0]), "estimate 0: 0 / 1"
        assert np.isnan(series[1]), "estimate 1 is not the NaN of 0 / 0: %r" % series[1]
        assert np.all(series[2:] == 0.0) and np.all(np.signbit(series[2:])), "the later estimates are not the -0 of 0 / a negative count: %r" % series[2:]
    assert np.all(np.isfinite(loc)) and np.all(np.isfinite(rot)) and np.all(loc[1:] > 0)
    nav.close()


# ---- 2. ancestry: real steps that resample -------------------------------------------------------------------------------
ANCESTRY_CASE = hs.CASES[0]          # 5 particles
ANCESTRY_FRAMES = 150


def test_ancestry_through_real_steps(nav_mod, host_exe):
    """150 frames of the history sequence (its twelve frames over and over: the skewed weights resample), an entry per frame
    in both logs; the estimate at entry k is the best particle the previous frame left. slots = NULL must give the same bits as
    those slots handed over."""
    case, L = ANCESTRY_CASE, ANCESTRY_FRAMES
    f = hs.frame_of(case)
    nav = nav_mod.PHDNavigator(hs.params_of(case), particlecount=f.P)
    nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
    nav.enable_history(L)
    nav.enable_map_history(L, L * 600)
    resampled = []
    for k in range(L):
        _, noise, w, z, u = hs.inputs(case)[k % hs.FRAMES]
        nav.UpdateOdometry(k / 30.0, hs.READING, noise)          # (appends to the trajectory log)
        nav.set_weights(w)
        nav.SlamUpdate(k / 30.0, z, u_resample=u)                # (appends to the map log)
        resampled.append(bool(nav.resample_sources()[1]))
    best = [m[1] for m in nav.WayMaps()]
    slots = np.array([0] + best[:-1], np.int32)                  # the newest map entry appended before trajectory entry k
    at = [nav.WayPointsAt(i, [slots[i]]) for i in range(L)]
    times, paths = at[-1][0], [a[1][0] for a in at]
    # preconditions: resamplings on both sides of the trace's chunk edges, and paths that are no prefixes of the newest one
    # (entry k's ancestry word is set by the resampling of frame k - 1)
    dirty = [False] + resampled[:-1]
    for edge in (64, 128):
        assert any(dirty[edge - 8:edge]) and any(dirty[edge:edge + 8]), "no resampling on both sides of entry %d" % edge
    strangers = [i for i in range(L) if not np.array_equal(at[i][2][0], at[-1][2][0][:i + 1])]
    print("resampled frames: %d of %d; estimates whose path is no prefix of the newest: %d" % (sum(resampled), L, len(strangers)))
    assert len(strangers) >= 3, "Timed would equal Smooth's prefixes: the trace goes untested"
    rng = np.random.default_rng(77)
    truth = noisy(rng, paths[-1], noise=0.1)
    queries = [(0, 0, 0, -1.0), (0, 1, 5, 70.5 / 30.0), (0, 0, L + 3, 1000.0), (1, 0, 0, 0.0), (1, 0, 5, 0.0), (2, 0, 0, 0.0), (2, 1, 5, 0.0)]
    check(nav, times, truth, paths, slots, queries, host_exe, "ancestry")
    for m, first, refentry, slam in queries:
        a = nav.PoseError(truth, mode=MODES[m], slots=slots, first_entry=first, ref_entry=refentry, slam_time=slam)
        b = nav.PoseError(truth, mode=MODES[m], slots=None, first_entry=first, ref_entry=refentry, slam_time=slam)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "slots = NULL differs from the slots of WayMaps: %r" % ((m, first, refentry, slam),)
    nav.close()


# ---- 3. determinism ------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_call_and_at_another_stride(nav_mod):
    L = 129
    P, poses, truth, slots = edge_inputs(L)
    got = []
    for stride in (P, P + 59):
        nav = make_nav(nav_mod, P, L, max_particles=stride)
        for k in range(L):
            nav.set_poses(poses[k])
            nav.append_history(k / 30.0)
        for _ in range(2):
            got.append([nav.PoseError(truth, mode=m, slots=slots, first_entry=1, ref_entry=5, slam_time=1.0) for m in MODES])
        nav.close()
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
def raw(nav, mode, truth, slots, first=0, refentry=0, slam=0.0, ntruth=None):
    """the call through ctypes with marked outputs: (status, outputs untouched)"""
    truth = np.ascontiguousarray(truth, np.float64)
    mark = C.cast(0x1234560, _lib.dp)
    n, m = C.c_int(-7), C.c_int(-7)
    out = [C.cast(mark, _lib.dp) for _ in range(6)]
    q = None if slots is None else np.ascontiguousarray(slots, np.int32)
    rc = nav._lib.phd_pose_error(nav._h, mode, truth.ctypes.data_as(_lib.dp), len(truth) if ntruth is None else ntruth, None if q is None else q.ctypes.data_as(_lib.ip),
                                 first, refentry, slam, C.byref(n), C.byref(out[0]), C.byref(out[1]), C.byref(out[2]), C.byref(m), C.byref(out[3]), C.byref(out[4]), C.byref(out[5]))
    untouched = n.value == -7 and m.value == -7 and all(C.cast(o, C.c_void_p).value == 0x1234560 for o in out)
    return rc, untouched


def test_refusals(nav_mod):
    L = 6
    P, poses, truth, slots = edge_inputs(12)
    poses, truth, slots = poses[:L], truth[:L].copy(), slots[:L].copy()
    refused = (PHD_ERR_BAD_ARGUMENT, True)
    nav = make_nav(nav_mod, P, 0)
    assert raw(nav, 0, truth, slots) == refused                                     # the trajectory log is off
    nav.enable_history(L)
    assert raw(nav, 0, truth[:0], slots[:0]) == refused                             # ... and empty
    assert "empty" in nav._lib.phd_last_error(nav._h).decode()
    for k in range(L):
        nav.set_poses(poses[k])
        nav.append_history(k / 30.0)
    assert raw(nav, 0, truth, slots) == (0, False)
    assert raw(nav, 0, truth[:L - 1], slots) == refused                             # ntruth != L
    assert raw(nav, 0, truth, slots, ntruth=L + 1) == refused
    assert raw(nav, -1, truth, slots) == refused and raw(nav, 3, truth, slots) == refused
    assert raw(nav, 0, truth, slots, first=-1) == refused and raw(nav, 0, truth, slots, first=L) == refused
    assert raw(nav, 0, truth, slots, first=L - 1) == (0, False)
    assert raw(nav, 0, truth, slots, refentry=-1) == refused
    for bad in (-1, P):
        s = slots.copy()
        s[3] = bad
        assert raw(nav, 0, truth, s) == refused
    for value in (np.nan, np.inf):
        t = truth.copy()
        t[2, 5] = value
        assert raw(nav, 0, t, slots) == refused
        assert raw(nav, 0, truth, slots, slam=value) == refused
    t = truth.copy()
    t[4, 3:] = 0.0
    assert raw(nav, 0, t, slots) == refused                                         # a truth quaternion of norm 0
    assert "norm 0" in nav._lib.phd_last_error(nav._h).decode()
    assert raw(nav, 0, truth, None) == refused                                      # slots = NULL with the map log off
    assert "map log" in nav._lib.phd_last_error(nav._h).decode()
    # slots = NULL after a restart of the map log: the entries made before it name map entries that are gone
    nav.enable_map_history(4, 100)
    assert raw(nav, 0, truth, None) == refused
    nav.enable_history(L)                                                           # both logs on from the first entry: served
    for k in range(L):
        nav.set_poses(poses[k])
        nav.append_history(k / 30.0)
    assert raw(nav, 0, truth, None) == (0, False)
    nav.enable_map_history(4, 100)
    assert raw(nav, 0, truth, None) == refused
    assert "restarted" in nav._lib.phd_last_error(nav._h).decode()
    assert raw(nav, 0, truth, slots) == (0, False)                                  # (the slots handed over need no map log)
    nav.close()
    multi = nav_mod.PHDNavigator(hs.params_of((4, 1, 0.1, None)), particlecount=4, devices=[0, 0])
    assert raw(multi, 0, truth, slots) == refused
    multi.close()


def test_capacity_refusal(nav_mod):
    """A log of PHD_POSE_ERROR_MAX entries is served and one entry more is refused with PHD_ERR_CAPACITY in every mode, the
    outputs untouched. One particle that never moves, the truth its pose: at the bound Smooth mode (one workgroup, the slot row
    at its full 48 KB) must give location errors of 0 and rotation errors of at most 1e-7 (acos at 1) at every entry. That the
    refused call enqueues nothing cannot be seen from outside: the library decides it from the log's length on the host, before
    it touches the stream.
    The appends are one small launch each and nothing waits between them: the PHD_POSE_ERROR_MAX + 1 of them, the served call
    and the wait for all took 0.155 s on an MI355X, the whole test 0.16 s (printed below)."""
    header = open(os.path.join(ROOT, "include", "phdhip.h")).read()
    most = int(re.search(r"#define PHD_POSE_ERROR_MAX\s+(\d+)", header).group(1))
    t0 = time.perf_counter()
    nav = nav_mod.PHDNavigator(prm3d_defaults(max_particles=1, max_components=600, max_measurements=1), particlecount=1)
    nav.enable_history(most + 1)
    pose = np.array([0.5, -0.25, 1.0, 1.0, 0.0, 0.0, 0.0])
    nav.set_poses(pose[None])
    truth, slots = np.tile(pose, (most + 1, 1)), np.zeros(most + 1, np.int32)
    t1 = time.perf_counter()
    for k in range(most + 1):
        if k == most:                                          # at the bound: served
            t, loc, rot, ot, oloc, orot = nav.PoseError(truth[:most], mode="smooth", slots=slots[:most])
        nav.append_history(k / 30.0)
    nav.sync()
    t2 = time.perf_counter()
    assert len(t) == most and len(ot) == most - 9 and t[-1] == (most - 1) / 30.0 and ot[-1] == t[-1]
    assert np.all(loc == 0) and np.all(oloc == 0) and np.all(np.abs(rot) <= 1e-7) and np.all(np.abs(orot) <= 1e-7)
    for mode in range(3):
        assert raw(nav, mode, truth, slots) == (PHD_ERR_CAPACITY, True), mode
        assert "PHD_POSE_ERROR_MAX" in nav._lib.phd_last_error(nav._h).decode()
    assert raw(nav, 0, truth, slots, first=most) == (PHD_ERR_CAPACITY, True)
    nav.close()
    print("%d appends, the served call at the bound among them, and the wait for all: %.3f s; the whole test %.3f s" % (most + 1, t2 - t1, time.perf_counter() - t0))


# ---- 5. scripts/replay.py --posted --estimate waypoints --pose-error ---------------------------------------------------
def test_replay_writes_the_series(nav_mod, tmp_path):
    """The four files against pose_error_ref.py over the run's own estimate.out and trajectory.out, in all three modes.
    estimate.out holds the poses in g6, the device computed on the poses themselves. A coordinate or quaternion component
    below 1 moves by at most 5e-6 (half a unit of the sixth digit), a location by sqrt(3) times that and a unit quaternion's
    angle by twice the length of its perturbation, 2e-5 (scaling to norm 1 keeps the angle well conditioned in the
    perturbation). A value compares two of the estimate's poses: 4e-5, and is then written in g6 itself (5e-6 of a value
    below 1). 5e-5 covers both; means of such values move by no more. The times are g6 of the same numbers."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    rec = rio.read_record(replay.make_synthetic_record(str(tmp_path / "rec.zip"), frames=24))
    times, truth = replay.true_poses_of(rec)
    assert np.abs(truth).max() <= 1.0
    for mode in MODES:
        out = replay.replay(rec, 20, 5, replay.DeviceSolver, estimate="waypoints", posted=True, pose_error=mode, reftime=2 / 30.0)
        history = rio.trajectory_history_from_descriptor(out["estimate.out"], 7)
        assert len(history) == 24 and [len(path) for _, path in history] == list(range(2, 26))
        trajectory = [(float(t), x) for t, x in zip([0.0] + [t for t, _ in history], truth)]
        estimate = [(float(t), [(float(a), np.asarray(b, float)) for a, b in path]) for t, path in history]
        refentry = replay.reference_entry([t for t, _ in trajectory], 2 / 30.0)
        assert refentry in (2, 3)
        want = ref.all_series(mode, trajectory, estimate, refentry, replay.slam_time_of(rec))
        for name, (wt, wv) in zip(("locerror.out", "roterror.out", "odolocerror.out", "odoroterror.out"), want):
            rows = rio.timed_array_from_descriptor([l for l in out[name].split("\n") if l != ""], 1)
            gt, gv = np.array([t for t, _ in rows]), np.array([v[0] for _, v in rows])
            # (25 entries, the estimates from entry 1 on: Timed 24 values; Smooth 25 and 1 + 15; Filter 24 positions and 1 + 14)
            assert len(gt) == len(wt) == {ref.TIMED: (24, 24), ref.SMOOTH: (25, 16), ref.FILTER: (24, 15)}[mode]["odo" in name], (mode, name, len(gt))
            assert np.allclose(gt, wt, rtol=1e-5, atol=1e-9), (mode, name)
            assert same_kind(gv, wv), (mode, name, gv, wv)
            ok = ~np.isnan(wv)
            print("%s %s: %d values, largest %.3g, largest difference %.3g" % (mode, name, len(gv), np.max(wv[ok], initial=0.0), np.max(np.abs(gv[ok] - wv[ok]), initial=0.0)))
            assert np.all(np.abs(gv[ok] - wv[ok]) <= 5e-5), (mode, name, np.abs(gv[ok] - wv[ok]).max())
