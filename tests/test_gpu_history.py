"""The trajectory log on the device (phd_history_enable / phd_history_append / phd_trajectories) against the reference's
meaning of a particle's path, a list per particle (tests/history_seq.py): synchronously, against the oracle in lockstep,
posted without a wait, across a dropped step, in frozen mode, at its capacity and through scripts/replay.py."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import history_seq as hs
import orc
from monorfs_amd import recordio as rio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = pytest.mark.parametrize("case", hs.CASES, ids=hs.CASE_IDS)


@pytest.fixture(scope="module")
def nav_mod():
    from monorfs_amd import navigator
    return navigator


def make_nav(nav_mod, case, monkeypatch, capacity=hs.FRAMES, **over):
    if case[3] is not None:
        monkeypatch.setenv("PHD_NR_GRID_MIN", str(case[3]))   # (read when the handle is made)
    f = hs.frame_of(case)
    p = hs.params_of(case, **over)
    nav = nav_mod.PHDNavigator(p, particlecount=f.P)
    nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
    if capacity:
        nav.enable_history(capacity)
    return nav, f, p


def assert_equals_model(nav, model, what):
    t, x, s = nav.WayPoints(range(model.P))
    assert np.array_equal(t, model.times), what + ": times"
    assert np.array_equal(s, model.slots), what + ": slots"
    assert np.array_equal(x, model.poses), what + ": poses"


def assert_pattern(case, skip=()):
    """(from the oracle's flags, not from the device)"""
    pat = hs.pattern(case) if not skip else "".join("1" if r[2] else "0" for r in hs.oracle_run(case, skip))
    assert hs.pattern_ok(pat), "the sequence does not exercise the log: " + pat


def sync_frame(nav, model, frame, what, step=True):
    """one frame with a wait after every call: the motion step and its append, then the step; the model follows the device"""
    t, noise, w, z, u = frame
    nav.UpdateOdometry(t, hs.READING, noise)          # (appends)
    moved = nav.poses()
    model.append(t, moved)
    assert_equals_model(nav, model, what + " after the append")
    nav.set_weights(w)
    if not step:
        return moved
    nav.SlamUpdate(None, z, u_resample=u)
    src, res = nav.resample_sources()
    if res:
        model.resample(src)
    assert np.array_equal(nav.poses(), moved[src]), what + ": the step's own poses"
    assert_equals_model(nav, model, what + " after the step")   # (resamplings since the last append: the pending map)
    return res


_final = {}


def sync_run(nav_mod, case, monkeypatch):
    """the whole sequence synchronously; its final WayPoints are kept for the test that posts it without a wait"""
    nav, f, p = make_nav(nav_mod, case, monkeypatch)
    model = hs.ListModel(f.P)
    flags = []
    for k, frame in enumerate(hs.inputs(case)):
        flags.append(sync_frame(nav, model, frame, "frame %d" % k))
    _final[case] = nav.WayPoints(range(f.P))
    nav.close()
    return flags


@CASES
def test_synchronous_run_equals_the_list_model(nav_mod, case, monkeypatch):
    assert_pattern(case)
    flags = sync_run(nav_mod, case, monkeypatch)
    assert "".join("1" if r else "0" for r in flags) == hs.pattern(case), "the device resampled at other frames than the oracle"


@CASES
def test_lockstep_with_the_oracle(nav_mod, case, monkeypatch):
    """the model fed by the oracle alone (its motion step from the device's poses of the frame before, its sources): slots
    exact, poses to the 1e-14 tests/test_gpu_parity.py holds the motion step to"""
    assert_pattern(case)
    nav, f, p = make_nav(nav_mod, case, monkeypatch)
    st = hs.oracle_state(f)
    model = hs.ListModel(f.P)

    def check(what):
        t, x, s = nav.WayPoints(range(f.P))
        assert np.array_equal(t, model.times) and np.array_equal(s, model.slots), what
        assert np.allclose(x, model.poses, rtol=0, atol=1e-14), "%s: %g" % (what, np.max(np.abs(x - model.poses)))

    for k, (t, noise, w, z, u) in enumerate(hs.inputs(case)):
        want = orc.update_motion(st.poses, hs.READING, noise, False)
        nav.UpdateOdometry(t, hs.READING, noise)
        model.append(t, want)
        check("frame %d after the append" % k)
        st.poses[:] = nav.poses()                     # lockstep: the oracle goes on from the device's poses
        st.weights[:] = w
        nav.set_weights(w)
        best, src, res, _ = orc.slam_update(p, st, z, u=u, threads=8)
        nav.SlamUpdate(None, z, u_resample=u)
        if res:
            model.resample(src)
        check("frame %d after the step" % k)
    nav.close()


@CASES
def test_posted_without_a_wait(nav_mod, case, monkeypatch):
    """motion, append, weights, measurements and step posted for all twelve frames with no getter and no sync in between"""
    if case not in _final:
        sync_run(nav_mod, case, monkeypatch)
    nav, f, p = make_nav(nav_mod, case, monkeypatch)
    for t, noise, w, z, u in hs.inputs(case):
        nav.UpdateOdometry(t, hs.READING, noise)
        nav.set_weights(w)
        nav.set_measurements(z)
        nav.step_async(u)
    got = nav.WayPoints(range(f.P))
    nav.sync()
    for a, b in zip(got, _final[case]):
        assert np.array_equal(a, b)
    nav.close()


DROP_CASE, DROP_FRAME = hs.CASES[1], 3


def test_a_dropped_step_composes_nothing(nav_mod, monkeypatch):
    """emit_capacity = max_quantity = 256 holds every frame of the sequence (the oracle counts at most 173 corrected components
    of MinWeight or more in any particle) but not a frame of 128 scattered measurements (at least 373 are certain to be
    emitted: every misdetection copy of MinWeight or more and the 256 heaviest entries). That step, at a frame whose weights
    would have made it resample, and the step queued behind it are dropped with PHD_ERR_CAPACITY. The log, and the frames
    after, are those of a model in which the step did nothing."""
    case = DROP_CASE
    assert_pattern(case, skip=(DROP_FRAME,))
    nav, f, p = make_nav(nav_mod, case, monkeypatch, max_quantity=256, emit_capacity=256, max_measurements=128)
    model = hs.ListModel(f.P)
    rng = np.random.default_rng(1)
    many = np.column_stack([rng.uniform(-300, 300, 128), rng.uniform(-220, 220, 128), rng.uniform(0.3, 1.8, 128)])
    resampled_after = 0
    for k, frame in enumerate(hs.inputs(case)):
        if k != DROP_FRAME:
            res = sync_frame(nav, model, frame, "frame %d" % k)
            resampled_after += int(res and k > DROP_FRAME)
            continue
        moved = sync_frame(nav, model, frame, "frame %d" % k, step=False)
        nav.set_measurements(many)
        nav.step_async(frame[4])
        nav.step_async(frame[4])                      # queued behind the failed one: dropped too
        with pytest.raises(nav_mod.PHDError) as e:
            nav.sync()
        assert e.value.status == 2
        assert np.array_equal(nav.poses(), moved)
        assert_equals_model(nav, model, "after the dropped step")
    assert resampled_after >= 1
    nav.close()


def test_frozen_steps_compose_nothing(nav_mod, monkeypatch):
    case = hs.CASES[2]
    nav, f, p = make_nav(nav_mod, case, monkeypatch)
    model = hs.ListModel(f.P)
    frames = hs.inputs(case)
    for k in range(6):
        sync_frame(nav, model, frames[k], "frame %d" % k)
    before = nav.WayPoints(range(f.P))
    nav.set_frozen(True)
    for k in (2, 3):
        nav.set_weights(hs.skewed_weights(f.P, k))
        nav.SlamUpdate(None, frames[k][3], u_resample=frames[k][4])
        assert nav.resample_sources()[1], "the frozen step was meant to resample"
        for a, b in zip(nav.WayPoints(range(f.P)), before):
            assert np.array_equal(a, b)
    nav.set_frozen(False)
    for k in range(6, hs.FRAMES):
        sync_frame(nav, model, frames[k], "frame %d" % k)
    nav.close()


def test_capacity_and_lifecycle(nav_mod, monkeypatch):
    case = hs.CASES[0]
    nav, f, p = make_nav(nav_mod, case, monkeypatch, capacity=4)
    model = hs.ListModel(f.P)
    frames = hs.inputs(case)
    for k in range(4):
        sync_frame(nav, model, frames[k], "frame %d" % k)
    with pytest.raises(nav_mod.PHDError) as e:
        nav.append_history(9.0)
    assert e.value.status == 2
    assert_equals_model(nav, model, "after the refused append")
    with pytest.raises(nav_mod.PHDError) as e:
        nav.WayPoints([f.P])
    assert e.value.status == 1
    assert nav._lib.phd_step_local_async(nav._h, 0) == 1          # sharded entry points are refused while the log is on
    nav.enable_history(8)                                         # restarts
    assert nav.WayPoints(range(f.P))[1].shape == (f.P, 0, 7)
    model = hs.ListModel(f.P)
    sync_frame(nav, model, frames[4], "after the restart")
    nav.reset(f.poses[0], (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3))), f.P)
    assert nav.WayPoints(range(f.P))[0].shape == (0,)
    nav.append_history()                                          # time=None: the entry's index
    t, x, s = nav.WayPoints([0, f.P - 1])
    assert np.array_equal(t, [0.0]) and np.array_equal(s, [[0], [f.P - 1]]) and np.array_equal(x[:, 0], nav.poses()[[0, f.P - 1]])
    nav.enable_history(0)                                         # off: appends and the getter are refused
    with pytest.raises(nav_mod.PHDError) as e:
        nav.append_history(0.0)
    assert e.value.status == 1
    nav.close()
    p2 = hs.params_of((4, 1, 0.1, None))
    multi = nav_mod.PHDNavigator(p2, particlecount=4, devices=[0, 0])
    with pytest.raises(nav_mod.PHDError) as e:
        multi.enable_history(4)
    assert e.value.status == 1
    multi.close()


def test_replay_writes_the_best_particles_path(nav_mod, tmp_path):
    """scripts/replay.py with estimate="waypoints" against the oracle behind the same interface with the list model, compared
    as tests/test_recordio.py compares estimate.out; the default output is untouched"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    rec = rio.read_record(replay.make_synthetic_record(str(tmp_path / "rec.zip")))
    resampled = []

    class OracleSolver:
        def __init__(self, p, pose, particles):
            self.p, self.st, self.best = p, orc.State(particles, 900), 0
            self.st.poses[:] = pose

        def start_waypoints(self, capacity):
            self.model = hs.ListModel(len(self.st.poses))
            self.model.append(0.0, self.st.poses)

        def step_waypoints(self, time, reading, noise, z, u):
            self.st.poses[:] = orc.update_motion(self.st.poses, reading, noise)
            self.model.append(time, self.st.poses)
            way = (self.model.times.copy(), self.model.poses[self.best].copy())
            if len(z):
                self.best, src, res, _ = orc.slam_update(self.p, self.st, z, u=u, threads=8)
                resampled.append(bool(res))
                if res:
                    self.model.resample(src)
            return way, tuple(np.array(x) for x in self.st.map(self.best))

    dev = replay.replay(rec, 20, 5, replay.DeviceSolver, estimate="waypoints")
    ref = replay.replay(rec, 20, 5, OracleSolver, estimate="waypoints")
    assert any(resampled), "no frame of the replay resampled: the path would be the list of best poses"
    dest = rio.trajectory_history_from_descriptor(dev["estimate.out"], 7)
    rest = rio.trajectory_history_from_descriptor(ref["estimate.out"], 7)
    assert len(dest) == len(rest) == 12
    for k, ((td, a), (tr, b)) in enumerate(zip(dest, rest)):
        assert td == tr and len(a) == len(b) == k + 2
        assert all(x[0] == y[0] and np.allclose(x[1], y[1], rtol=2e-5, atol=1e-9) for x, y in zip(a, b))
    plain = replay.replay(rec, 20, 5, replay.DeviceSolver)
    assert plain == replay.replay(rec, 20, 5, replay.DeviceSolver, estimate="poses")
    assert plain["estimate.out"] != dev["estimate.out"] and plain["maps.out"] == dev["maps.out"]
