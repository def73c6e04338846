"""The map log on the device (phd_map_history_enable / _append, phd_map_history) and the paths as of a past entry
(phd_trajectories_at), on the twelve-frame sequence of tests/history_seq.py: against the getters frame by frame, against the
oracle, posted without a wait, at the copy's edges, at its capacity, across a dropped step, through its lifecycle and through
scripts/replay.py --posted. Every comparison between two device runs is bit for bit."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import history_seq as hs
import orc
from monorfs_amd import _lib
from monorfs_amd import recordio as rio
from test_gpu_parity import assert_mix_close   # (the tolerances a step's pruned map is held to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (1024 particles: the smallest size at which a step runs on two streams; its oracle pattern is 001110111011)
ALL_CASES = hs.CASES + [(1024, 12, 0.1, None)]
CASES = pytest.mark.parametrize("case", ALL_CASES, ids=hs.CASE_IDS + ["P1024"])
EMPTY = (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3)))


@pytest.fixture(scope="module")
def nav_mod():
    from monorfs_amd import navigator
    return navigator


def make_nav(nav_mod, case, monkeypatch, entries=hs.FRAMES, components=hs.FRAMES * 600, history=hs.FRAMES, **over):
    if case[3] is not None:
        monkeypatch.setenv("PHD_NR_GRID_MIN", str(case[3]))   # (read when the handle is made)
    f = hs.frame_of(case)
    p = hs.params_of(case, **over)
    nav = nav_mod.PHDNavigator(p, particlecount=f.P)
    nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
    if history:
        nav.enable_history(history)
    if entries:
        nav.enable_map_history(entries, components)
    return nav, f, p


def same_entry(a, b):
    if not (a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and (a[3] is None) == (b[3] is None)):
        return False
    return a[3] is None or all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a[3], b[3]))


def assert_same_maps(got, want, what):
    assert len(got) == len(want), "%s: %d entries, expected %d" % (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert same_entry(a, b), "%s: entry %d differs (best %d / %d, %s / %s components)" % (
            what, k, a[1], b[1], "no" if a[3] is None else len(a[3][0]), "no" if b[3] is None else len(b[3][0]))


def state_entry(nav, t):
    """what the existing getters say the log's next entry is"""
    best = nav.BestParticle
    return (float(t), best, nav.poses()[best], nav.MapModel(best))


def assert_same_paths(a, b, what):
    for x, y, name in zip(a, b, ("times", "poses", "slots")):
        assert x.shape == y.shape and np.array_equal(x, y), "%s: %s" % (what, name)


_sync = {}


def sync_run(nav_mod, case, monkeypatch):
    """Run 1, once per case: every call waited for. Kept: the entries as the getters gave them behind every step, the log as
    read at the end, WayPoints right after every trajectory append and at the end."""
    if case in _sync:
        return _sync[case]
    nav, f, p = make_nav(nav_mod, case, monkeypatch)
    want, snaps = [], []
    for k, (t, noise, w, z, u) in enumerate(hs.inputs(case)):
        nav.UpdateOdometry(t, hs.READING, noise)          # (appends to the trajectory log)
        snaps.append(nav.WayPoints(range(f.P)))
        # the newest entry, nothing resampled since: the paths as of it are the current ones
        assert_same_paths(nav.WayPointsAt(k, range(f.P)), snaps[k], "frame %d: WayPointsAt of the newest entry" % k)
        nav.set_weights(w)
        nav.SlamUpdate(t, z, u_resample=u)                # (appends to the map log)
        want.append(state_entry(nav, t))
    got = nav.WayMaps()
    at = [nav.WayPointsAt(k, range(f.P)) for k in range(hs.FRAMES)]
    _sync[case] = {"want": want, "got": got, "snaps": snaps, "at": at, "final": nav.WayPoints(range(f.P)), "P": f.P}
    nav.close()
    return _sync[case]


@functools.lru_cache(maxsize=None)
def oracle_first_frame(case):
    """the oracle's best particle and best map behind the first frame's step"""
    f, p = hs.frame_of(case), hs.params_of(case)
    st = hs.oracle_state(f)
    t, noise, w, z, u = hs.inputs(case)[0]
    st.poses[:] = orc.update_motion(st.poses, hs.READING, noise, False)
    st.weights[:] = w
    best, src, res, _ = orc.slam_update(p, st, z, u=u, threads=8)
    return int(best), tuple(np.array(x) for x in st.map(best))


@CASES
def test_synchronous_run_logs_what_the_getters_gave(nav_mod, case, monkeypatch):
    assert hs.pattern_ok(hs.pattern(case)), "the sequence does not exercise the log: " + hs.pattern(case)
    run = sync_run(nav_mod, case, monkeypatch)
    assert_same_maps(run["got"], run["want"], "WayMaps against the getters")
    bests = [e[1] for e in run["got"]]
    assert bests == [r[3] for r in hs.oracle_run(case)], "best particles differ from the oracle's"
    assert len(set(bests)) > 1, "the best particle never changes"
    counts = [len(e[3][0]) for e in run["got"]]
    assert min(counts) >= 1 and max(counts) <= 600
    obest, omap = oracle_first_frame(case)
    assert run["got"][0][1] == obest
    assert_mix_close(run["got"][0][3], omap, 1e-7, "the first frame's logged map")


@CASES
def test_posted_without_a_wait(nav_mod, case, monkeypatch):
    """all twelve frames with no getter and no sync: motion, trajectory append, weights, measurements, step, map append"""
    run = sync_run(nav_mod, case, monkeypatch)
    paths = []
    for maplog in (True, False):
        nav, f, p = make_nav(nav_mod, case, monkeypatch, entries=hs.FRAMES if maplog else 0)
        for t, noise, w, z, u in hs.inputs(case):
            nav.UpdateOdometry(t, hs.READING, noise)
            nav.set_weights(w)
            nav.set_measurements(z)
            nav.step_async(u)
            if maplog:
                nav.append_map_history(t)
        if maplog:
            assert_same_maps(nav.WayMaps(), run["got"], "the posted run's WayMaps against the synchronous run's")
        paths.append(nav.WayPoints(range(f.P)))
        nav.sync()
        nav.close()
    assert_same_paths(paths[0], paths[1], "phd_trajectories with and without the map log")
    assert_same_paths(paths[0], run["final"], "phd_trajectories against the synchronous run")


@CASES
def test_waypoints_as_of_every_entry(nav_mod, case, monkeypatch):
    run = sync_run(nav_mod, case, monkeypatch)
    resampled_later = 0
    for k in range(hs.FRAMES):
        assert_same_paths(run["at"][k], run["snaps"][k], "WayPointsAt(%d) at the end against WayPoints right after that append" % k)
        assert run["at"][k][0].shape == (k + 1,) and np.array_equal(run["at"][k][2][:, k], np.arange(run["P"]))
        resampled_later += int(not np.array_equal(run["final"][2][:, k], run["at"][k][2][:, k]))
    assert resampled_later >= 3, "no resampling after the entries: WayPointsAt would equal a prefix of WayPoints"


def random_map(rng, n):
    a = rng.normal(size=(n, 3, 3))
    cov = a @ a.transpose(0, 2, 1) + np.eye(3)
    iu = np.triu_indices(3)
    cov[:, iu[1], iu[0]] = cov[:, iu[0], iu[1]]     # (exactly symmetric: the device keeps the upper triangle)
    return rng.uniform(0.1, 2.0, n), rng.normal(size=(n, 3)), cov


def raw_history(nav):
    n = C.c_int(0)
    t, b, x, cnt, off, w, m, c = _lib.dp(), _lib.ip(), _lib.dp(), _lib.ip(), _lib.i64p(), _lib.dp(), _lib.dp(), _lib.dp()
    rc = nav._lib.phd_map_history(nav._h, C.byref(n), C.byref(t), C.byref(b), C.byref(x), C.byref(cnt), C.byref(off), C.byref(w), C.byref(m), C.byref(c))
    return rc, [cnt[k] for k in range(n.value)], [off[k] for k in range(n.value + 1)]


def test_counts_at_the_copys_edges(nav_mod, monkeypatch):
    """No step: set_map on particle 0 (the best after reset), then append. The kernel moves 16 bytes per thread, five to a
    record, 256 threads to a workgroup: 51 / 52 and 102 / 103 records straddle a workgroup's edge (256 and 512 accesses),
    25 / 26 a pair of waves' (128 accesses, 256 doubles); 0 is the entry ResetHistory makes, 600 is max_components."""
    sizes = [0, 1, 25, 26, 51, 52, 102, 103, 600]
    p = hs.params_of((3, 1, 0.1, None))
    nav = nav_mod.PHDNavigator(p, particlecount=3)
    nav.enable_map_history(len(sizes), sum(sizes))
    rng = np.random.default_rng(7)
    models = [random_map(rng, n) for n in sizes]
    for n, model in zip(sizes, models):
        nav.set_map(0, model)
        nav.append_map_history()
    rc, counts, offsets = raw_history(nav)
    assert rc == 0 and counts == sizes and offsets == [int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]
    pose = nav.poses()[0]
    assert_same_maps(nav.WayMaps(), [(float(k), 0, pose, m) for k, m in enumerate(models)], "the maps that were set")
    nav.close()


CAP_CASE = hs.CASES[1]


def posted_maps(nav, case):
    for t, noise, w, z, u in hs.inputs(case):
        nav.UpdateOdometry(t, hs.READING, noise)
        nav.set_weights(w)
        nav.set_measurements(z)
        nav.step_async(u)
        nav.append_map_history(t)


def test_capacity(nav_mod, monkeypatch):
    case = CAP_CASE
    run = sync_run(nav_mod, case, monkeypatch)
    counts = [len(e[3][0]) for e in run["got"]]
    total = sum(counts)
    assert counts[-1] >= 2
    nav, f, p = make_nav(nav_mod, case, monkeypatch, entries=hs.FRAMES + 1, components=total, history=0)
    posted_maps(nav, case)
    assert_same_maps(nav.WayMaps(), run["got"], "components exactly the sum of the counts")
    nav.close()

    nav, f, p = make_nav(nav_mod, case, monkeypatch, entries=hs.FRAMES + 1, components=total - 1, history=0)
    posted_maps(nav, case)
    rc, got_counts, offsets = raw_history(nav)
    assert rc == 2 and "entry %d " % (hs.FRAMES - 1) in nav._lib.phd_last_error(nav._h).decode()
    assert got_counts == counts[:-1] + [-1] and offsets[-1] == offsets[-2] == total - counts[-1]
    with pytest.raises(nav_mod.PHDError) as e:
        nav.WayMaps()
    assert e.value.status == 2
    partial = nav.WayMaps(allow_missing=True)
    assert_same_maps(partial[:-1], run["got"][:-1], "the entries that fit")
    assert partial[-1][3] is None and partial[-1][1] == run["got"][-1][1] and np.array_equal(partial[-1][2], run["got"][-1][2])
    small = random_map(np.random.default_rng(5), 1)
    best = nav.BestParticle
    nav.set_map(best, small)
    nav.append_map_history(99.0)                                  # a later, smaller map fits what is left
    after = nav.WayMaps(allow_missing=True)
    assert_same_maps(after[:-1], partial, "the log before the small map")
    assert same_entry(after[-1], (99.0, best, nav.poses()[best], small))
    with pytest.raises(nav_mod.PHDError) as e:                    # entries used up: at once, and the log is as it was
        nav.append_map_history(100.0)
    assert e.value.status == 2
    assert_same_maps(nav.WayMaps(allow_missing=True), after, "after the refused append")
    nav.close()


DROP_CASE, DROP_FRAME = hs.CASES[1], 3


def test_a_dropped_step_logs_the_state_before_it(nav_mod, monkeypatch):
    """the means of test_gpu_history.test_a_dropped_step_composes_nothing: emit_capacity = max_quantity = 256 holds every frame
    of the sequence but not a frame of 128 scattered measurements; that step and the step queued behind it are dropped"""
    case = DROP_CASE
    rng = np.random.default_rng(1)
    many = np.column_stack([rng.uniform(-300, 300, 128), rng.uniform(-220, 220, 128), rng.uniform(0.3, 1.8, 128)])
    logs = []
    for drop in (True, False):
        nav, f, p = make_nav(nav_mod, case, monkeypatch, entries=hs.FRAMES + 1, history=0, max_quantity=256, emit_capacity=256, max_measurements=128)
        want = []
        for k, (t, noise, w, z, u) in enumerate(hs.inputs(case)):
            nav.UpdateOdometry(t, hs.READING, noise)
            nav.set_weights(w)
            if k != DROP_FRAME:
                nav.SlamUpdate(t, z, u_resample=u)
                want.append(state_entry(nav, t))
                continue
            if drop:
                nav.set_measurements(many)
                nav.step_async(u)
            nav.append_map_history(t)
            if drop:
                nav.step_async(u)                         # queued behind the failed one: dropped too
            nav.append_map_history(t + 0.01)
            if drop:
                with pytest.raises(nav_mod.PHDError) as e:
                    nav.sync()
                assert e.value.status == 2
            before = state_entry(nav, t)
            want += [before, (t + 0.01,) + before[1:]]
        logs.append(nav.WayMaps())
        assert_same_maps(logs[-1], want, "the log against the getters (%s)" % ("dropped steps" if drop else "no step at that frame"))
        nav.close()
    assert_same_maps(logs[0], logs[1], "a run with the dropped steps against a run without a step at that frame")
    assert logs[0][DROP_FRAME][1] == logs[0][DROP_FRAME - 1][1] and len(set(e[1] for e in logs[0][DROP_FRAME + 2:])) > 1


def test_lifecycle(nav_mod, monkeypatch):
    case = hs.CASES[0]
    frames = hs.inputs(case)
    nav, f, p = make_nav(nav_mod, case, monkeypatch, entries=4, history=0)

    def frame(k):
        t, noise, w, z, u = frames[k]
        nav.UpdateOdometry(t, hs.READING, noise)
        nav.set_weights(w)
        nav.SlamUpdate(t, z, u_resample=u)
        return state_entry(nav, t)

    def status_of(fn, *a, **kw):
        with pytest.raises(nav_mod.PHDError) as e:
            fn(*a, **kw)
        return e.value.status

    want = [frame(0), frame(1)]                                   # (the map log with the trajectory log off)
    assert status_of(nav.WayPoints, [0]) == 1 and status_of(nav.WayPointsAt, 0, [0]) == 1
    nav.set_frozen(True)                                          # frozen: info[0] describes a result the state never took
    assert status_of(nav.append_map_history, 5.0) == 1
    nav.set_frozen(False)
    assert_same_maps(nav.WayMaps(), want, "after the refused append")
    assert nav._lib.phd_step_local_async(nav._h, 0) == 1          # sharded entry points are refused while the log is on
    assert "map log" in nav._lib.phd_last_error(nav._h).decode()
    nav.enable_map_history(4, 2400)                               # enable again: restarts
    assert nav.WayMaps() == [] and nav.map_history_length == 0
    want = [frame(2)]
    assert_same_maps(nav.WayMaps(), want, "after the restart")
    nav.reset(f.poses[0], EMPTY, f.P)                             # reset restarts; its entry is the one ResetHistory makes
    assert nav.WayMaps() == []
    nav.append_map_history()                                      # time=None: the entry's index
    assert_same_maps(nav.WayMaps(), [(0.0, 0, f.poses[0], EMPTY)], "after the reset")
    nav.upload_state(f.planes(), f.counts, f.poses, f.weights)    # upload restarts
    assert nav.WayMaps() == []
    assert status_of(nav.enable_map_history, -1, 10) == 1
    nav.enable_map_history(0, 0)                                  # off: append and getter are refused
    assert status_of(nav.append_map_history, 0.0) == 1 and status_of(nav.WayMaps) == 1
    nav.enable_history(3)                                         # the trajectory log with the map log off
    for k in (3, 4):
        frame(k)
    t, x, s = nav.WayPoints(range(f.P))
    assert t.shape == (2,) and x.shape == (f.P, 2, 7) and s.shape == (f.P, 2)
    assert status_of(nav.WayPointsAt, 2, [0]) == 1 and status_of(nav.WayPointsAt, -1, [0]) == 1 and status_of(nav.WayPointsAt, 0, [f.P]) == 1
    assert nav.WayPointsAt(1, [0, f.P - 1])[2][:, 1].tolist() == [0, f.P - 1]
    nav.close()
    p2 = hs.params_of((4, 1, 0.1, None))
    multi = nav_mod.PHDNavigator(p2, particlecount=4, devices=[0, 0])
    with pytest.raises(nav_mod.PHDError) as e:
        multi.enable_map_history(4, 100)
    assert e.value.status == 1
    multi.close()


def test_replay_posted_writes_the_same_bytes(nav_mod, tmp_path):
    """scripts/replay.py --posted on the synthetic record: estimate.out and maps.out as strings, for both estimate modes"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    rec = rio.read_record(replay.make_synthetic_record(str(tmp_path / "rec.zip")))
    resampled = []

    class Watching(replay.DeviceSolver):
        def step(self, reading, noise, z, u):
            out = super().step(reading, noise, z, u)
            if len(z):
                resampled.append(self.nav.resample_sources()[1])
            return out

    plain = replay.replay(rec, 20, 5, Watching)
    assert any(resampled), "no frame of the replay resampled"
    assert plain == replay.replay(rec, 20, 5, replay.DeviceSolver, posted=False)
    for mode in ("poses", "waypoints"):
        sync = plain if mode == "poses" else replay.replay(rec, 20, 5, replay.DeviceSolver, estimate=mode)
        posted = replay.replay(rec, 20, 5, replay.DeviceSolver, estimate=mode, posted=True)
        assert posted["maps.out"] == sync["maps.out"], mode
        assert posted["estimate.out"] == sync["estimate.out"], mode
    assert len(rio.map_history_from_descriptor(plain["maps.out"])) == 12
