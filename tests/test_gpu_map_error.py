"""phd_map_error on the device: the OSPA distance, its cardinality and spatial parts and the estimate's size of every logged map
(Plot.MapError / Plot.OSPA / Map.BestMapEstimate) against the oracle at the kernel's shape edges, on degenerate entries, with
the alignment, through real steps, at its refusals and capacity, and through scripts/replay.py --posted --map-error.

Maps are logged without steps, as test_gpu_map_history.test_counts_at_the_copys_edges does: set_map on particle 0 (the best
after a reset), then append_map_history. Covariances are the identity.

Tolerances. ospa and cardinality: 1e-12 * C — the value is a mean of at most 1024 pair costs, each good to a few ulp (about
2.3e-13 relative in all); different optimal assignments give the same optimum. spatial: compared as spatial^P within
1e-12 * C^P (it is the root of a difference, which the root would magnify next to 0)."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import history_seq as hs
import orc
import rigid
from monorfs_amd import recordio as rio
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, PHD_ERR_CAPACITY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (41, 42)
TRUTH_SIZES = (1, 5, 64, 65, 130)
MAP_SIZES = (0, 1, 2, 63, 64, 65, 129, 257)      # a wave's edge, more than one workgroup's worth of threads, both empty sets
CP_CASES = ((1.0, 1.0), (0.5, 2.0), (5.0, 2.0))
BOUND = 1024                                     # PHD_MAP_ERROR_MAX
EMPTY = (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3)))


@pytest.fixture(scope="module")
def nav_mod():
    from monorfs_amd import navigator
    return navigator


def make_nav(nav_mod, entries, components, particles=3):
    p = hs.params_of((particles, 1, 0.1, None))
    nav = nav_mod.PHDNavigator(p, particlecount=particles)
    if entries:
        nav.enable_map_history(entries, components)
    return nav


def log_maps(nav, maps):
    for m in maps:
        nav.set_map(0, m)
        nav.append_map_history()


def with_identity(w, mean):
    w, mean = np.asarray(w, float), np.asarray(mean, float).reshape(-1, 3)
    return w, mean, np.tile(np.eye(3), (len(w), 1, 1))


def expected(truth, model, C, P, poses=None):
    """the oracle's (ospa, cardinality, spatial, size) of one logged map"""
    est = orc.best_map_estimate(model)[0] if len(model[0]) else np.zeros((0, 3))
    card = orc.ospa(truth, est, C, P)[1]                                   # (the sizes alone decide it)
    if poses is None:
        ospa, spatial = orc.map_error(truth, est, cutoff=C, order=P)
    else:
        ospa, spatial = orc.map_error(truth, est, poses[0], poses[1], C, P)
    return ospa, card, spatial, len(est)


def assert_close(got, want, C, P, what):
    """got: (time, ospa, cardinality, spatial, size) of the device; want: expected()"""
    print("%s: size %d / %d, ospa %.17g / %.17g, cardinality %.17g / %.17g, spatial %.17g / %.17g" % (
        what, got[4], want[3], got[1], want[0], got[2], want[1], got[3], want[2]))
    assert got[4] == want[3], "%s: estimate of %d landmarks, the oracle's has %d" % (what, got[4], want[3])
    assert abs(got[1] - want[0]) <= 1e-12 * C, "%s: ospa %r, oracle %r" % (what, got[1], want[0])
    assert abs(got[2] - want[1]) <= 1e-12 * C, "%s: cardinality %r, oracle %r" % (what, got[2], want[1])
    assert abs(got[3] ** P - want[2] ** P) <= 1e-12 * C ** P, "%s: spatial %r, oracle %r" % (what, got[3], want[2])


# ---- 1. against the oracle at the shape edges ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_inputs(seed):
    """per truth size: (truth[nt][3], [map of n components for n in MAP_SIZES])"""
    rng = np.random.default_rng(seed)
    out = {}
    for nt in TRUTH_SIZES:
        truth = rng.uniform(-2, 2, (nt, 3))
        maps = []
        for n in MAP_SIZES:
            w = rng.uniform(0.3, 1.3, n)
            if n > 2:
                w[0] = 2.6                                                        # picked twice
            mean = truth[rng.integers(0, nt, n)] + rng.normal(0, 0.05, (n, 3))
            far = rng.uniform(size=n) < 0.2                                      # one fifth beyond every cut-off
            mean[far] += rng.uniform(3, 4, (int(far.sum()), 3))
            maps.append(with_identity(w, mean))
        out[nt] = (truth, maps)
    return out


def assert_preconditions(truth, model, C, P, what):
    """rounding must not decide the result: the weight sum away from an integer, no pair on the 1e-5 storage threshold, the
    spatial part away from 0"""
    w = model[0]
    if len(w):
        s = float(np.sum(w))
        assert abs(s - round(s)) >= 1e-6, "%s: the weight sum %r lies on an integer" % (what, s)
    est = orc.best_map_estimate(model)[0] if len(w) else np.zeros((0, 3))
    if len(est) and len(truth):
        d = np.sqrt(((truth[:, None, :] - est[None, :, :]) ** 2).sum(axis=2))
        gain = C ** P - np.minimum(C, d) ** P
        assert np.all(np.abs(gain - 1e-5) >= 1e-9), "%s: a pair on the storage threshold" % what
        ospa, card = orc.ospa(truth, est, C, P)
        assert ospa ** P - card ** P >= 1e-9 * C ** P, "%s: the spatial part lies on 0" % what


@pytest.mark.parametrize("nt", TRUTH_SIZES)
@pytest.mark.parametrize("seed", SEEDS)
def test_against_the_oracle_at_the_shape_edges(nav_mod, seed, nt):
    truth, maps = edge_inputs(seed)[nt]
    nav = make_nav(nav_mod, len(maps), sum(MAP_SIZES))
    log_maps(nav, maps)
    twice = 0
    for C, P in CP_CASES:
        got = nav.MapError(truth, C, P)
        assert len(got) == len(maps) and [g[0] for g in got] == [float(k) for k in range(len(maps))]
        for k, (n, model) in enumerate(zip(MAP_SIZES, maps)):
            what = "seed %d, %d truth points, %d components, C %g, P %g" % (seed, nt, n, C, P)
            assert_preconditions(truth, model, C, P, what)
            assert_close(got[k], expected(truth, model, C, P), C, P, what)
            if n > 2:
                src = orc.best_map_estimate(model)[1]
                twice += int(np.count_nonzero(src == 0) >= 2)
    assert twice == 3 * sum(1 for n in MAP_SIZES if n > 2), "the heavy component is not picked twice in every map"
    sizes = [g[4] for g in nav.MapError(truth)]
    assert any(s > nt for s in sizes) or nt > 200, "no estimate larger than the truth set"
    assert any(0 < s < nt for s in sizes) or nt == 1, "no estimate smaller than the truth set"
    nav.close()


# ---- 2. degenerate entries, exact values ------------------------------------------------------------------------------------
def test_degenerate_entries_are_exact(nav_mod):
    rng = np.random.default_rng(43)
    truth = rng.uniform(-2, 2, (70, 3))
    same = with_identity(np.ones(70), truth[::-1])                        # the truth set itself, in another order
    beyond = with_identity(np.ones(9), truth[:9] + [40.0, 0.0, 0.0])      # every pair beyond every cut-off
    nav = make_nav(nav_mod, 2, 79)
    log_maps(nav, [same, beyond])
    for C, P in CP_CASES:
        got = nav.MapError(truth, C, P)
        assert got[0][1:] == (0.0, 0.0, 0.0, 70), (C, P, got[0])
        assert got[1][1] == C and got[1][4] == 9, (C, P, got[1])
        assert_close(got[1], expected(truth, beyond, C, P), C, P, "beyond the cut-off, C %g, P %g" % (C, P))
        got = nav.MapError(truth[:9] - [40.0, 0.0, 0.0], C, P)            # m = n and every pair beyond the cut-off: no cardinality part
        assert got[1][1:] == (C, 0.0, C, 9), (C, P, got[1])
        got = nav.MapError(np.zeros((0, 3)), C, P)                        # an empty truth set against non-empty maps
        assert got[0][1:] == (C, C, 0.0, 70) and got[1][1:] == (C, C, 0.0, 9), (C, P, got)
    nav.close()


# ---- 3. the alignment -----------------------------------------------------------------------------------------------------
def test_alignment(nav_mod):
    rng = np.random.default_rng(44)
    truth = rng.uniform(-2, 2, (12, 3))
    n = 15
    w = rng.uniform(0.3, 1.3, n)
    w[0] = 2.6
    mean = truth[rng.integers(0, 12, n)] + rng.normal(0, 0.05, (n, 3))
    # Plot.MapError turns about the estimated location by the pose difference as the TRUE pose's frame sees it: with a true pose
    # that looks along the world's axes the alignment undoes the motion exactly, with any other it does not (and need not:
    # the oracle states the same formula). Three entries of the first kind, one of the second.
    upright = np.array([0.3, -0.2, 0.5, 1.0, 0.0, 0.0, 0.0])
    turned = np.array([0.3, -0.2, 0.5, 0.9, 0.1, -0.3, 0.2])
    turned[3:] /= np.linalg.norm(turned[3:])
    names = ["x90", "generic-negw", "y180", "axes120"]
    maps, pairs = [], []
    for name in names:
        q = rigid.POSES[name]
        true_pose = turned if name == "axes120" else upright
        maps.append(with_identity(w, rigid.move_points(mean, q)))           # the map and its estimated pose, moved together
        pairs.append((rigid.move_poses(true_pose, q), true_pose))
    nav = make_nav(nav_mod, len(maps), n * len(maps))
    log_maps(nav, maps)
    skipped = 2
    for C, P in CP_CASES:
        aligned = nav.MapError(truth, C, P, align=pairs)
        plain = nav.MapError(truth, C, P)
        mixed = nav.MapError(truth, C, P, align=[None if k == skipped else pr for k, pr in enumerate(pairs)])
        unmoved = expected(truth, with_identity(w, mean), C, P)
        for k, name in enumerate(names):
            what = "%s, C %g, P %g" % (name, C, P)
            assert_close(aligned[k], expected(truth, maps[k], C, P, pairs[k]), C, P, what + ", aligned")
            assert_close(plain[k], expected(truth, maps[k], C, P), C, P, what + ", not aligned")
            assert mixed[k] == (plain[k] if k == skipped else aligned[k]), what + ", has_reference"
            # the alignment undoes the motion (to rounding: 1e-9 is far above it and far below the motion's effect)
            if name != "axes120":
                assert abs(aligned[k][1] - unmoved[0]) <= 1e-9 * C and plain[k][1] > aligned[k][1] + 1e-3 * C, what
    nav.close()


# ---- 4. through real steps -------------------------------------------------------------------------------------------------
def test_through_real_steps(nav_mod, monkeypatch):
    case = hs.CASES[hs.CASE_IDS.index("P64")]
    f, p = hs.frame_of(case), hs.params_of(case)
    nav = nav_mod.PHDNavigator(p, particlecount=f.P)
    nav.upload_state(f.planes(), f.counts, f.poses, f.weights)
    nav.enable_map_history(hs.FRAMES, hs.FRAMES * 600)
    times = []
    for t, noise, w, z, u in hs.inputs(case):                             # posted: no getter and no wait between the frames
        nav.UpdateOdometry(t, hs.READING, noise)
        nav.set_weights(w)
        nav.set_measurements(z)
        nav.step_async(u)
        nav.append_map_history(t)
        times.append(float(t))
    truth = f.mean[0][:20] + 0.01                                         # near some of the landmarks the maps hold
    for C, P in CP_CASES:
        got = nav.MapError(truth, C, P)
        maps = nav.WayMaps()
        assert [g[0] for g in got] == times == [m[0] for m in maps]
        for k, entry in enumerate(maps):
            assert_close(got[k], expected(truth, entry[3], C, P), C, P, "frame %d, C %g, P %g" % (k, C, P))
    assert min(g[4] for g in got) >= 1
    nav.sync()
    nav.close()


# ---- 5. refusals and capacity ---------------------------------------------------------------------------------------------
def status_of(nav_mod, fn, *a, **kw):
    with pytest.raises(nav_mod.PHDError) as e:
        fn(*a, **kw)
    return e.value.status


def test_refusals(nav_mod):
    truth = np.random.default_rng(45).uniform(-2, 2, (6, 3))
    nav = make_nav(nav_mod, 0, 0)
    assert status_of(nav_mod, nav.MapError, truth) == PHD_ERR_BAD_ARGUMENT            # the log is off
    assert "map log is off" in nav._lib.phd_last_error(nav._h).decode()
    nav.enable_map_history(2, 10)
    log_maps(nav, [with_identity([0.9, 1.4], truth[:2])])
    bad = truth.copy()
    bad[3, 1] = np.nan
    assert status_of(nav_mod, nav.MapError, bad) == PHD_ERR_BAD_ARGUMENT
    assert status_of(nav_mod, nav.MapError, truth, 0.0) == PHD_ERR_BAD_ARGUMENT
    assert status_of(nav_mod, nav.MapError, truth, -1.0) == PHD_ERR_BAD_ARGUMENT
    assert status_of(nav_mod, nav.MapError, truth, 1.0, 0.5) == PHD_ERR_BAD_ARGUMENT
    assert status_of(nav_mod, nav.MapError, np.zeros((BOUND + 1, 3))) == PHD_ERR_BAD_ARGUMENT
    pose = np.array([0.0, 0, 0, 1, 0, 0, 0])
    assert status_of(nav_mod, nav.MapError, truth, align=[(pose + np.inf, pose)]) == PHD_ERR_BAD_ARGUMENT
    assert len(nav.MapError(np.zeros((BOUND, 3)))) == 1                             # the bound itself is served
    assert nav.MapError(truth)[0][4] == 2
    nav.close()
    multi = nav_mod.PHDNavigator(hs.params_of((4, 1, 0.1, None)), particlecount=4, devices=[0, 0])
    assert status_of(nav_mod, multi.MapError, truth) == PHD_ERR_BAD_ARGUMENT
    multi.close()


def test_capacity_repeats_and_leaves_the_logs_alone(nav_mod):
    rng = np.random.default_rng(46)
    truth = rng.uniform(-2, 2, (7, 3))

    def some_map(n):
        return with_identity(rng.uniform(0.3, 1.3, n) + 0.0123, truth[rng.integers(0, 7, n)] + rng.normal(0, 0.05, (n, 3)))

    maps = [some_map(3), some_map(7), some_map(4), with_identity([600.25, 600.5], truth[:2])]   # the last: an estimate of 1200
    nav = make_nav(nav_mod, len(maps), 3 + 4 + 2)                                               # the second does not fit: count -1
    nav.enable_history(2)
    nav.append_history(0.0)
    log_maps(nav, maps)
    before = nav.WayMaps(allow_missing=True)
    paths = nav.WayPoints(range(3))
    assert [None if e[3] is None else len(e[3][0]) for e in before] == [3, None, 4, 2]
    assert status_of(nav_mod, nav.MapError, truth) == PHD_ERR_CAPACITY
    assert "entry 1 " in nav._lib.phd_last_error(nav._h).decode()
    got = nav.MapError(truth, allow_missing=True)
    again = nav.MapError(truth, allow_missing=True)
    assert np.array_equal(np.array(got).view(np.uint64), np.array(again).view(np.uint64)), "two calls, different bits"
    assert got[1][4] == -1 and all(np.isnan(got[1][1:4]))
    assert got[3][4] == 1200 and all(np.isnan(got[3][1:4]))
    for k in (0, 2):
        assert_close(got[k], expected(truth, maps[k], 1.0, 1.0), 1.0, 1.0, "entry %d beside the ones without values" % k)
    after = nav.WayMaps(allow_missing=True)
    assert len(after) == len(before)
    for a, b in zip(after, before):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and (a[3] is None) == (b[3] is None)
        assert a[3] is None or all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    assert all(np.array_equal(x, y) for x, y in zip(nav.WayPoints(range(3)), paths))
    assert np.array_equal(nav.MapModel(0)[0], maps[-1][0])                                      # the state is the last map set
    nav.close()
    # an estimate over the bound alone is named too
    nav = make_nav(nav_mod, 1, 2)
    log_maps(nav, maps[3:])
    assert status_of(nav_mod, nav.MapError, truth) == PHD_ERR_CAPACITY
    assert "1200" in nav._lib.phd_last_error(nav._h).decode()
    nav.close()


# ---- 6. replay ------------------------------------------------------------------------------------------------------------
def test_replay_writes_the_series(nav_mod, tmp_path, monkeypatch, capsys):
    """scripts/replay.py --posted --map-error on tests/golden/record: one line per frame, the oracle's values on the maps.out
    written beside it. maps.out holds the means in g6, the device computed on the means themselves: a coordinate of up to 10
    moves by up to 5e-6 (half a unit of the sixth digit), a distance by up to sqrt(3) times that, the OSPA (C = P = 1: a mean of
    distances) by no more; the value is then written in g6 itself, half a unit of its sixth digit (5e-7 below 1). 1e-5 covers
    both. The weights' sums must not lie within 1e-4 of an integer, where g6 could change the estimate's size."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import replay
    out = str(tmp_path / "out")
    monkeypatch.setattr(sys, "argv", ["replay.py", os.path.join(ROOT, "tests", "golden", "record"), "--posted", "--map-error",
                                      "--particles", "20", "--seed", "5", "--out", out])
    replay.main()
    assert "replayed 3 frames" in capsys.readouterr().out
    rec = rio.read_record(os.path.join(ROOT, "tests", "golden", "record"))
    truth = replay.truth_of(rec)
    assert truth.shape == (3, 3)
    maps = rio.map_history_from_descriptor(open(os.path.join(out, "maps.out")).read())
    series = {}
    for name in ("maperror.out", "spatialmaperror.out"):
        lines = [l for l in open(os.path.join(out, name)).read().split("\n") if l != ""]
        assert len(lines) == len(maps) == 3, name
        series[name] = rio.timed_array_from_descriptor(lines, 1)
    nonempty = 0
    for k, (t, model) in enumerate(maps):
        s = float(np.sum(model[0]))
        assert len(model[0]) == 0 or abs(s - round(s)) >= 1e-4, "frame %d: the weight sum %r lies on an integer" % (k, s)   # (an empty map's 0 is exact)
        ospa, card, spatial, size = expected(truth, model, 1.0, 1.0)
        nonempty += int(size > 0)
        for name, want in (("maperror.out", ospa), ("spatialmaperror.out", spatial)):
            tk, value = series[name][k]
            print("frame %d %s: %r, oracle %r" % (k, name, float(value[0]), want))
            assert rio.g6(tk) == rio.g6(t) and abs(float(value[0]) - want) <= 1e-5, (k, name, float(value[0]), want)
    assert nonempty >= 1, "every estimate of the replay is empty"
