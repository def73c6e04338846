"""phd_quasi_ascent_multi / phd_quasi_set_loglik_multi on the device: every estimate (pose) of a call over many problems bit for
bit what the single calls of the same handle give it with its problem alone — whole ascents with the estimates of three
problems interleaved, the edges of a problem, the batch calls, the measurement-block classes, the refusals, that nothing else
of the handle moves, the fits of many frames through it, and the C++ host mirror."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from loopy_stub import scene
from monorfs_amd import _lib, loopy
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, PHD_ERR_CAPACITY, prm3d_defaults
from monorfs_amd.navigator import PHDError, pose3d_add
from monorfs_amd.synth import Frame
from test_ascent_multi_abi import frames

SCALE = [4e-3, 4e-3, 4e-3, 2e-3, 2e-3, 2e-3]
RUNS = {21: (10, 7, 6, 1.0), 31: (6, 5, 1, 0.3), 61: (3, 2, 4, 1.0)}   # tests/test_gpu_ascent.py: seed: landmarks, measurements, starts, sigma
# the linearisation pose of each problem: the scene's, moved and rotated by this; the starts are restated in its chart, so that
# they are the poses they were and the searches climb as they did
ROTATE = {21: [0.01, -0.02, 0.005, 0.4, -0.7, 0.5], 31: [-0.02, 0.01, 0.01, -0.3, 0.2, 0.6], 61: [0.0, 0.015, -0.01, 0.5, 0.5, -0.4]}
ORDER = [0, 2, 0, 1, 2, 0, 2, 0, 2, 0, 0]   # the problem of each of the 11 estimates


def params(max_measurements=16):
    return prm3d_defaults(max_particles=256, max_components=600, max_measurements=max_measurements)


@pytest.fixture(scope="module")
def nav():
    from monorfs_amd import navigator
    n = navigator.PHDNavigator(params(), particlecount=1)
    yield n
    n.close()


@pytest.fixture(scope="module")
def nav128():
    from monorfs_amd import navigator
    n = navigator.PHDNavigator(params(128), particlecount=1)
    yield n
    n.close()


def rechart(lin, rotated, starts):
    """the linear poses `starts` around `lin`, restated around `rotated`"""
    return np.array([loopy.pose3d_subtract(pose3d_add(lin, s), rotated) for s in starts])


def three(p):
    """the three problems (landmarks, measurements, a rotated linearisation pose of their own), the 11 starts interleaved as ORDER
    says, and per problem the indices of its estimates"""
    problems, starts = [], []
    for seed in (21, 31, 61):
        J, M, n, sigma = RUNS[seed]
        rng = np.random.default_rng(seed)
        lin, lm, z = scene(rng, p, J, M, sigma=sigma)
        rotated = pose3d_add(lin, ROTATE[seed])
        starts.append(rechart(lin, rotated, rng.normal(0, 1, (n, 6)) * SCALE))
        problems.append((lm, z, rotated))
    taken = [0, 0, 0]
    initial = np.empty((len(ORDER), 6))
    for e, q in enumerate(ORDER):
        initial[e] = starts[q][taken[q]]
        taken[q] += 1
    assert taken == [6, 1, 4]
    return problems, initial, [[e for e, q in enumerate(ORDER) if q == k] for k in range(3)]


def singles(nav, problems, initial, problem, mode, **kw):
    """the reference route: one nav.QuasiAscent per problem, the results put where the estimates stand"""
    n = len(initial)
    out = [np.zeros((n, 6)), np.zeros(n), np.zeros(n, np.int32), False, np.zeros((n, 6, 6))]
    problem = np.asarray(problem)
    for q, (lm, z, lin) in enumerate(problems):
        mine = np.nonzero(problem == q)[0]
        if not len(mine):
            continue
        got = nav.QuasiAscent(initial[mine], z, lm, lin, mode, **kw)
        for k in (0, 1, 2):
            out[k][mine] = got[k]
        out[3] = out[3] or got[3]
        if kw.get("hessians"):
            out[4][mine] = got[4]
    return out


def assert_same(got, want, hessians=False):
    for k, name in ((0, "poses"), (1, "values"), (2, "iterations")):
        assert np.array_equal(got[k], want[k], equal_nan=True), (name, got[k], want[k])
    assert got[3] == want[3]
    if hessians:
        assert np.array_equal(got[4], want[4], equal_nan=True)


# ---------------------------------------------------------------------------------------------- 1. whole ascents
@pytest.mark.parametrize("mode", [0, 1])
def test_interleaved_estimates_of_three_problems_equal_the_single_calls(nav, mode):
    problems, initial, _ = three(nav.params)
    assert all(abs(lin[3]) < 0.95 for _, _, lin in problems) and len({tuple(lin) for _, _, lin in problems}) == 3   # a real rotation of its own each
    want = singles(nav, problems, initial, ORDER, mode, hessians=True)
    got = nav.QuasiAscentMulti(problems, initial, ORDER, mode, hessians=True)
    print("mode %d: iterations %s" % (mode, got[2]))
    assert_same(got, want, hessians=True)
    assert not got[3] and len(set(got[2])) > 1                       # estimates stop at different iterations ...
    its, n = got[2], len(ORDER)   # ... and one that has stopped stands between two of other problems that still climb
    assert any(its[a] > its[e] < its[b] and ORDER[a] != ORDER[e] != ORDER[b] for e in range(n) for a in range(e) for b in range(e + 1, n)), its
    assert np.any(np.abs(got[0] - initial) > 1e-5)


# ---------------------------------------------------------------------------------------------- 2. edges
def with_edge(nav, edge, mode=0, **kw):
    """the normal problem of seed 21 and `edge` in one call, estimates alternating"""
    problems, initial, where = three(nav.params)
    problems = [problems[0], edge]
    initial = initial[where[0]]
    problem = [0, 1, 0, 1, 1, 0]
    want = singles(nav, problems, initial, problem, mode, **kw)
    got = nav.QuasiAscentMulti(problems, initial, problem, mode, **kw)
    assert_same(got, want, hessians=bool(kw.get("hessians")))
    return got


def test_a_problem_without_landmarks_measurements_or_both(nav):
    problems, _, _ = three(nav.params)
    lm, z, lin = problems[2]
    none = np.zeros((0, 3))
    with_edge(nav, (none, z, lin))
    got = with_edge(nav, (lm, none, lin), 1, hessians=True)
    assert np.all(got[2][[1, 3, 4]] == 1)                            # one iteration, zero gain
    with_edge(nav, (none, none, lin))


def test_a_problem_without_an_estimate_and_a_single_problem(nav):
    problems, initial, where = three(nav.params)
    mine = initial[where[0]]
    lm, z, lin = problems[0]
    want = nav.QuasiAscent(mine, z, lm, lin, 1, hessians=True)
    for table, problem in (([problems[1], problems[0], problems[2]], [1] * 6), ([problems[0]], [0] * 6)):
        got = nav.QuasiAscentMulti(table, mine, problem, 1, hessians=True)
        assert_same(got, list(want), hessians=True)
    # ... in the C call itself: problem 0 and problem 2 have no estimate
    lmoff = np.cumsum([0] + [len(p[0]) for p in problems]).astype(np.int32)
    zoff = np.cumsum([0] + [len(p[1]) for p in problems]).astype(np.int32)
    rc, out = c_ascent(nav, lmoff, np.concatenate([p[0] for p in problems]), zoff, np.concatenate([p[1] for p in problems]),
                       np.array([p[2] for p in problems]), initial[where[1]], [1], mode=1)
    single = nav.QuasiAscent(initial[where[1]], problems[1][1], problems[1][0], problems[1][2], 1)
    assert rc == 0 and np.array_equal(out[0], single[0]) and np.array_equal(out[1], single[1]) and np.array_equal(out[2], single[2])


def test_rounds_of_one_and_of_eight_iterations_give_the_same_bits(nav):
    problems, initial, _ = three(nav.params)
    a = nav.QuasiAscentMulti(problems, initial, ORDER, 1, round_iterations=1, hessians=True)
    b = nav.QuasiAscentMulti(problems, initial, ORDER, 1, round_iterations=8, hessians=True)
    assert_same(a, b, hessians=True)
    assert_same(a, singles(nav, problems, initial, ORDER, 1, hessians=True), hessians=True)


def test_iteration_bound_returns_the_state_at_the_bound(nav):
    problems, initial, _ = three(nav.params)
    want = singles(nav, problems, initial, ORDER, 1, max_iterations=1)
    assert want[3] and np.all(want[2] == 1)
    lmoff = np.cumsum([0] + [len(p[0]) for p in problems]).astype(np.int32)
    zoff = np.cumsum([0] + [len(p[1]) for p in problems]).astype(np.int32)
    rc, out = c_ascent(nav, lmoff, np.concatenate([p[0] for p in problems]), zoff, np.concatenate([p[1] for p in problems]),
                       np.array([p[2] for p in problems]), initial, ORDER, mode=1, max_iterations=1)
    assert rc == PHD_ERR_CAPACITY
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1]) and np.array_equal(out[2], want[2])
    assert_same(nav.QuasiAscentMulti(problems, initial, ORDER, 1, max_iterations=1), want)


# ---------------------------------------------------------------------------------------------- 3. the batch calls
@pytest.mark.parametrize("mode", [0, 1])
def test_batch_calls_equal_the_single_batch_calls(nav, mode):
    problems, initial, _ = three(nav.params)
    which = ORDER + [2, 0, 1]
    extra = np.random.default_rng(5).normal(0, 1, (3, 6)) * SCALE
    poses7 = np.array([pose3d_add(problems[q][2], v) for q, v in zip(which, np.concatenate([initial, extra]))])
    values = nav.QuasiSetLogLikelihoodMulti(problems, poses7, which)
    gvalues, grads = nav.QuasiSetLogLikelihoodGradientMulti(problems, poses7, which, mode)
    assert len(values) == 14 and grads.shape == (14, 6)
    which = np.asarray(which)
    for q, (lm, z, _) in enumerate(problems):
        mine = np.nonzero(which == q)[0]
        assert np.array_equal(values[mine], nav.QuasiSetLogLikelihood(z, lm, poses7[mine]))
        wv, wg = nav.QuasiSetLogLikelihoodGradient(z, lm, poses7[mine], mode)
        assert np.array_equal(gvalues[mine], wv) and np.array_equal(grads[mine], wg)
    assert np.any(grads != 0)


# ---------------------------------------------------------------------------------------------- 4. block classes
def second_class(p):
    rng = np.random.default_rng(72)
    lin, lm, z = scene(rng, p, 72, 70)
    a = (lm, z, pose3d_add(lin, ROTATE[21]))
    starts = rechart(lin, a[2], rng.normal(0, 1, (2, 6)) * SCALE)
    lin, lm, z = scene(rng, p, 100, 100, sigma=0.3)
    b = (lm, z, pose3d_add(lin, ROTATE[31]))
    last = rechart(lin, b[2], rng.normal(0, 1, (1, 6)) * SCALE)
    return [a, b], np.array([starts[0], last[0], starts[1]]), [0, 1, 0]


def test_two_problems_of_the_second_block_class(nav128):
    problems, initial, problem = second_class(nav128.params)
    assert [len(p[1]) for p in problems] == [70, 100]
    want = singles(nav128, problems, initial, problem, 1, max_iterations=3, hessians=True)   # (an association flag here would raise)
    got = nav128.QuasiAscentMulti(problems, initial, problem, 1, max_iterations=3, hessians=True)
    print("iterations %s capped %s" % (got[2], got[3]))
    assert_same(got, want, hessians=True)
    poses7 = np.array([pose3d_add(problems[q][2], v) for q, v in zip(problem, initial)])
    gv, gg = nav128.QuasiSetLogLikelihoodGradientMulti(problems, poses7, problem, 1)
    for e, q in enumerate(problem):
        wv, wg = nav128.QuasiSetLogLikelihoodGradient(problems[q][1], problems[q][0], poses7[e:e + 1], 1)
        assert gv[e] == wv[0] and np.array_equal(gg[e], wg[0])


def test_mixed_block_classes_are_refused_by_the_call_and_split_by_the_wrapper(nav128):
    big, _, _ = second_class(nav128.params)
    rng = np.random.default_rng(33)
    lin3, lm3, z3 = scene(rng, nav128.params, 4, 3)
    problems = [(lm3, z3, pose3d_add(lin3, ROTATE[61])), big[0]]
    assert [len(p[1]) for p in problems] == [3, 70]
    problem = [0, 1, 1, 0]
    identity = np.array([0, 0, 0, 1.0, 0, 0, 0])
    initial = np.array([rechart(identity, problems[q][2], [s])[0] for q, s in zip(problem, rng.normal(0, 1, (4, 6)) * SCALE)])
    lmoff = np.cumsum([0] + [len(p[0]) for p in problems]).astype(np.int32)
    zoff = np.cumsum([0] + [len(p[1]) for p in problems]).astype(np.int32)
    rc, out = c_ascent(nav128, lmoff, np.concatenate([p[0] for p in problems]), zoff, np.concatenate([p[1] for p in problems]),
                       np.array([p[2] for p in problems]), initial, problem, mode=1, max_iterations=3)
    assert rc == PHD_ERR_BAD_ARGUMENT and all(np.all(a == 7) for a in out)
    want = singles(nav128, problems, initial, problem, 1, max_iterations=3)
    assert_same(nav128.QuasiAscentMulti(problems, initial, problem, 1, max_iterations=3), want)


# ---------------------------------------------------------------------------------------------- 5. refusals
def c_ascent(nav, lmoff, lm, zoff, z, lins, initial, problem, mode=0, max_iterations=100, rounds=0, nproblems=None):
    """the C call as given, outputs pre-filled with 7: (status, (poses, values, iterations, hessians))"""
    d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_lib.dp)
    lmoff, zoff, problem = np.ascontiguousarray(lmoff, np.int32), np.ascontiguousarray(zoff, np.int32), np.ascontiguousarray(problem, np.int32)
    keep = [np.ascontiguousarray(a, np.float64) for a in (lm, z, lins, initial)]
    n = len(problem)
    out = (np.full((n, 6), 7.0), np.full(n, 7.0), np.full(n, 7, np.int32), np.full((n, 6, 6), 7.0))
    rc = nav._lib.phd_quasi_ascent_multi(nav._h, len(lmoff) - 1 if nproblems is None else nproblems, lmoff.ctypes.data_as(_lib.ip), d(keep[0]),
                                         zoff.ctypes.data_as(_lib.ip), d(keep[1]), d(keep[2]), d(keep[3]), problem.ctypes.data_as(_lib.ip), n,
                                         mode, max_iterations, rounds, d(out[0]), d(out[1]), out[2].ctypes.data_as(_lib.ip), d(out[3]))
    return rc, out


def test_refusals_leave_the_outputs_untouched(nav):
    problems, initial, where = three(nav.params)
    problems, initial, problem = problems[:2], initial[:4], [0, 1, 0, 0]
    lm, z, lins = np.concatenate([p[0] for p in problems]), np.concatenate([p[1] for p in problems]), np.array([p[2] for p in problems])
    lmoff, zoff = [0, 10, 16], [0, 7, 12]
    good = dict(lmoff=lmoff, lm=lm, zoff=zoff, z=z, lins=lins, initial=initial, problem=problem)
    rc, _ = c_ascent(nav, **good)
    assert rc == 0                                                   # the case every refusal below differs from in one thing

    def nan_in(a):
        a = np.array(a, float)
        a.flat[a.size // 2] = np.nan
        return a
    many = np.random.default_rng(6).normal(0, 1, (17, 6)) * SCALE
    wide = np.zeros((641, 3))                                        # one landmark more than the scratch of max_quantity 600 holds
    wide[:, 2] = 1.0
    cases = {"offsets decrease": dict(lmoff=[0, 12, 10]), "measurement offsets decrease": dict(zoff=[0, 8, 7]),
             "offsets do not start at 0": dict(lmoff=[1, 10, 16]), "measurement offsets do not start at 0": dict(zoff=[2, 7, 12]),
             "problem -1": dict(problem=[0, -1, 0, 0]), "problem nproblems": dict(problem=[0, 2, 0, 0]),
             "J beyond the scratch": dict(lmoff=[0, 641, 647], lm=np.concatenate([wide, problems[1][0]])),
             "17 estimates": dict(initial=many, problem=[0] * 17),
             "NaN landmark": dict(lm=nan_in(lm)), "NaN measurement": dict(z=nan_in(z)), "NaN linearisation pose": dict(lins=nan_in(lins)),
             "NaN start": dict(initial=nan_in(initial)), "average_mode 2": dict(mode=2),
             "max_iterations 0": dict(max_iterations=0), "round_iterations -1": dict(rounds=-1), "no problem": dict(nproblems=0),
             "17 measurements": dict(zoff=[0, 7, 24], z=np.concatenate([z, np.ones((12, 3))]))}
    for name, change in cases.items():
        rc, out = c_ascent(nav, **dict(good, **change))
        assert rc == PHD_ERR_BAD_ARGUMENT, name
        assert all(np.all(a == 7) for a in out), name
    d = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(_lib.dp)
    i = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(_lib.ip)
    poses7 = np.array([pose3d_add(lins[q], v) for q, v in zip(problem, initial)])
    for name, change in (("problem nproblems", dict(problem=[0, 2, 0, 0])), ("NaN pose", dict(poses=nan_in(poses7))), ("offsets decrease", dict(zoff=[0, 8, 7])),
                         ("average_mode 2", dict(mode=2))):
        a = dict(dict(lmoff=lmoff, zoff=zoff, problem=problem, poses=poses7, mode=0), **change)
        out, grad = np.full(4, 7.0), np.full((4, 6), 7.0)
        rc = nav._lib.phd_quasi_set_loglik_multi(nav._h, 2, i(a["lmoff"]), d(lm), i(a["zoff"]), d(z), d(a["poses"]), i(a["problem"]), 4, a["mode"], d(out), d(grad))
        assert rc == PHD_ERR_BAD_ARGUMENT and np.all(out == 7) and np.all(grad == 7), name
    with pytest.raises(PHDError) as e:
        nav.QuasiAscentMulti(problems, initial, problem, 2)
    assert e.value.status == PHD_ERR_BAD_ARGUMENT


# ---------------------------------------------------------------------------------------------- 6. nothing else moves
def test_the_step_and_the_single_calls_are_as_without_a_multi_call(nav):
    from monorfs_amd import navigator
    problems, initial, where = three(nav.params)
    lm, z, lin = problems[0]
    poses7 = np.array([pose3d_add(lin, s) for s in initial[where[0]]])
    before = nav.QuasiSetLogLikelihood(z, lm, poses7)
    beforeg = nav.QuasiSetLogLikelihoodGradient(z, lm, poses7, 1)
    beforea = nav.QuasiAscent(initial[where[0]], z, lm, lin, 1, hessians=True)
    f = Frame(8, 40, 12, 81, weight_profile="steady")
    other = navigator.PHDNavigator(params(), particlecount=8)
    try:
        weights = []
        for handle, multi in ((nav, True), (other, False)):
            handle.upload_state(f.planes(), f.counts, f.poses, f.weights)
            handle.SlamUpdate(None, f.z, u_resample=0.3)
            if multi:
                handle.QuasiAscentMulti(problems, initial, ORDER, 1, hessians=True)
                handle.QuasiSetLogLikelihoodGradientMulti(problems, poses7, [0] * len(poses7), 1)
            handle.SlamUpdate(None, f.z, u_resample=0.6)
            weights.append(handle.VehicleWeights.copy())
        assert np.array_equal(weights[0], weights[1]) and len(weights[0]) == 8
    finally:
        other.close()
        nav.reset(np.array([0, 0, 0, 1.0, 0, 0, 0]), (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3))), 1)
    assert np.array_equal(nav.QuasiSetLogLikelihood(z, lm, poses7), before)
    afterg = nav.QuasiSetLogLikelihoodGradient(z, lm, poses7, 1)
    assert np.array_equal(afterg[0], beforeg[0]) and np.array_equal(afterg[1], beforeg[1])
    assert_same(nav.QuasiAscent(initial[where[0]], z, lm, lin, 1, hessians=True), beforea, hessians=True)


# ---------------------------------------------------------------------------------------------- 7. the fits
def same_fit(got, want):
    (empty, comps), (wempty, wcomps) = got, want
    assert empty == wempty and len(comps) == len(wcomps), (empty, wempty, len(comps), len(wcomps))
    for (w, m, c), (ww, wm, wc) in zip(comps, wcomps):
        assert w == ww and np.array_equal(m, wm) and np.array_equal(c, wc)


def test_guided_fit_mixtures_equal_the_per_frame_fits(nav):
    pose0s, zs, models, lins = frames(nav.params)
    got = loopy.GuidedFitMixtures(nav, pose0s, zs, models, lins, 1)
    assert len(got) == 3 and len(got[0][1]) >= 1
    for i in range(3):
        same_fit(got[i], loopy.GuidedFitMixture(nav, pose0s[i], zs[i], models[i], lins[i], 1, resident=True))


def test_map_message_mixtures_equal_filter_missing_and_the_per_frame_fit():
    from monorfs_amd import navigator
    rng = np.random.default_rng(41)
    f = Frame(1, 40, 12, 41, weight_profile="steady")
    trajectory, factors = [], []
    for t in range(4):   # as tests/test_gpu_leave_one_out.py builds its trajectories
        pose = pose3d_add(f.poses[0], rng.normal(0, 1, 6) * [3e-3, 3e-3, 3e-3, 1e-3, 1e-3, 1e-3])
        zt = f.z + rng.normal(0, 1, f.z.shape) * [0.5, 0.5, 0.01]
        trajectory.append((0.1 * t, pose))
        factors.append((0.1 * t, zt))
    factors[2] = (factors[2][0], np.zeros((0, 3)))
    pose0s = [rng.normal(0, 1, 6) * [3e-3, 3e-3, 3e-3, 1e-3, 1e-3, 1e-3] for _ in range(4)]
    lins = [trajectory[t][1] for t in range(4)]
    handle = navigator.PHDNavigator(params(), particlecount=1)
    try:
        got = loopy.MapMessageMixtures(handle, trajectory, factors, pose0s, lins, average_mode=1)
        assert len(got) == 4 and got[2] == (0.0, [])
        for t in (0, 1, 3):
            model = loopy.FilterMissing(handle, trajectory, factors, t, 4)
            same_fit(got[t], loopy.GuidedFitMixture(handle, pose0s[t], factors[t][1], model, lins[t], 1, resident=True))
    finally:
        handle.close()


# ---------------------------------------------------------------------------------------------- 8. the C++ host mirror
def test_cpp_mirror_matches_the_python_host(nav, tmp_path):
    """monorfs_amd/host/PHDNavigator.hpp::QuasiAscentMulti and Loopy.hpp::GuidedFitMixtures (tests/ascent_multi_check.cpp) against
    the Python host: the same device calls behind both"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = _lib.build()
    exe = str(tmp_path / "ascent_multi_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(root, "tests", "ascent_multi_check.cpp"), so,
                           "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    problems, initial, where = three(nav.params)
    problems = [problems[0], problems[2]]
    initial = np.concatenate([initial[where[0]][:3], initial[where[2]][:2]])[[0, 3, 1, 4, 2]]
    problem = [0, 1, 0, 1, 0]
    path = tmp_path / "scene.txt"
    num = lambda a: " ".join("%.17g" % v for v in np.asarray(a, float).ravel())
    with open(path, "w") as fh:
        fh.write("%d %d\n" % (len(problems), len(initial)))
        for lm, z, lin in problems:
            fh.write("%d %d\n%s\n%s\n%s\n" % (len(lm), len(z), num(lm), num(z), num(lin)))
        fh.write("%s\n%s\n" % (" ".join(str(q) for q in problem), num(initial)))
    models = [(np.full(len(lm), 1.0001), lm, np.broadcast_to(1e-4 * np.eye(3), (len(lm), 3, 3))) for lm, _, _ in problems]
    for mode in (0, 1):
        r = subprocess.run([exe, str(path), str(mode)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        rows = [ln.split() for ln in r.stdout.splitlines()]
        table = lambda tag: np.array([[float(v) for v in row[1:]] for row in rows if row[0] == tag])
        poses, values, iters, capped = nav.QuasiAscentMulti(problems, initial, problem, mode)
        asc = table("ascent")
        assert not capped and np.all(iters >= 1)
        assert np.allclose(asc[:, 0], values, rtol=0, atol=1e-12) and np.allclose(asc[:, 1:], poses, rtol=0, atol=1e-13)
        fits = loopy.GuidedFitMixtures(nav, [np.zeros(6)] * 2, [p[1] for p in problems], models, [p[2] for p in problems], mode)
        fit = table("fit")          # frame, components, emptyspace
        assert [int(v) for v in fit[:, 1]] == [len(c) for _, c in fits]
        assert np.allclose(fit[:, 2], [e for e, _ in fits], rtol=0, atol=1e-12)
        means = table("fitmean")    # frame, component, mean[6]
        want = np.array([[k, j] + list(m) for k, (_, comps) in enumerate(fits) for j, (_, m, _) in enumerate(comps)])
        assert means.shape == want.shape and np.allclose(means, want, rtol=0, atol=1e-13)
