"""phd_quasi_guesses_multi on the device: the guess loop of GuidedFitMixture (LoopyPHDNavigator.cs:789-797) for many problems in
one call against the numpy host route (loopy.fit_to_measurement / pose3d_subtract / pose3d_add, pinned by
tests/test_loopy_host.py) — the lists and their order exactly, the guesses within a derived bound, the first values bit for bit
the batch call's —, the tile edges, empty problems, a non-finite fit, the chunked evaluation, the capacity rule, the refusals,
that nothing else of the handle moves, the whole fits through it, and the C++ host mirror.

The bound on guesses6 (derived, not tuned). Location entries: |delta| <= 1e-12 max(1, largest |coordinate| of the problem) —
about 50 roundings of 1.1e-16 give 1e-14 relative, the bound is 100 times that. Rotation entries go through acos(w) at w near
1: with dw = 16 * 2^-53 and phi the host's angle for that guess (the value of its acos: half the norm of the rotation entries),
|delta| <= 2 min(dw / sin phi, sqrt(2 dw)) + 1e-12.

Every comparison case first asserts, on the CPU, that no pair of its input has |d|^2 within relative 1e-6 of radius^2: the
host alone decides every pair of these inputs."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from loopy_stub import scene
from monorfs_amd import _lib, loopy
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, PHD_ERR_CAPACITY, prm3d_defaults
from monorfs_amd.navigator import pose3d_add
from monorfs_amd.synth import Frame
from test_ascent_multi_abi import frames
from test_gpu_ascent_multi import ROTATE, SCALE, same_fit, three

IDENTITY = np.array([0, 0, 0, 1.0, 0, 0, 0])
FAR = pose3d_add(IDENTITY, np.full(6, 1e5))
DW = 16 * 2.0 ** -53
WORST = {"location": 0.0, "rotation": 0.0}   # the largest observed errors, in units of their bounds (printed by the cases)


def params(max_particles=256, max_measurements=16):
    return prm3d_defaults(max_particles=max_particles, max_components=600, max_measurements=max_measurements)


@pytest.fixture(scope="module")
def nav():
    from monorfs_amd import navigator
    n = navigator.PHDNavigator(params(), particlecount=1)
    yield n
    n.close()


@pytest.fixture(scope="module")
def nav64():
    from monorfs_amd import navigator
    n = navigator.PHDNavigator(params(max_particles=64), particlecount=1)
    yield n
    n.close()


@pytest.fixture(scope="module")
def nav128():
    from monorfs_amd import navigator
    n = navigator.PHDNavigator(params(max_measurements=128), particlecount=1)
    yield n
    n.close()


# ---------------------------------------------------------------------------------------------- the inputs and the host route
def problem_of(seed, J, M, sigma=1.0, rotate=None):
    """a scene of J landmarks and M measurements, its linearisation pose moved and rotated by `rotate`; pose0 is a pose near the
    scene's restated in that chart (as tests/test_gpu_ascent_multi.py::three restates its starts), so the initial pose is where
    the measurements were taken and a good part of the pairs pass"""
    rng = np.random.default_rng(seed)
    lin, lm, z = scene(rng, params(), J, M, sigma=sigma)
    rotated = pose3d_add(lin, ROTATE[21] if rotate is None else rotate)
    return (lm, z, rotated), loopy.pose3d_subtract(pose3d_add(lin, rng.normal(0, 1, 6) * SCALE), rotated)


@functools.lru_cache(maxsize=None)
def case(name):
    """(problems, pose0s) of a named input, made once"""
    if name == "three":      # J x M = 6 x 5, 3 x 2, 40 x 12, a rotated linearisation pose of its own each
        made = [problem_of(31, 6, 5, 0.3, ROTATE[31]), problem_of(61, 3, 2, 1.0, ROTATE[61]), problem_of(1064, 40, 12, 1.0, ROTATE[21])]
    elif name.startswith("edge"):
        J, M = {"edge1": (1, 1), "edge255": (17, 15), "edge256": (16, 16), "edge257": (257, 1), "edge9600": (600, 16)}[name]
        made = [problem_of(500 + J, J, M)]
    elif name == "empty":    # no landmarks, no measurements, neither: each between two problems that have both
        (lm, z, lin), p0 = problem_of(92, 5, 4, 0.3, ROTATE[31])
        none = np.zeros((0, 3))
        made = [problem_of(91, 6, 5, 0.3), ((none, z, lin), p0), problem_of(31, 6, 5, 0.3, ROTATE[31]), ((lm, none, lin), p0),
                problem_of(61, 3, 2, 1.0, ROTATE[61]), ((none, none, lin), p0), problem_of(92, 3, 2, 0.3)]
    elif name == "at the pose":   # pose0 = 0, an identity-rotation linearisation pose, one landmark exactly at its location
        rng = np.random.default_rng(77)
        lin, lm, z = scene(rng, params(), 7, 4, sigma=0.3)
        lin = np.array([0.05, -0.02, 0.03, 1.0, 0, 0, 0])
        lm = lm + lin[:3]
        lm[3] = lin[:3]
        made = [((lm, z, lin), np.zeros(6))]
    elif name == "many":     # more than 128 guesses at radius 1e3
        made = [problem_of(1064, 40, 12, 1.0, ROTATE[21])]
    else:
        raise KeyError(name)
    return [m[0] for m in made], [m[1] for m in made]


@functools.lru_cache(maxsize=None)
def fits(name):
    """the host's fit of every pair of a case, once: per problem (d2[J M], guess6[J M][6]) in landmark-major order"""
    problems, pose0s = case(name)
    p = params()
    out = []
    for (lm, z, lin), pose0 in zip(problems, pose0s):
        initpose = pose3d_add(lin, pose0)
        d2, g6 = np.empty(len(lm) * len(z)), np.empty((len(lm) * len(z), 6))
        with np.errstate(invalid="ignore", divide="ignore"):
            for j, landmark in enumerate(lm):
                for m, measurement in enumerate(z):
                    guess = loopy.fit_to_measurement(p, initpose, measurement, landmark)
                    d = loopy.pose3d_subtract(guess, initpose)
                    d2[j * len(z) + m] = float(np.dot(d, d))
                    g6[j * len(z) + m] = loopy.pose3d_subtract(guess, lin)
        out.append((d2, g6))
    return out


def host_lists(name, radius):
    """The precondition, then the host's lists: per problem (pairs[n][2], guesses6[n][6]), pose0 first"""
    problems, pose0s = case(name)
    out = []
    for ((lm, z, _), pose0, (d2, g6)) in zip(problems, pose0s, fits(name)):
        finite = d2[np.isfinite(d2)]
        margin = np.min(np.abs(finite / (radius * radius) - 1.0)) if len(finite) else np.inf
        assert margin > 1e-6, (name, radius, margin)     # the host alone decides every pair
        keep = np.nonzero(d2 < radius * radius)[0]       # (false on NaN)
        M = max(len(z), 1)
        pairs = np.array([(-1, -1)] + [(i // M, i % M) for i in keep], np.int32).reshape(-1, 2)
        out.append((pairs, np.concatenate([pose0.reshape(1, 6), g6[keep]])))
    return out


def assert_within_bound(got6, want6, problem, what):
    lm, _, lin = problem
    scale = max(1.0, float(np.max(np.abs(lm))) if len(lm) else 0.0, float(np.max(np.abs(lin[:3]))))
    loc = np.abs(got6[:, :3] - want6[:, :3])
    phi = 0.5 * np.linalg.norm(want6[:, 3:], axis=1)
    with np.errstate(divide="ignore"):
        rb = 2 * np.minimum(DW / np.sin(phi), math.sqrt(2 * DW)) + 1e-12
    rot = np.abs(got6[:, 3:] - want6[:, 3:])
    WORST["location"] = max(WORST["location"], float(loc.max()))
    WORST["rotation"] = max(WORST["rotation"], float(rot.max()))
    print("%s: %d guesses, largest location error %.3g (bound %.3g), largest rotation error %.3g (smallest bound %.3g)"
          % (what, len(got6), loc.max(), 1e-12 * scale, rot.max(), rb.min()))
    assert np.all(loc <= 1e-12 * scale), (what, loc.max())
    assert np.all(rot <= rb[:, None]), (what, rot.max(), rb.min())


def batch_values(nav, problems, poses7, which):
    """QuasiSetLogLikelihoodMulti (it chunks by max_particles itself)"""
    return nav.QuasiSetLogLikelihoodMulti(problems, poses7, which) if len(poses7) else np.zeros(0)


def check_call(nav, name, radius, compare_guesses=True):
    """one call over the problems of a case against the host route: everything the issue lists. Returns the call's results."""
    problems, pose0s = case(name)
    want = host_lists(name, radius)
    off, pairs, g6, p7, values, empties = nav.QuasiGuessesMulti(problems, pose0s, radius)
    assert off[0] == 0 and list(np.diff(off)) == [len(w[0]) for w in want], (name, list(np.diff(off)), [len(w[0]) for w in want])
    assert np.array_equal(pairs, np.concatenate([w[0] for w in want]))
    which = np.repeat(np.arange(len(problems)), np.diff(off))
    for q, (problem, pose0) in enumerate(zip(problems, pose0s)):
        mine = slice(off[q], off[q + 1])
        assert np.array_equal(g6[mine][0], pose0)                         # pose0 itself, bits
        if compare_guesses:
            assert_within_bound(g6[mine], want[q][1], problem, "%s[%d] radius %g" % (name, q, radius))
        added = np.array([pose3d_add(problem[2], g) for g in g6[mine]])
        assert np.max(np.abs(p7[mine] - added)) <= 1e-14
    assert np.array_equal(values, batch_values(nav, problems, p7, which))
    assert np.array_equal(empties, batch_values(nav, problems, np.tile(FAR, (len(problems), 1)), np.arange(len(problems))))
    return off, pairs, g6, p7, values, empties


# ---------------------------------------------------------------------------------------------- 1. against the host route
def test_three_problems_in_one_call_equal_the_host_lists(nav):
    problems, _ = case("three")
    assert [(len(p[0]), len(p[1])) for p in problems] == [(6, 5), (3, 2), (40, 12)]
    assert all(abs(p[2][3]) < 0.95 for p in problems) and len({tuple(p[2]) for p in problems}) == 3
    off, pairs, _, _, values, _ = check_call(nav, "three", 0.5)
    print("guesses per problem %s" % list(np.diff(off)))
    assert off[3] > 3 and off[3] < 3 + 30 + 6 + 480                       # some pairs pass, some do not
    assert np.all(np.isfinite(values))


@pytest.mark.parametrize("name", ["edge1", "edge255", "edge256", "edge257", "edge9600"])
def test_tile_edges_every_pair_and_none(nav, name):
    problems, _ = case(name)
    J, M = len(problems[0][0]), len(problems[0][1])
    off, pairs, _, _, _, _ = check_call(nav, name, 1e3)
    assert off[1] == 1 + J * M                                            # every pair passes ...
    assert np.array_equal(pairs[1:], np.array([(j, m) for j in range(J) for m in range(M)], np.int32))   # ... landmark-major
    off, pairs, _, _, _, _ = check_call(nav, name, 1e-9)
    assert list(off) == [0, 1] and np.array_equal(pairs, [[-1, -1]])      # only pose0 remains


def test_empty_problems_yield_the_pose0_guess_alone(nav):
    problems, _ = case("empty")
    assert [(len(p[0]) > 0, len(p[1]) > 0) for p in problems] == [(True, True), (False, True), (True, True), (True, False), (True, True), (False, False), (True, True)]
    off, pairs, _, _, _, _ = check_call(nav, "empty", 0.5)
    for q in (1, 3, 5):
        assert off[q + 1] - off[q] == 1 and np.array_equal(pairs[off[q]], [-1, -1])
    assert all(off[q + 1] - off[q] > 1 for q in (0, 2, 4, 6))


def test_a_landmark_at_the_pose_makes_no_guess(nav):
    (problem,), (pose0,) = case("at the pose")
    lm, z, lin = problem
    assert not np.any(pose0) and np.array_equal(lin[3:], [1, 0, 0, 0]) and np.array_equal(lm[3], lin[:3])
    d2, _ = fits("at the pose")[0]
    assert np.all(np.isnan(d2[3 * len(z):4 * len(z)])) and np.all(np.isfinite(np.delete(d2, range(3 * len(z), 4 * len(z)))))
    off, pairs, _, _, values, _ = check_call(nav, "at the pose", 1e3)
    assert off[1] == 1 + 6 * len(z) and 3 not in pairs[:, 0]              # the pairs behind it keep their places (check_call: and values)
    assert np.all(np.isfinite(values))


def test_values_of_a_chunked_evaluation_equal_the_batch_call_in_chunks(nav64, nav):
    problems, pose0s = case("many")
    off, pairs, g6, p7, values, empties = check_call(nav64, "many", 1e3)
    assert nav64.params.max_particles == 64 and off[1] > 128
    whole = nav.QuasiGuessesMulti(problems, pose0s, 1e3)                   # (256 poses a launch there: the chunking does not show)
    for a, b in zip((off, pairs, g6, p7, values, empties), whole):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- 2. the C call: capacity, refusals
def c_guesses(nav, problems, pose0s, radius=0.5, capacity=None, handle=True, null=(), **change):
    """the C call as given, outputs pre-filled with 7: (status, (guess_offsets, pairs2, guesses6, poses7, values, emptyspace))"""
    a = dict(lmoff=np.cumsum([0] + [len(p[0]) for p in problems]), lm=np.concatenate([p[0] for p in problems] + [np.zeros((0, 3))]),
             zoff=np.cumsum([0] + [len(p[1]) for p in problems]), z=np.concatenate([p[1] for p in problems] + [np.zeros((0, 3))]),
             lins=np.array([p[2] for p in problems]), start=np.array(pose0s), far=FAR, nproblems=len(problems))
    a.update(change)
    np_ = len(problems)
    cap = 1 + np_ + sum(len(p[0]) * len(p[1]) for p in problems) if capacity is None else capacity
    room = max(cap, 1)
    out = dict(goff=np.full(np_ + 1, 7, np.int32), pairs=np.full((room, 2), 7, np.int32), g6=np.full((room, 6), 7.0), p7=np.full((room, 7), 7.0),
               values=np.full(room, 7.0), empty=np.full(np_, 7.0))
    keep = {k: np.ascontiguousarray(a[k], np.float64) for k in ("lm", "z", "lins", "start", "far")}
    keep.update({k: np.ascontiguousarray(a[k], np.int32) for k in ("lmoff", "zoff")})
    d = lambda k: None if k in null else keep[k].ctypes.data_as(_lib.dp)
    i = lambda k: None if k in null else keep[k].ctypes.data_as(_lib.ip)
    od = lambda k: None if k in null else out[k].ctypes.data_as(_lib.dp)
    oi = lambda k: None if k in null else out[k].ctypes.data_as(_lib.ip)
    rc = nav._lib.phd_quasi_guesses_multi(nav._h if handle else None, a["nproblems"], i("lmoff"), d("lm"), i("zoff"), d("z"), d("lins"), d("start"), d("far"),
                                          float(radius), cap, oi("goff"), oi("pairs"), od("g6"), od("p7"), od("values"), od("empty"))
    return rc, tuple(out[k] for k in ("goff", "pairs", "g6", "p7", "values", "empty"))


def test_capacity_rule(nav):
    problems, pose0s = case("three")
    off, pairs, g6, p7, values, empties = nav.QuasiGuessesMulti(problems, pose0s, 0.5)
    total = int(off[-1])
    rc, out = c_guesses(nav, problems, pose0s, capacity=total)            # exactly the total: succeeds
    assert rc == 0
    for got, want in zip(out, (off, pairs, g6, p7, values, empties)):
        assert np.array_equal(got[:len(want)], want)
    rc, out = c_guesses(nav, problems, pose0s, capacity=total - 1)        # one less: the offsets, nothing else
    assert rc == PHD_ERR_CAPACITY
    assert np.array_equal(out[0], off) and all(np.all(a == 7) for a in out[1:])
    rc, out = c_guesses(nav, problems, pose0s, capacity=2)                # below one guess per problem: a refusal
    assert rc == PHD_ERR_BAD_ARGUMENT and all(np.all(a == 7) for a in out)


def test_refusals_leave_the_outputs_untouched(nav, nav128):
    problems, pose0s = case("three")
    problems, pose0s = problems[:2], pose0s[:2]
    rc, _ = c_guesses(nav, problems, pose0s)
    assert rc == 0                                                        # the case every refusal below differs from in one thing

    def nan_in(a, value=np.nan):
        a = np.array(a, float)
        a.flat[a.size // 2] = value
        return a
    lm, z = np.concatenate([p[0] for p in problems]), np.concatenate([p[1] for p in problems])
    lins = np.array([p[2] for p in problems])
    wide = np.zeros((641, 3))                                             # one landmark more than the scratch of max_quantity 600 holds
    wide[:, 2] = 1.0
    cases = {"no handle": dict(handle=False), "no problem": dict(nproblems=0),
             "offsets decrease": dict(lmoff=[0, 8, 6]), "measurement offsets decrease": dict(zoff=[0, 6, 5]),
             "offsets do not start at 0": dict(lmoff=[1, 6, 9]), "measurement offsets do not start at 0": dict(zoff=[2, 5, 7]),
             "J beyond the scratch": dict(lmoff=[0, 641, 644], lm=np.concatenate([wide, problems[1][0]])),
             "17 measurements": dict(zoff=[0, 5, 22], z=np.concatenate([z, np.ones((15, 3))])),
             "NaN landmark": dict(lm=nan_in(lm)), "NaN measurement": dict(z=nan_in(z)), "infinite measurement": dict(z=nan_in(z, np.inf)),
             "NaN linearisation pose": dict(lins=nan_in(lins)), "NaN pose0": dict(start=nan_in(pose0s)), "NaN far pose": dict(far=nan_in(FAR)),
             "radius 0": dict(radius=0.0), "radius negative": dict(radius=-0.5), "radius NaN": dict(radius=np.nan), "radius infinite": dict(radius=np.inf),
             "capacity below the problems": dict(capacity=1)}
    for k in ("lmoff", "lm", "zoff", "z", "lins", "start", "far", "goff", "pairs", "g6", "p7", "values", "empty"):
        cases["NULL " + k] = dict(null=(k,))
    for name, change in cases.items():
        rc, out = c_guesses(nav, problems, pose0s, **change)
        assert rc == PHD_ERR_BAD_ARGUMENT, name
        assert all(np.all(a == 7) for a in out), name
    # mixed block classes, on a handle that takes 70 measurements
    rng = np.random.default_rng(72)
    lin, lm70, z70 = scene(rng, nav128.params, 72, 70)                     # (a scene measures its first landmarks: M <= J)
    mixed = [problems[0], (lm70, z70, pose3d_add(lin, ROTATE[21]))]
    rc, out = c_guesses(nav128, mixed, pose0s)
    assert rc == PHD_ERR_BAD_ARGUMENT and all(np.all(a == 7) for a in out)
    got = nav128.QuasiGuessesMulti(mixed, pose0s, 0.5)                    # ... and split by the wrapper, in the caller's order
    for q in (0, 1):
        alone = nav128.QuasiGuessesMulti([mixed[q]], [pose0s[q]], 0.5)
        mine = slice(got[0][q], got[0][q + 1])
        assert all(np.array_equal(got[k][mine], alone[k]) for k in (1, 2, 3, 4)) and got[5][q] == alone[5][0]


# ---------------------------------------------------------------------------------------------- 3. nothing else moves
def test_the_step_and_the_other_calls_are_as_without_a_guesses_call(nav):
    from monorfs_amd import navigator
    problems, initial, where = three(nav.params)
    order = [0, 2, 0, 1, 2, 0, 2, 0, 2, 0, 0]
    lm, z, lin = problems[0]
    gproblems, gpose0s = case("three")
    beforea = nav.QuasiAscent(initial[where[0]], z, lm, lin, 1, hessians=True)
    beforem = nav.QuasiAscentMulti(problems, initial, order, 1, hessians=True)
    f = Frame(8, 40, 12, 81, weight_profile="steady")
    other = navigator.PHDNavigator(params(), particlecount=8)
    try:
        weights = []
        for handle, guesses in ((nav, True), (other, False)):
            handle.upload_state(f.planes(), f.counts, f.poses, f.weights)
            handle.SlamUpdate(None, f.z, u_resample=0.3)
            if guesses:
                handle.QuasiGuessesMulti(gproblems, gpose0s, 0.5)
            handle.SlamUpdate(None, f.z, u_resample=0.6)
            weights.append(handle.VehicleWeights.copy())
        assert np.array_equal(weights[0], weights[1]) and len(weights[0]) == 8
    finally:
        other.close()
        nav.reset(IDENTITY, (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3))), 1)
    nav.QuasiGuessesMulti(gproblems, gpose0s, 0.5)
    aftera = nav.QuasiAscent(initial[where[0]], z, lm, lin, 1, hessians=True)
    nav.QuasiGuessesMulti(gproblems, gpose0s, 0.5)
    afterm = nav.QuasiAscentMulti(problems, initial, order, 1, hessians=True)
    for got, want in ((aftera, beforea), (afterm, beforem)):
        for k in (0, 1, 2, 4):
            assert np.array_equal(got[k], want[k], equal_nan=True)
        assert got[3] == want[3]


# ---------------------------------------------------------------------------------------------- 4. the whole fits
def frames_margin(problems, pose0s, radius=0.5):
    """the precondition for frames that are not a named case"""
    p = params()
    for (lm, z, lin), pose0 in zip(problems, pose0s):
        initpose = pose3d_add(lin, pose0)
        for landmark in lm:
            for measurement in z:
                d = loopy.pose3d_subtract(loopy.fit_to_measurement(p, initpose, measurement, landmark), initpose)
                assert abs(float(np.dot(d, d)) / (radius * radius) - 1.0) > 1e-6


def test_guided_fit_mixtures_with_device_guesses(nav):
    pose0s, zs, models, lins = frames(nav.params)
    problems, starts = loopy._problems_of(pose0s, zs, models, lins)
    frames_margin(problems, starts)
    got = loopy.GuidedFitMixturesRouted(nav, pose0s, zs, models, lins, 1, device_guesses=True)
    # bit for bit the host pipeline fed the device's own guess lists and first values
    guesses, firsts, empties, dpairs = loopy.DeviceGuesses(nav, problems, starts)
    fed = loopy.FitMixturesFromGuesses(nav, problems, starts, guesses, firsts, empties, 1)
    assert len(got) == 3
    for i in range(3):
        same_fit(got[i], fed[i])
    # against the host route: the guess lists, then the count of components and the far pose's value
    hguesses, _, hempties, hpairs = loopy.HostGuesses(nav, problems, starts)
    assert dpairs == hpairs and [len(g) for g in guesses] == [len(g) for g in hguesses]
    for i in range(3):
        assert_within_bound(np.array(guesses[i]), np.array(hguesses[i]), problems[i], "frame %d" % i)
    host = loopy.GuidedFitMixtures(nav, pose0s, zs, models, lins, 1)
    for i in range(3):
        assert got[i][0] == host[i][0] == hempties[i] and len(got[i][1]) == len(host[i][1]) >= 1, (i, got[i][0], host[i][0], len(got[i][1]), len(host[i][1]))


def test_map_message_mixtures_with_device_guesses():
    from monorfs_amd import navigator
    rng = np.random.default_rng(41)
    f = Frame(1, 40, 12, 41, weight_profile="steady")
    trajectory, factors = [], []
    for t in range(4):   # the trajectory of tests/test_gpu_ascent_multi.py::test_map_message_mixtures_equal_filter_missing_and_the_per_frame_fit
        pose = pose3d_add(f.poses[0], rng.normal(0, 1, 6) * [3e-3, 3e-3, 3e-3, 1e-3, 1e-3, 1e-3])
        zt = f.z + rng.normal(0, 1, f.z.shape) * [0.5, 0.5, 0.01]
        trajectory.append((0.1 * t, pose))
        factors.append((0.1 * t, zt))
    factors[2] = (factors[2][0], np.zeros((0, 3)))
    pose0s = [rng.normal(0, 1, 6) * [3e-3, 3e-3, 3e-3, 1e-3, 1e-3, 1e-3] for _ in range(4)]
    lins = [trajectory[t][1] for t in range(4)]
    handle = navigator.PHDNavigator(params(), particlecount=1)
    try:
        got = loopy.MapMessageMixturesRouted(handle, trajectory, factors, pose0s, lins, average_mode=1, device_guesses=True)
        assert len(got) == 4 and got[2] == (0.0, [])
        maps, _ = loopy.LeaveOneOutMaps(handle, trajectory, factors, to=4)
        seen = [0, 1, 3]
        problems, starts = loopy._problems_of([pose0s[t] for t in seen], [factors[t][1] for t in seen], [maps[t] for t in seen], [lins[t] for t in seen])
        frames_margin(problems, starts)
        guesses, firsts, empties, dpairs = loopy.DeviceGuesses(handle, problems, starts)
        fed = loopy.FitMixturesFromGuesses(handle, problems, starts, guesses, firsts, empties, 1)
        for k, t in enumerate(seen):
            same_fit(got[t], fed[k])
        _, _, _, hpairs = loopy.HostGuesses(handle, problems, starts)
        assert dpairs == hpairs
        host = loopy.MapMessageMixtures(handle, trajectory, factors, pose0s, lins, average_mode=1)
        for t in seen:
            assert got[t][0] == host[t][0] and len(got[t][1]) == len(host[t][1]) >= 1, (t, got[t][0], host[t][0], len(got[t][1]), len(host[t][1]))
    finally:
        handle.close()


# ---------------------------------------------------------------------------------------------- 5. the C++ host mirror
def test_cpp_mirror_matches_the_python_host(nav, tmp_path):
    """monorfs_amd/host/PHDNavigator.hpp::QuasiGuessesMulti and Loopy.hpp::GuidedFitMixtures(..., device_guesses)
    (tests/guesses_check.cpp) against the Python host: the same device call behind both, the same host guess loop beside it"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = _lib.build()
    exe = str(tmp_path / "guesses_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(root, "tests", "guesses_check.cpp"), so,
                           "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    pose0s, zs, models, lins = frames(nav.params)
    problems, starts = loopy._problems_of(pose0s, zs, models, lins)
    path = tmp_path / "scene.txt"
    num = lambda a: " ".join("%.17g" % v for v in np.asarray(a, float).ravel())
    with open(path, "w") as fh:
        fh.write("%d\n" % len(problems))
        for (lm, z, lin), pose0 in zip(problems, starts):
            fh.write("%d %d\n%s\n%s\n%s\n%s\n" % (len(lm), len(z), num(lm), num(z), num(lin), num(pose0)))
    r = subprocess.run([exe, str(path), "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    table = lambda tag: np.array([[float(v) for v in row[1:]] for row in rows if row[0] == tag])
    off, pairs, g6, p7, values, empties = nav.QuasiGuessesMulti(problems, starts, 0.5)
    assert np.array_equal(table("offsets")[0], off)
    dev = table("guess")        # pair[2], guess[6], pose[7], value
    assert np.array_equal(dev[:, :2], pairs) and np.array_equal(dev[:, 2:8], g6) and np.array_equal(dev[:, 8:15], p7) and np.array_equal(dev[:, 15], values)
    assert np.array_equal(table("empty")[:, 1], empties)
    hguesses, _, _, hpairs = loopy.HostGuesses(nav, problems, starts)
    host = table("hostguess")   # frame, pair[2], guess[6]: the C++ host loop
    assert np.array_equal(host[:, 1:3], np.concatenate([np.array(p) for p in hpairs]))
    assert np.allclose(host[:, 3:], np.concatenate([np.array(g) for g in hguesses]), rtol=0, atol=1e-13)
    fits_ = loopy.GuidedFitMixturesRouted(nav, pose0s, zs, models, lins, 1, device_guesses=True)
    fit = table("fit")          # frame, components, emptyspace
    assert [int(v) for v in fit[:, 1]] == [len(c) for _, c in fits_]
    assert np.array_equal(fit[:, 2], [e for e, _ in fits_])
    means = table("fitmean")    # frame, component, mean[6]
    want = np.array([[k, j] + list(m) for k, (_, comps) in enumerate(fits_) for j, (_, m, _) in enumerate(comps)])
    assert means.shape == want.shape and np.allclose(means, want, rtol=0, atol=1e-13)
