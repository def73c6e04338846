"""phd_quasi_ascent on the device: the control kernels alone against the numpy statement of the loop's line search, whole
ascents (resident=True) against the host-driven loop of monorfs_amd/loopy.py on the same handle — both use the same evaluation
kernels —, the edges of the call, FitGaussian / GuidedFitMixture through it, and the C++ host mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from ascent_util import CountingNav, control_reference
from loopy_stub import scene
from monorfs_amd import _lib, loopy
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, PHD_ERR_CAPACITY, prm3d_defaults
from monorfs_amd.navigator import pose3d_add
from monorfs_amd.synth import Frame

SCALE = [4e-3, 4e-3, 4e-3, 2e-3, 2e-3, 2e-3]
RUNS = {21: (10, 7, 6, 1.0), 22: (10, 7, 6, 1.0), 31: (6, 5, 1, 0.3), 61: (3, 2, 4, 1.0)}   # seed: landmarks, measurements, starts, sigma


def params():
    return prm3d_defaults(max_particles=256, max_components=600, max_measurements=16)


@pytest.fixture(scope="module")
def nav():
    from monorfs_amd import navigator
    n = navigator.PHDNavigator(params(), particlecount=1)
    yield n
    n.close()


def run_scene(p, seed):
    J, M, n, sigma = RUNS[seed]
    rng = np.random.default_rng(seed)
    lin, lm, z = scene(rng, p, J, M, sigma=sigma)
    return lin, lm, z, rng.normal(0, 1, (n, 6)) * SCALE


_host = {}


def host_loop(nav, seed, mode, max_iterations=None):
    """the host-driven loop on the device's batches, once per case: (poses, values, iterations per estimate)"""
    key = (seed, mode, max_iterations)
    if key not in _host:
        lin, lm, z, starts = run_scene(nav.params, seed)
        counting = CountingNav(nav)
        poses, values = loopy.LogLikeGradientAscent(counting, starts, z, lm, lin, mode, max_iterations=max_iterations)
        _host[key] = (poses, values, counting.iterations())
        for a in _host[key]:
            a.setflags(write=False)
    return _host[key]


def d(a):
    return a.ctypes.data_as(_lib.dp)


# ---------------------------------------------------------------------------------------------- 1. the control step alone
def control_case(n, rng):
    """estimate a of n: gradient a % 4 (norm 3, exactly 10 twice, 1e4 — integer entries: the squares and their sum are exact in any
    order, so numpy's norm and the kernel's are the same number), value row a % 5 (accept at 0, accept at 7, all 16 rejected, equal
    to loglike throughout, NaN at 0) — with 16 estimates every gradient meets four of the rows"""
    grads = np.array([[1, 2, 2, 0, 0, 0], [6, 8, 0, 0, 0, 0], [0, 0, 6, 0, 0, -8], [6000, -8000, 0, 0, 0, 0]], float)
    pose6 = rng.normal(0, 1, (n, 6)) * SCALE
    loglike = rng.uniform(-30, -20, n)
    grad, values = np.empty((n, 6)), np.empty((n, 16))
    for a in range(n):
        grad[a] = grads[a % 4] if a < 8 else np.rint(rng.normal(0, 1, 6) * [3000, 3000, 3000, 2000, 2000, 2000]) if a % 4 == 3 else grads[a % 4][::-1]
        row = a % 5
        below, above = loglike[a] - rng.uniform(0.5, 2, 16), loglike[a] + rng.uniform(0.5, 2, 16)
        values[a] = [above, np.concatenate([below[:7], above[7:]]), below, np.full(16, loglike[a]), np.concatenate([[np.nan], below[1:]])][row]
    return pose6, loglike, grad, values


@pytest.mark.parametrize("n", [1, 16])
def test_control_step_against_the_numpy_statement(nav, n):
    rng = np.random.default_rng(70 + n)
    lin = pose3d_add([0.3, -0.2, 0.1, 1.0, 0, 0, 0], [0, 0, 0, 0.4, -0.7, 0.5])   # a real rotation
    assert abs(lin[3]) < 0.9
    pose6, loglike, grad, values = control_case(n, rng)
    if n == 1:
        values[0] = np.concatenate([loglike[0] - 1 - np.arange(7), loglike[0] + 1 + np.arange(9)])   # accept at 7
        grad[0] = [6000, -8000, 0, 0, 0, 0]
    cand6, cand7, newpose, newll, next7 = np.zeros((n, 16, 6)), np.zeros((n, 16, 7)), np.zeros((n, 6)), np.zeros(n), np.zeros((n, 7))
    chosen, active = np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc = nav._lib.phd_test_ascent_control(nav._h, d(pose6), d(loglike), d(grad), d(values), n, d(np.ascontiguousarray(lin)), d(cand6), d(cand7),
                                          chosen.ctypes.data_as(_lib.ip), d(newpose), d(newll), d(next7), active.ctypes.data_as(_lib.ip))
    nav._check(rc)
    w6, w7, wchosen, wpose, wll, wnext, wactive = control_reference(pose6, loglike, grad, values, lin)
    assert np.array_equal(chosen, wchosen) and np.array_equal(active, wactive), (chosen, wchosen, active, wactive)
    assert np.array_equal(cand6, w6), np.max(np.abs(cand6 - w6))
    assert np.max(np.abs(cand7 - w7)) <= 1e-14                       # device sin / cos against libm
    assert np.array_equal(newpose, wpose) and np.array_equal(newll, wll)
    assert np.array_equal(next7, cand7[np.arange(n), chosen]) and np.max(np.abs(next7 - wnext)) <= 1e-14
    if n == 16:   # every branch was there
        assert set(chosen) == {0, 7, 15} and set(active) == {0, 1}
        assert np.any(np.all(newpose == pose6, axis=1)) and np.any(np.any(newpose != pose6, axis=1))
        norms = np.linalg.norm(grad, axis=1)
        assert np.any(norms == 3) and np.any(norms == 10) and np.any(norms == 1e4)
        assert np.array_equal(cand6[1, 0], pose6[1] + 1e-2 * grad[1])   # norm exactly 10: not clipped


# ---------------------------------------------------------------------------------------------- 2. whole ascents
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("seed", sorted(RUNS))
def test_resident_ascent_against_the_host_loop(nav, seed, mode):
    lin, lm, z, starts = run_scene(nav.params, seed)
    want, wantv, wantit = host_loop(nav, seed, mode)
    got, gotv, gotit, capped = nav.QuasiAscent(starts, z, lm, lin, mode)
    print("seed %d mode %d: iterations host %s device %s, max |dv| %.3g, max |dpose| %.3g" % (seed, mode, wantit, gotit, np.max(np.abs(gotv - wantv)), np.max(np.abs(got - want))))
    assert not capped
    assert np.array_equal(gotit, wantit), (gotit, wantit)
    assert np.allclose(gotv, wantv, rtol=1e-9, atol=1e-8), np.max(np.abs(gotv - wantv))
    assert np.allclose(got, want, rtol=0, atol=1e-9), np.max(np.abs(got - want))
    if seed in (21, 22):
        assert np.any(np.abs(got - starts) > 1e-5)                  # some estimate did climb (seed 61: every line search is rejected)
    viaflag, viaflagv = loopy.LogLikeGradientAscent(nav, starts, z, lm, lin, mode, resident=True)
    assert np.array_equal(viaflag, got) and np.array_equal(viaflagv, gotv)


def test_estimates_stop_at_different_iterations(nav):
    counts = host_loop(nav, 21, 1)[2]
    assert len(set(counts)) >= 3 and min(counts) >= 1


# ---------------------------------------------------------------------------------------------- 3. edges
def both_rounds(nav, starts, z, lm, lin, mode, **kw):
    """the call with rounds of 1 and of 8 iterations: the same bits"""
    a = nav.QuasiAscent(starts, z, lm, lin, mode, round_iterations=1, **kw)
    b = nav.QuasiAscent(starts, z, lm, lin, mode, round_iterations=8, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)
    return a


def against_host(nav, starts, z, lm, lin, mode, max_iterations=None):
    counting = CountingNav(nav)
    want, wantv = loopy.LogLikeGradientAscent(counting, starts, z, lm, lin, mode, max_iterations=max_iterations)
    got = both_rounds(nav, starts, z, lm, lin, mode, **({} if max_iterations is None else {"max_iterations": max_iterations}))
    assert np.array_equal(got[2], counting.iterations()), (got[2], counting.iterations())
    assert np.allclose(got[1], wantv, rtol=1e-9, atol=1e-8) and np.allclose(got[0], want, rtol=0, atol=1e-9)
    return got


def test_no_landmarks_and_no_measurements(nav):
    lin, lm, z, starts = run_scene(nav.params, 61)
    against_host(nav, starts, z, np.zeros((0, 3)), lin, 0)
    got = against_host(nav, starts, np.zeros((0, 3)), lm, lin, 1)
    assert np.all(got[2] == 1) and np.array_equal(got[0], starts)    # one iteration, zero gain
    against_host(nav, starts, np.zeros((0, 3)), np.zeros((0, 3)), lin, 0)


def test_iteration_bound_returns_the_state_at_the_bound(nav):
    lin, lm, z, starts = run_scene(nav.params, 21)
    want, wantv, wantit = host_loop(nav, 21, 1, 1)
    assert np.all(wantit == 1)
    poses, values, iters = np.zeros((6, 6)), np.zeros(6), np.zeros(6, np.int32)
    rc = nav._lib.phd_quasi_ascent(nav._h, d(np.ascontiguousarray(starts)), 6, d(np.ascontiguousarray(lin)), d(np.ascontiguousarray(lm)), len(lm),
                                   d(np.ascontiguousarray(z)), len(z), 1, 1, 0, d(poses), d(values), iters.ctypes.data_as(_lib.ip), None)
    assert rc == PHD_ERR_CAPACITY
    assert np.all(iters == 1) and np.allclose(values, wantv, rtol=1e-9, atol=1e-8) and np.allclose(poses, want, rtol=0, atol=1e-9)
    got = against_host(nav, starts, z, lm, lin, 1, max_iterations=1)
    assert got[3] and np.array_equal(got[0], poses) and np.array_equal(got[1], values)
    full = host_loop(nav, 21, 1)
    for k in (2, 4):   # the bound is reached by some, by none
        got = against_host(nav, starts, z, lm, lin, 1, max_iterations=k)
        assert got[3] == bool(np.any(full[2] > k)) and np.array_equal(got[2], np.minimum(full[2], k))
    with pytest.raises(RuntimeError):
        bound, loopy.ResidentIterationBound = loopy.ResidentIterationBound, 1
        try:
            loopy.LogLikeGradientAscent(nav, starts, z, lm, lin, 1, resident=True)
        finally:
            loopy.ResidentIterationBound = bound


def test_sixteen_estimates_fit_a_call_seventeen_are_chunked(nav):
    lin, lm, z, _ = run_scene(nav.params, 22)
    starts = np.random.default_rng(23).normal(0, 1, (17, 6)) * SCALE
    got16 = against_host(nav, starts[:16], z, lm, lin, 1)
    poses, values, iters = np.full((17, 6), 7.0), np.full(17, 7.0), np.full(17, 7, np.int32)
    rc = nav._lib.phd_quasi_ascent(nav._h, d(np.ascontiguousarray(starts)), 17, d(np.ascontiguousarray(lin)), d(np.ascontiguousarray(lm)), len(lm),
                                   d(np.ascontiguousarray(z)), len(z), 1, 100, 0, d(poses), d(values), iters.ctypes.data_as(_lib.ip), None)
    assert rc == PHD_ERR_BAD_ARGUMENT and np.all(poses == 7) and np.all(values == 7) and np.all(iters == 7)
    got17 = nav.QuasiAscent(starts, z, lm, lin, 1)
    for x, y in zip(got17[:3], got16[:3]):
        assert np.array_equal(x[:16], y)                             # an estimate's search does not depend on its neighbours
    last = nav.QuasiAscent(starts[16:], z, lm, lin, 1)
    assert all(np.array_equal(x[16:], y) for x, y in zip(got17[:3], last[:3]))


def test_refusals(nav):
    lin, lm, z, starts = run_scene(nav.params, 61)
    args = lambda **kw: dict({"initial": starts, "measurements": z, "landmarks": lm, "linearpoint": lin}, **kw)
    from monorfs_amd.navigator import PHDError
    bad = starts.copy()
    bad[1, 2] = np.nan
    for kw in (args(initial=bad), args(linearpoint=[0, 0, 0, np.inf, 0, 0, 0]), args(average_mode=2), args(max_iterations=0), args(round_iterations=-1),
               args(measurements=np.zeros((17, 3)))):
        with pytest.raises(PHDError) as e:
            nav.QuasiAscent(**kw)
        assert e.value.status == PHD_ERR_BAD_ARGUMENT


def test_batch_calls_and_the_step_are_as_without_an_ascent(nav):
    from monorfs_amd import navigator
    lin, lm, z, starts = run_scene(nav.params, 21)
    poses7 = np.array([pose3d_add(lin, s) for s in starts])
    before = nav.QuasiSetLogLikelihood(z, lm, poses7)
    beforeg = nav.QuasiSetLogLikelihoodGradient(z, lm, poses7, 1)
    f = Frame(8, 40, 12, 81, weight_profile="steady")
    other = navigator.PHDNavigator(params(), particlecount=8)
    try:
        weights = []
        for handle, ascend in ((nav, True), (other, False)):
            handle.upload_state(f.planes(), f.counts, f.poses, f.weights)
            handle.SlamUpdate(None, f.z, u_resample=0.3)
            if ascend:
                handle.QuasiAscent(starts, z, lm, lin, 1, hessians=True)
            handle.SlamUpdate(None, f.z, u_resample=0.6)
            weights.append(handle.VehicleWeights.copy())
        assert np.array_equal(weights[0], weights[1]) and len(weights[0]) == 8
    finally:
        other.close()
        nav.reset(np.array([0, 0, 0, 1.0, 0, 0, 0]), (np.zeros(0), np.zeros((0, 3)), np.zeros((0, 3, 3))), 1)
    assert np.array_equal(nav.QuasiSetLogLikelihood(z, lm, poses7), before)
    afterg = nav.QuasiSetLogLikelihoodGradient(z, lm, poses7, 1)
    assert np.array_equal(afterg[0], beforeg[0]) and np.array_equal(afterg[1], beforeg[1])


# ---------------------------------------------------------------------------------------------- 4. the fits
def test_fit_gaussian_and_guided_mixture_resident_against_host_loop(nav):
    lin, lm, z, starts = run_scene(nav.params, 31)
    mean, cov = loopy.FitGaussian(nav, starts[0], z, lm, lin, 1, resident=True)
    wmean, wcov = loopy.FitGaussian(nav, starts[0], z, lm, lin, 1)
    assert np.allclose(mean, wmean, rtol=0, atol=1e-9), np.max(np.abs(mean - wmean))
    assert np.allclose(cov, wcov, rtol=1e-4, atol=1e-12)            # pinv of a finite-difference Hessian (eps 1e-5)
    assert np.any(cov != 0)
    model = (np.full(len(lm), 1.0001), lm, np.broadcast_to(1e-4 * np.eye(3), (len(lm), 3, 3)))
    empty, comps = loopy.GuidedFitMixture(nav, np.zeros(6), z, model, lin, 1, resident=True)
    wempty, wcomps = loopy.GuidedFitMixture(nav, np.zeros(6), z, model, lin, 1)
    assert empty == wempty
    assert len(comps) == len(wcomps) >= 1
    for (w, m, c), (ww, wm, wc) in zip(comps, wcomps):
        assert np.allclose(m, wm, rtol=0, atol=1e-9) and np.array_equal(c, wc)
        assert np.isclose(w, ww, rtol=1e-3)


# ---------------------------------------------------------------------------------------------- 5. the C++ host mirror
def test_cpp_mirror_resident_ascent_matches_the_python_host(nav, tmp_path):
    """monorfs_amd/host/Loopy.hpp with resident = true (tests/ascent_check.cpp) against PHDNavigator.QuasiAscent: the same
    device call behind both"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = _lib.build()
    exe = str(tmp_path / "ascent_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(root, "tests", "ascent_check.cpp"), so,
                           "-Wl,-rpath," + os.path.dirname(so), "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(51)
    lin, lm, z = scene(rng, nav.params, 9, 6)
    lin = pose3d_add(lin, [0.01, -0.02, 0.005, 0.02, 0.01, -0.03])
    starts = rng.normal(0, 1, (5, 6)) * SCALE
    path = tmp_path / "scene.txt"
    with open(path, "w") as fh:
        num = lambda a: " ".join("%.17g" % v for v in np.asarray(a, float).ravel())
        fh.write("%d %d %d\n%s\n%s\n%s\n%s\n" % (len(lm), len(z), len(starts), num(lm), num(z), num(lin), num(starts)))
    for mode in (0, 1):
        r = subprocess.run([exe, str(path), str(mode)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        rows = [ln.split() for ln in r.stdout.splitlines()]
        table = lambda tag: np.array([[float(v) for v in row[1:]] for row in rows if row[0] == tag])
        poses, values, iters, capped = nav.QuasiAscent(starts, z, lm, lin, mode)
        asc = table("ascent")
        assert not capped and np.all(iters >= 1)
        assert np.allclose(asc[:, 0], values, rtol=0, atol=1e-12) and np.allclose(asc[:, 1:], poses, rtol=0, atol=1e-13)
        climbing = bool(np.any(iters > 1))
        poses, values, iters, capped = nav.QuasiAscent(starts, z, lm, lin, mode, max_iterations=1)
        asc = table("bounded")
        assert capped == climbing and np.all(iters == 1) and np.allclose(asc[:, 0], values, rtol=0, atol=1e-12) and np.allclose(asc[:, 1:], poses, rtol=0, atol=1e-13)
        mean, cov = loopy.FitGaussian(nav, starts[0], z, lm, lin, mode, resident=True)
        assert np.allclose(table("fitmean")[0], mean, rtol=0, atol=1e-13)
        assert np.allclose(table("fitcovariance")[0].reshape(6, 6), cov, rtol=1e-6, atol=1e-12 * np.abs(cov).max())
