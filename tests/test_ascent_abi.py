"""The boundary of phd_quasi_ascent without a GPU: the entry points are declared, exported and bound, a NULL handle is refused
with the outputs untouched, the wrappers, hosts and documents carry the members, and the host-driven loop of
monorfs_amd/loopy.py is what it was with the defaults and truncates at max_iterations (the oracle evaluates)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from ascent_util import CountingNav, control_reference
from loopy_stub import OracleNav, scene
from monorfs_amd import _lib, loopy
from monorfs_amd.abi import PHD_ERR_BAD_ARGUMENT, prm3d_defaults
from monorfs_amd.navigator import pose3d_add

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = [4e-3, 4e-3, 4e-3, 2e-3, 2e-3, 2e-3]
# (seed, landmarks, measurements, starts, sigma): the runs of tests/test_gpu_ascent.py and the iterations per estimate of each
RUNS = {21: (10, 7, 6, 1.0, [2, 3, 3, 2, 1, 4]), 22: (10, 7, 6, 1.0, [2, 2, 3, 1, 1, 2]), 31: (6, 5, 1, 0.3, [3]), 61: (3, 2, 4, 1.0, [1, 1, 1, 1])}


def run_scene(params, seed):
    J, M, n, sigma, counts = RUNS[seed]
    rng = np.random.default_rng(seed)
    lin, lm, z = scene(rng, params, J, M, sigma=sigma)
    return lin, lm, z, rng.normal(0, 1, (n, 6)) * SCALE, counts


def ascent_before(nav, initial, measurements, landmarks, linearpoint, average_mode=0, stop_after=None):
    """loopy.LogLikeGradientAscent as it stood before `resident` and `max_iterations`, statement for statement; stop_after: leave
    the loop after that many rounds"""
    pose = np.asarray(initial, float).reshape(-1, 6).copy()
    n = len(pose)
    lin = np.asarray(linearpoint, float)
    nextpose7 = np.array([pose3d_add(lin, pose[a]) for a in range(n)])
    loglike, _ = nav.QuasiSetLogLikelihoodGradient(measurements, landmarks, nextpose7, average_mode)
    loglike = np.array(loglike)
    prevvalue = np.full(n, -np.inf)
    active = [a for a in range(n) if loglike[a] - prevvalue[a] > 1e-3]
    rounds = 0
    while active and (stop_after is None or rounds < stop_after):
        rounds += 1
        _, grad = nav.QuasiSetLogLikelihoodGradient(measurements, landmarks, nextpose7[active], average_mode)
        cand6 = np.empty((len(active), 16, 6))
        for u, a in enumerate(active):
            g = grad[u]
            size = np.linalg.norm(g)
            if size > 10.0:
                g = g * (10.0 / size)
            multiplier = 1e-2
            for c in range(16):
                cand6[u, c] = pose[a] + multiplier * g
                multiplier /= 2.0
        cand7 = np.array([[pose3d_add(lin, cand6[u, c]) for c in range(16)] for u in range(len(active))])
        vals = nav.QuasiSetLogLikelihood(measurements, landmarks, cand7.reshape(-1, 7)).reshape(len(active), 16)
        still = []
        for u, a in enumerate(active):
            c = 0
            while True:
                nextloglike = vals[u, c]
                c += 1
                if not (nextloglike < loglike[a] and c < 16):
                    break
            nextpose7[a] = cand7[u, c - 1]
            prevvalue[a] = loglike[a]
            if nextloglike > loglike[a]:
                pose[a] = cand6[u, c - 1]
                loglike[a] = nextloglike
            if loglike[a] - prevvalue[a] > 1e-3:
                still.append(a)
        active = still
    return pose, loglike


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "phdhip.h")).read()
    lib = C.CDLL(_lib.build())
    assert "int phd_quasi_ascent(phd_navigator* nav, const double* initial6, int nestimates, const double* linearpoint7," in header
    assert re.search(r"#define PHD_ASCENT_LINE\s+16\b", header)
    assert "#define PHD_API_VERSION 4" in header              # detected by symbol: no version bump
    for name, nargs in (("phd_quasi_ascent", 15), ("phd_test_ascent_control", 14)):
        assert hasattr(lib, name), "libphdhip.so does not export %s" % name
        assert name in _lib.EXPORTS
        bound = getattr(_lib.load(), name)
        assert bound.restype is C.c_int and len(bound.argtypes) == nargs
    assert "phd_ascent.h" in _lib.SOURCES
    kernels = open(os.path.join(ROOT, "monorfs_amd", "csrc", "phd_ascent.h")).read()
    for k in ("k_ascent_begin", "k_ascent_candidates", "k_ascent_select", "k_ascent_setll", "k_ascent_setll_grad"):
        assert "void %s(" % k in kernels, k


def test_null_handle_is_refused_with_the_outputs_untouched():
    lib = _lib.load()
    d = lambda a: a.ctypes.data_as(_lib.dp)
    start, lin = np.zeros((2, 6)), np.array([0, 0, 0, 1.0, 0, 0, 0])
    poses, values, iters, hess = np.full((2, 6), 7.0), np.full(2, 7.0), np.full(2, 7, np.int32), np.full((2, 6, 6), 7.0)
    rc = lib.phd_quasi_ascent(None, d(start), 2, d(lin), None, 0, None, 0, 0, 10, 0, d(poses), d(values), iters.ctypes.data_as(_lib.ip), d(hess))
    assert rc == PHD_ERR_BAD_ARGUMENT
    assert np.all(poses == 7) and np.all(values == 7) and np.all(iters == 7) and np.all(hess == 7)
    c6, c7, ch, act = np.full((2, 16, 6), 7.0), np.full((2, 16, 7), 7.0), np.full(2, 7, np.int32), np.full(2, 7, np.int32)
    rc = lib.phd_test_ascent_control(None, d(start), d(values), d(start), d(np.zeros((2, 16))), 2, d(lin), d(c6), d(c7), ch.ctypes.data_as(_lib.ip),
                                     d(poses), d(values), d(np.zeros((2, 7))), act.ctypes.data_as(_lib.ip))
    assert rc == PHD_ERR_BAD_ARGUMENT
    assert np.all(c6 == 7) and np.all(c7 == 7) and np.all(ch == 7) and np.all(act == 7)


def test_wrappers_hosts_and_documents_have_the_members():
    from monorfs_amd import navigator
    sig = inspect.signature(navigator.PHDNavigator.QuasiAscent)
    assert list(sig.parameters) == ["self", "initial", "measurements", "landmarks", "linearpoint", "average_mode", "max_iterations", "round_iterations", "hessians"]
    assert sig.parameters["round_iterations"].default == 0 and sig.parameters["hessians"].default is False
    for fn in (loopy.LogLikeGradientAscent, loopy.FitGaussian, loopy.GuidedFitMixture):
        params = inspect.signature(fn).parameters
        assert params["resident"].default is False and params["max_iterations"].default is None, fn.__name__
    assert callable(loopy.HessianToCovariance)
    hpp = open(os.path.join(ROOT, "monorfs_amd", "host", "PHDNavigator.hpp")).read()
    mirror = open(os.path.join(ROOT, "monorfs_amd", "host", "Loopy.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "HipPHDNavigator.cs")).read()
    assert "phd_quasi_ascent(nav_" in hpp and "AscentResult QuasiAscent(" in hpp
    assert "bool resident = false, int maxiterations = 0" in mirror and "nav.QuasiAscent(" in mirror and "HessianToCovariance(" in mirror
    assert "phd_quasi_ascent(HandleRef nav" in cs and "DeviceLogLikeGradientAscent(" in cs
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md", os.path.join("profiles", "ascent_cost.md")):
        assert "phd_quasi_ascent" in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "scripts", "ascent_cost.py"))
    assert os.path.exists(os.path.join(ROOT, "tests", "ascent_check.cpp"))


@pytest.mark.parametrize("seed", sorted(RUNS))
@pytest.mark.parametrize("mode", [0, 1])
def test_host_loop_with_the_defaults_is_what_it_was(seed, mode):
    params = prm3d_defaults(max_particles=256, max_components=600, max_measurements=16)
    lin, lm, z, starts, counts = run_scene(params, seed)
    stub = OracleNav(params)
    assert not hasattr(stub, "QuasiAscent")
    counting = CountingNav(stub)
    got, gotv = loopy.LogLikeGradientAscent(counting, starts, z, lm, lin, mode)
    calls = stub.calls
    want, wantv = ascent_before(stub, starts, z, lm, lin, mode)
    assert np.array_equal(got, want) and np.array_equal(gotv, wantv)
    assert stub.calls == 2 * calls and calls == 1 + 2 * max(counts)        # the same batches: one, then two per iteration
    assert list(counting.iterations()) == counts
    one, onev = loopy.LogLikeGradientAscent(stub, starts[0], z, lm, lin, mode)   # a single estimate keeps its shape
    assert one.shape == (6,) and np.array_equal(one, loopy.LogLikeGradientAscent(stub, starts[:1], z, lm, lin, mode)[0][0]) and np.ndim(onev) == 0


@pytest.mark.parametrize("k", [1, 2, 3, 4, 9])
def test_max_iterations_truncates_the_host_loop(k):
    params = prm3d_defaults(max_particles=256, max_components=600, max_measurements=16)
    lin, lm, z, starts, counts = run_scene(params, 21)
    counting = CountingNav(OracleNav(params))
    got, gotv = loopy.LogLikeGradientAscent(counting, starts, z, lm, lin, 1, max_iterations=k)
    want, wantv = ascent_before(OracleNav(params), starts, z, lm, lin, 1, stop_after=k)
    assert np.array_equal(got, want) and np.array_equal(gotv, wantv)
    assert list(counting.iterations()) == [min(k, c) for c in counts]
    if k >= max(counts):
        full, fullv = loopy.LogLikeGradientAscent(OracleNav(params), starts, z, lm, lin, 1)
        assert np.array_equal(got, full) and np.array_equal(gotv, fullv)


def test_fit_gaussian_shares_the_covariance_tail():
    """LogLikeFitCovariance is its finite-difference rows through HessianToCovariance: NaN rows give the zero matrix's
    pseudo-inverse, a positive direction carries no information"""
    params = prm3d_defaults(max_particles=256, max_components=600, max_measurements=16)
    lin, lm, z, starts, _ = run_scene(params, 31)
    stub = OracleNav(params)
    mean, cov = loopy.FitGaussian(stub, starts[0], z, lm, lin, 1)
    assert np.array_equal(cov, loopy.LogLikeFitCovariance(stub, mean, z, lm, lin, 1))
    h = -np.diag([4.0, 2.0, 1.0, 0.5, 0.25, 0.125])
    assert np.allclose(loopy.HessianToCovariance(h), np.diag(1 / np.array([4.0, 2.0, 1.0, 0.5, 0.25, 0.125])))
    h[0, 0] = 3.0
    assert loopy.HessianToCovariance(h)[0, 0] == 0
    h[1, 2] = np.nan
    assert np.array_equal(loopy.HessianToCovariance(h), np.zeros((6, 6)))


def test_control_reference_is_the_loops_line_search():
    """the numpy statement the device's control kernels are held to takes the all-rejected, the tie and the NaN branch as the
    reference's do-while does"""
    lin = np.array([0, 0, 0, 1.0, 0, 0, 0])
    values = np.array([np.full(16, -2.0), np.full(16, -1.0), [np.nan] + [0.0] * 15, [-2.0] * 7 + [-0.5] + [0.0] * 8])
    out = control_reference(np.zeros((4, 6)), np.full(4, -1.0), np.tile([6.0, 8.0, 0, 0, 0, 0], (4, 1)), values, lin)
    assert list(out[2]) == [15, 0, 0, 7] and list(out[6]) == [0, 0, 0, 1]
    assert np.array_equal(out[3][:3], np.zeros((3, 6))) and np.array_equal(out[3][3], out[0][3, 7]) and list(out[4]) == [-1, -1, -1, -0.5]
    assert np.array_equal(out[0][0, 0], [0.06, 0.08, 0, 0, 0, 0])      # norm exactly 10: not clipped
